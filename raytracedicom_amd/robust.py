"""Error scenarios for robust optimisation (Engine.create_robust_optimizer, include/rtd.h "Robust spot-weight optimisation").

A scenario is an ordinary list of fields whose matrices are computed under an error. Two kinds can be made with what exists:

  set-up error   shifted_beam(beam, shift_mm): the patient displaced by shift_mm in gantry coordinates, the spot map untouched;
  range error    range_scaled_luts(es, factor): LUTs whose stopping-power table is scaled, so every water-equivalent depth scales.

The recipe (the matrix lives with its field and survives the next set_luts, so one engine serves every range factor in turn):

    eng.set_options(opts)                  # ray_weight_cutoff = 0: the matrix needs it
    eng.set_ct(ct)
    scenario_fields = []
    for factor, shifts in ((1.0, [(0, 0, 0), (3, 0, 0), (-3, 0, 0)]), (0.965, [(0, 0, 0)]), (1.035, [(0, 0, 0)])):
        eng.set_luts(es if factor == 1.0 else range_scaled_luts(es, factor))
        for shift in shifts:
            fields = [eng.create_field(b, dose_dims) for b in scenario_beams(beams, [shift])[0]]
            for f in fields:
                f.dose_influence()
            scenario_fields.append(fields)     # scenario 0: factor 1, no shift -- the nominal one
    opt = eng.create_robust_optimizer(scenario_fields, objective, abi.RTD_ROBUST_WORST_CASE)
    opt.run(100)
    values, lambdas, worst = opt.scenario_values()
"""
import copy

import numpy as np

from .scenarios import BeamSettings, Float3AffineTransform


def _shifted(t, shift):
    """T' with T'(g) = T(g - shift): the same matrix, the offset moved by -m shift."""
    return Float3AffineTransform(t.m, t.v - t.m @ shift)


def shifted_beam(beam, shift_mm):
    """The beam as it sees a patient displaced by shift_mm (x, y, z in gantry coordinates, the unit of the geometry): both
    gantryToImIdx and gantryToDoseIdx are composed with the translation, T'(g) = T(g - shift). The spot map, energies, sigmas and
    every other member are shared with `beam`, not copied."""
    shift = np.asarray(shift_mm, dtype=np.float64).reshape(3)
    b = copy.copy(beam)
    assert isinstance(b, BeamSettings)
    b.gantryToImIdx = _shifted(beam.gantryToImIdx, shift)
    b.gantryToDoseIdx = b.gantryToImIdx if beam.gantryToDoseIdx is beam.gantryToImIdx else _shifted(beam.gantryToDoseIdx, shift)
    return b


def range_scaled_luts(es, factor):
    """A copy of the EnergyStruct whose stopping-power table is float32(spVector * factor): every water-equivalent path length, and
    with it every range, scales by `factor` (1.035: 3.5 % denser, the beam stops 3.5 % earlier). Nothing else changes; the other
    arrays are shared with `es`."""
    out = copy.copy(es)
    out.spVector = np.ascontiguousarray((es.spVector * np.float32(factor)).astype(np.float32))
    return out


def scenario_beams(beams, shifts):
    """One beam list per shift: [[shifted_beam(b, s) for b in beams] for s in shifts]. A zero shift gives the beams themselves."""
    out = []
    for s in shifts:
        s = np.asarray(s, dtype=np.float64).reshape(3)
        out.append(list(beams) if not s.any() else [shifted_beam(b, s) for b in beams])
    return out
