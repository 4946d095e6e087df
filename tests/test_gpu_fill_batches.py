"""GPU tests of k_fill's batches ("The waits of a batch, corrected").

Both walks take kFillBatch = 8 steps per batch; the replaying build reads the per-step constants of a batch from the block's copy of
the step table, runs the full batches in a loop of their own with the layer's last batch behind it, and refills every prefetch slot
for the step one batch later. What can go wrong is a matter of where a layer's steps begin and end against
the batches and against the end of the tables, so every scene here is chosen (with the CPU oracle) for the step counts of its layers,
c = afterLast - beam_first_inside, and asserts from the fetched info and layer_plan that it still has them: a change of the scene
generator then fails the test instead of emptying it.

Every comparison is bitwise, as in test_gpu_sigma_reuse.py: the computes of one field — walked, recorded and replayed, replayed,
replayed (sigma_reused 0, 1, 2, 2) — against a field created under RTD_NO_SIGMA_REUSE (every compute walks) and one under
RTD_NO_TRACE_REUSE (every compute traces, plans and walks). idd and rsigma are compared over the steps the fill writes,
[beam_first_inside, afterLast of the layer), bev over the slices the superposition writes.

The planner never gives afterLast = S: findFirstLargerOrdered returns S - 1 at the most (as the reference's does). The scenes of the
end of the table therefore have afterLast = S - 1, the largest there is: the read-ahead of the last batches runs past the step table
and past the record there all the same."""
import numpy as np
import pytest

from gpu_support import FieldRig, bits, hetero_scene, options, rig_fixture
from raytracedicom_amd import luts

pytestmark = pytest.mark.gpu

_FETCHED = ("bev", "idd", "rsigma", "tile_radius", "eff_radius", "layer_plan", "first_passive", "active")

rig_of = rig_fixture(FieldRig)


def _compute(rig, f, names=_FETCHED):
    """One compute with a finish: (sigma_reused, {dose, info, the fetched arrays})."""
    dose, info, _ = rig.compute(f)
    out = {"info": info, "dose": dose}
    for nm in names:
        out[nm] = f.fetch(nm).copy()
    return int(f.fetch("sigma_reused")[0]), out


def _steps(out):
    """(beam_first_inside, afterLast per layer) of a result."""
    info = out["info"]
    plan = out["layer_plan"].reshape(info["ray_dims"][2], 8)
    return info["beam_first_inside"], [int(a) for a in plan[:, 5]]


def _written(out, nm):
    """The part of a fetched array that the compute wrote, as bit patterns where it holds floats."""
    a = out[nm]
    if nm in ("idd", "rsigma", "bev"):
        info = out["info"]
        first, after = _steps(out)
        if nm == "bev":
            S = a.size // ((info["ray_dims"][0] + 64) * (info["ray_dims"][1] + 64))
            return bits(a.reshape(S, -1)[first:max(info["beam_first_calculated_passive"], first)])
        W, H, L = info["ray_dims"]
        a = a.reshape(L, -1, H, W)
        return np.concatenate([bits(a[l, first:max(after[l], first)]).reshape(-1) for l in range(L)])
    return bits(a) if a.dtype == np.float32 else a


def _same(a, b):
    assert a["info"] == b["info"]
    np.testing.assert_array_equal(bits(a["dose"]), bits(b["dose"]), err_msg="dose")
    for nm in _FETCHED:
        np.testing.assert_array_equal(_written(a, nm), _written(b, nm), err_msg=nm)


def _runs(rig, beam, expect, **env):
    """len(expect) computes of one field with a finish in between -> their results, after the check of what sigma_reused read."""
    f = rig.field(beam, **env)
    runs = [_compute(rig, f) for _ in expect]
    assert tuple(r for r, _ in runs) == tuple(expect)
    return [out for _, out in runs]


def _four_against_walking(rig, beam):
    """Walked, recorded and replayed, replayed, replayed against the field that walks and the one that traces, plans and walks ->
    the walked result."""
    outs = _runs(rig, beam, (0, 1, 2, 2))
    walked = _runs(rig, beam, (0, 0), RTD_NO_SIGMA_REUSE="1")
    traced = _runs(rig, beam, (0,), RTD_NO_TRACE_REUSE="1")
    for out in outs + walked[1:] + traced:
        _same(out, walked[0])
    assert walked[0]["dose"].max() > 0
    return walked[0]


# name -> (CT size, gantry angle, layers, tracer steps)
_SCENES = {
    "even_first": (96, 0.0, 5, 512),
    "odd_first": (128, 37.0, 5, 512),
    "table_end": (128, 0.0, 5, 162),
    "short": (128, 0.0, 3, 6),
}


@pytest.mark.parametrize("case", sorted(_SCENES))
def test_step_counts(rig_of, synth, case):
    """The step counts of the layers against the batch of 8 (full batches in a loop of their own, the last batch behind it), the parity of the
    table offset, and the end of the tables:
      even_first  beam_first_inside even; a layer with c = 8 mod 16 (an odd number of full batches, no tail), one with c = 7 mod 8
      odd_first   beam_first_inside odd; a layer with c = 1 mod 8, one with c = 8 mod 16
      table_end   layers that end at the last step the planner gives (afterLast = S - 1), with c = 0 mod 16 (an even number of
                  full batches, no tail): the read-ahead of their last batch lies wholly behind the step table and the record
      short       every layer has 0 < c < 8 (one tail batch, nothing else) and ends at S - 1"""
    n, deg, layers, steps = _SCENES[case]
    scn = hetero_scene(synth, n, [deg], spots=7, pitch=6.0, layers=layers, steps=steps)
    rig = rig_of(scn, options(1.0))
    first, after = _steps(_four_against_walking(rig, scn.beams[0]))
    c = [a - first for a in after]
    assert all(x > 0 for x in c), (first, after)
    if case == "even_first":
        assert first % 2 == 0 and any(x % 16 == 8 for x in c) and any(x % 8 == 7 for x in c), (first, after)
    elif case == "odd_first":
        assert first % 2 == 1 and any(x % 8 == 1 for x in c) and any(x % 16 == 8 for x in c), (first, after)
    elif case == "table_end":
        assert any(a == steps - 1 and (a - first) % 16 == 0 for a in after), (first, after)
    else:
        assert all(x < 8 for x in c) and all(a == steps - 1 for a in after), (first, after)


@pytest.mark.parametrize("dose_to_water", [0, 1])
def test_carried_dose(rig_of, synth, dose_to_water):
    """The phantom's air cavity lies inside the patient: on its steps the mass of a step is at most 1e-2 (a parallel beam with rays
    1 mm apart and steps of 1 mm: the step volume is 1, so the mass is the density, or the step of the water-equivalent depth under
    dose_to_water), and the dose walk keeps the value of the step before. Such (ray, step) exist, with a dose above zero."""
    scn = hetero_scene(synth, 128, [0.0], spots=7, pitch=6.0, layers=3)
    opt = options(1.0)
    opt.dose_to_water = dose_to_water
    rig = rig_of(scn, opt)
    ref = _four_against_walking(rig, scn.beams[0])
    W, H, L = ref["info"]["ray_dims"]
    S = scn.beams[0].tracerSteps
    first, after = _steps(ref)
    f = rig.field(scn.beams[0])
    _compute(rig, f)
    thick = f.fetch("density").reshape(S, H, W)
    if dose_to_water:
        wepl = f.fetch("wepl").reshape(S, H, W)
        thick = np.concatenate([wepl[:1], wepl[1:] - wepl[:-1]])
    idd = ref["idd"].reshape(L, S, H, W)
    carried = 0
    for l in range(L):
        cur, prev = idd[l, first + 1:after[l]], idd[l, first:after[l] - 1]
        carried += int(((thick[first + 1:after[l]] <= 1e-2) & (cur > 0) & (bits(cur) == bits(prev))).sum())
    assert carried > 0


def _resampled(es, n):
    """The tables with the cumulative-IDD rows resampled to n samples (linear; the scale factors follow)."""
    x = np.arange(n, dtype=np.float64) * (es.nEnergySamples - 1) / (n - 1)
    cidd = np.stack([np.interp(x, np.arange(es.nEnergySamples), es.ciddMatrix[i].astype(np.float64)) for i in range(es.nEnergies)])
    scale = es.scaleFacts.astype(np.float64) * (n - 1) / (es.nEnergySamples - 1)
    return luts.EnergyStruct(es.energiesPerU, es.peakDepths, scale, cidd, es.densityScaleFact, es.densityVector, es.spScaleFact,
                             es.spVector, es.rRlScaleFact, es.rRlVector)


def test_lut_rows_beyond_lds(rig_of, synth):
    """Rows of 7424 samples: two of them (58 KiB) do not fit the block's LDS, the dose walk reads them from memory
    (k_fill<false, false, *>) while the step table is still the block's copy."""
    big = _resampled(synth, 7424)
    assert 2 * big.nEnergySamples * 4 > 56 * 1024
    scn = hetero_scene(big, 96, [0.0], spots=5, pitch=8.0, layers=2)
    rig = rig_of(scn, options(1.0))
    first, after = _steps(_four_against_walking(rig, scn.beams[0]))
    assert all(a - first > 8 and (a - first) % 8 != 0 for a in after), (first, after)      # full batches and a tail
