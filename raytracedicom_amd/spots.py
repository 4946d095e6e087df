"""From a target to the spot map of a field: host helpers around Field.project_target / Field.select_spots (include/rtd.h "Spots
from a target").

    energies_for_range   the layer energies whose Bragg peaks cover a range of water-equivalent depths
    spot_grid_for        a regular spot grid over the target's footprint in the ray grid
    place_spots          candidate beam -> compute, project, select -> the beam of the selected spots

The decisions are the engine's (rtd_field_select_spots); this module only shapes its inputs and crops its output."""
import math

import numpy as np

from . import scenarios


def energies_for_range(luts, wepl_lo, wepl_hi, spacing_mm):
    """Ascending float32 energies (MeV/u) whose peak depths step from wepl_hi down to wepl_lo in steps of spacing_mm: depth
    wepl_hi - n * spacing_mm for n = 0 .. floor((wepl_hi - wepl_lo) / spacing_mm), each turned into an energy by inverse linear
    interpolation of luts.peakDepths over luts.energiesPerU. Depths outside the table are clamped to it; energies that coincide
    after rounding are kept once."""
    if not (spacing_mm > 0.0) or not (wepl_hi >= wepl_lo):
        raise ValueError("spacing_mm must be positive and wepl_hi >= wepl_lo")
    n = int(math.floor((float(wepl_hi) - float(wepl_lo)) / float(spacing_mm))) + 1
    depths = float(wepl_hi) - float(spacing_mm) * np.arange(n, dtype=np.float64)
    peaks = np.asarray(luts.peakDepths, dtype=np.float64)
    energies = np.interp(depths, peaks, np.asarray(luts.energiesPerU, dtype=np.float64))
    return np.unique(energies.astype(np.float32))


def spot_grid_for(field_info, target_info, pitch, margin_mm=0.0):
    """(nx, ny, offset_x, offset_y) of a regular spot grid of `pitch` (mm; a number or a pair) that covers the target's ray box
    (target_info ray_lo / ray_hi, as Field.project_target returns them) widened by margin_mm on every side. The offsets are the
    gantry coordinates of spot (0, 0) at the isocentre plane: what spotIdxToGantry.offset[0:2] takes. Spot positions are ray
    positions rounded outwards, so the first and last spot of a row lie on or outside the widened box."""
    px, py = (float(pitch), float(pitch)) if np.isscalar(pitch) else (float(pitch[0]), float(pitch[1]))
    out = []
    for a, p in ((0, px), (1, py)):
        res, off = float(field_info["ray_res"][a]), float(field_info["ray_offset"][a])
        lo = off + res * float(target_info["ray_lo"][a]) - float(margin_mm)
        hi = off + res * float(target_info["ray_hi"][a]) + float(margin_mm)
        n = int(math.ceil((hi - lo) / p - 1e-9)) + 1
        start = 0.5 * (lo + hi) - 0.5 * (n - 1) * p             # centred on the box
        out.append((n, start))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def place_spots(eng, beam, mask, dose_dims, lateral=0.0, proximal=0.0, distal=0.0):
    """The beam of the spots of candidate `beam` (a scenarios.BeamSettings: its spot grid and energies are what is on offer) that
    belong to the target `mask` (what Field.project_target takes) on the dose grid dose_dims (x, y, z), or None if no spot does.
    The candidate is computed once on `eng` (CT and LUTs set), the target projected and the spots selected with the three margins
    (mm; lateral in the isocentre plane, proximal / distal water-equivalent). In the result the layers without a spot are dropped, the
    grid is cropped to the box of the selected spots (spotIdxToGantry.offset shifted accordingly), and the weights are the selection
    as 0.0 / 1.0: unselected spots inside the box stay in the map with weight 0."""
    n = int(dose_dims[0]) * int(dose_dims[1]) * int(dose_dims[2])
    f = eng.create_field(beam, dose_dims)
    d = eng.device_alloc(4 * n)
    try:
        eng.device_zero(d, 4 * n)
        f.compute(d)
        f.finish()
        f.project_target(mask)
        sel = f.select_spots(lateral, proximal, distal)
    finally:
        f.destroy()
        eng.device_free(d)
    if not sel.any():
        return None
    layers = np.flatnonzero(sel.any(axis=(1, 2)))
    rows = np.flatnonzero(sel.any(axis=(0, 2)))
    cols = np.flatnonzero(sel.any(axis=(0, 1)))
    y0, y1, x0, x1 = int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])
    weights = sel[layers][:, y0:y1 + 1, x0:x1 + 1].astype(np.float32)
    t = beam.spotIdxToGantry
    shifted = scenarios.Float3IdxTransform(t.delta, (t.offset[0] + x0 * t.delta[0], t.offset[1] + y0 * t.delta[1], t.offset[2]))
    return beam.replace(spotWeights=weights, beamEnergies=beam.beamEnergies[layers], spotSigmas=beam.spotSigmas[layers], spotIdxToGantry=shifted)
