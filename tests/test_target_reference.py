"""The numpy restatement of the spot-selection rule (tests/target_reference.py; include/rtd.h "Spots from a target") on its own, and
the host helpers of raytracedicom_amd/spots.py. No GPU: closed-form answers on a synthetic trace, and the conditions on the scene-A
fixture (tests/target_scenes.py) that the GPU comparisons of tests/test_gpu_target.py rely on, from the oracle's trace."""
import numpy as np
import pytest

import target_reference as T
import target_scenes as TS
from raytracedicom_amd import spots

W, H, S = 24, 10, 70             # rays and steps of the synthetic field: 70 steps = two words and six bits
DIMS = (64, W, H)                # dose grid (x, y, z): sample (i, j, k) is voxel (x = k, y = i, z = j); the steps 64 .. 69 leave the grid
FOOT_I, FOOT_J = (5, 12), (3, 6)  # the box target's footprint in the ray grid, inclusive
SPOTS = (10, 4)                  # spot (sx, sy) sits on ray (2 + 2 sx, 1 + 2 sy)


def _geometry():
    """A parallel beam along dose x: gantry z -> -x, gantry x -> y, gantry y -> z; 1 mm rays, steps and voxels."""
    ox, oy, oz = -12.0, -5.0, 60.0
    m = [0, 0, -1, 1, 0, 0, 0, 1, 0]
    return T.Geometry((W, H), (1.0, 1.0, -1.0), (ox, oy, oz), (np.inf, np.inf), m, (oz, -ox, -oy), SPOTS, (2.0, 2.0, -1.0), (ox + 2.0, oy + 1.0, oz), S)


def _wepl():
    return np.broadcast_to((np.arange(S, dtype=np.float32) + np.float32(1.0))[:, None, None], (S, H, W)).copy()


def _box(k_ranges):
    mask = np.zeros((DIMS[2], DIMS[1], DIMS[0]), dtype=np.uint8)
    for k0, k1 in k_ranges:
        mask[FOOT_J[0]:FOOT_J[1] + 1, FOOT_I[0]:FOOT_I[1] + 1, k0:k1 + 1] = 1
    return mask


def _footprint():
    f = np.zeros((H, W), dtype=bool)
    f[FOOT_J[0]:FOOT_J[1] + 1, FOOT_I[0]:FOOT_I[1] + 1] = True
    return f


def test_projection_and_summary_of_a_box():
    g = _geometry()
    inside = T.project(g, _box([(20, 29)]))
    want = np.zeros((S, H, W), dtype=bool)
    want[20:30] = _footprint()[None]
    np.testing.assert_array_equal(inside, want)
    assert T.summary(inside, _wepl()) == {"n_samples": 10 * 8 * 4, "wepl_min": 21.0, "wepl_max": 30.0, "ray_lo": [5, 3], "ray_hi": [12, 6],
                                         "step_lo": 20, "step_hi": 29}
    packed = T.pack(inside)
    assert packed.shape == (3, H, W) and packed.dtype == np.uint32
    assert packed[0, 4, 6] == 0x3ff00000 and packed[1, 4, 6] == 0 and packed[0, 2, 6] == 0
    # the whole grid as the target: every sample whose voxel exists, and none of the steps beyond the grid
    full = T.project(g, np.ones((DIMS[2], DIMS[1], DIMS[0]), dtype=np.uint8))
    assert full[:64].all() and not full[64:].any()
    assert T.pack(full)[2].max() == 0 and (T.pack(full)[:2] == 0xffffffff).all()
    empty = T.project(g, np.zeros((DIMS[2], DIMS[1], DIMS[0]), dtype=np.uint8))
    assert T.summary(empty, _wepl())["n_samples"] == 0


PEAKS = np.array([10, 17, 18, 19, 21, 25, 30, 31, 33, 34, 40, 64, 70, 71], dtype=np.float32)


@pytest.mark.parametrize("proximal,distal", [(0, 0), (2, 0), (0, 3), (2, 3), (1, 1)])
def test_layer_hits_of_a_box_in_water(proximal, distal):
    """wepl[k] = k + 1: a layer of integer peak depth R first reaches it at step R - 1, and the margins widen that step to
    [R - 1 - distal, R - 1 + proximal]. The box holds the steps 20 .. 29; a peak beyond wepl's last value (70) is never reached."""
    g = _geometry()
    inside = T.project(g, _box([(20, 29)]))
    hit = T.hits(inside, _wepl(), PEAKS, proximal, distal)
    for l, r in enumerate(PEAKS):
        k_lo, k_hi = int(r) - 1 - distal, min(int(r) - 1 + proximal, S - 1)
        on = k_lo < S and k_lo <= 29 and k_hi >= 20
        np.testing.assert_array_equal(hit[l], (_footprint() & on).astype(np.uint8), err_msg="peak %g" % r)
    layers = {int(r) for l, r in enumerate(PEAKS) if hit[l].any()}
    assert layers == {r for r in (10, 17, 18, 19, 21, 25, 30, 31, 33, 34, 40) if 21 - proximal <= r <= 30 + distal}


@pytest.mark.parametrize("lateral", [0.0, 1.0, 2.0, 2.5, 3.0, 100.0])
def test_spots_of_a_box_in_water(lateral):
    """A spot is selected iff the distance of its ray position to the footprint rectangle is within the lateral margin."""
    g = _geometry()
    inside = T.project(g, _box([(20, 29)]))
    hit = T.hits(inside, _wepl(), PEAKS)
    sel = T.spots(g, hit, lateral)
    assert sel.shape == (len(PEAKS), SPOTS[1], SPOTS[0]) and sel.dtype == np.uint8
    for sy in range(SPOTS[1]):
        for sx in range(SPOTS[0]):
            cx, cy = 2 + 2 * sx, 1 + 2 * sy
            dx, dy = max(FOOT_I[0] - cx, 0, cx - FOOT_I[1]), max(FOOT_J[0] - cy, 0, cy - FOOT_J[1])
            near = dx * dx + dy * dy <= lateral * lateral
            for l, r in enumerate(PEAKS):
                assert sel[l, sy, sx] == (1 if near and 21 <= r <= 30 else 0), (lateral, sx, sy, r)
    if lateral == 0.0:
        assert sel[4].sum() == 4 * 2
    if lateral == 100.0:
        assert sel[4].all() and not sel[0].any()


def test_two_slabs_along_the_beam():
    """Steps 20 .. 24 and 33 .. 37 with a gap of 8 steps. The layer of peak depth 30 reaches it at step 29, in the gap: 5 steps behind
    the first slab, 4 in front of the second."""
    g = _geometry()
    inside = T.project(g, _box([(20, 24), (33, 37)]))
    peaks = np.array([22, 30, 35], dtype=np.float32)
    zero = T.hits(inside, _wepl(), peaks)
    assert zero[0].any() and not zero[1].any() and zero[2].any()
    for p in range(7):
        for d in range(7):
            got = bool(T.hits(inside, _wepl(), peaks, p, d)[1].any())
            assert got == (p >= 4 or d >= 5), (p, d)
            if p + d >= 8:
                assert got
    sel = T.spots(g, T.hits(inside, _wepl(), peaks, 4, 0), 0.0)
    assert sel[1].sum() == 4 * 2 == sel[0].sum()


# ------------------------------------------------------------------------------------------------------------- an oracle trace

@pytest.fixture(scope="module")
def scene_a(orc, synth):
    scn = TS.scene(synth, "A")
    dose = np.zeros(scn.dose_shape, dtype=np.float32)
    of = orc.run_field(scn, scn.beams[0], dose, options=TS.options(), keep_layers=True, dose_dims=scn.dose_dims)
    assert of.status == 0, of.error
    g = T.geometry_of(of.info, scn.beams[0])
    wepl = of.get("wepl").reshape(g.S, g.H, g.W)
    peaks = of.get("layer_plan").reshape(-1, 8)[:, 2].copy()
    of.close()
    return scn, g, wepl, peaks, TS.target(scn, g, wepl, peaks)


def test_oracle_trace_of_scene_a(scene_a):
    """Oblique, divergent, coarse dose grid, 300 steps (the last word is partial), 9 x 7 spots, 8 layers, an ellipsoid at the depth
    between the peaks of layers 2 and 5."""
    scn, g, wepl, peaks, mask = scene_a
    assert (g.W, g.H, g.S) == (128, 80, 300) and len(peaks) == 8
    assert (np.diff(wepl, axis=0) >= 0).all()                         # what lets the engine count by bisection
    inside, info, hit0, sel0 = T.select(g, mask, wepl, peaks)
    assert info["n_samples"] > 5000 and inside.any(axis=0).sum() > 400
    assert peaks[0] < info["wepl_min"] < info["wepl_max"] < peaks[7]
    packed = T.pack(inside)
    assert int(sum(bin(int(w)).count("1") for w in packed.ravel()[packed.ravel() != 0])) == info["n_samples"]
    assert (packed[-1] >> np.uint32(S_LAST_BITS)).max() == 0
    n_spots = sel0.shape[1] * sel0.shape[2]
    per_layer = sel0.sum(axis=(1, 2))
    assert n_spots == 63
    assert ((per_layer >= 0.1 * n_spots) & (per_layer <= 0.5 * n_spots)).sum() >= 2, per_layer
    assert (per_layer == 0).sum() >= 4, per_layer
    _, _, hit1, sel1 = T.select(g, mask, wepl, peaks, 6.0, 2.0, 5.0)
    assert (sel1 >= sel0).all() and (hit1 >= hit0).all()
    wider = sel1.sum(axis=(1, 2))
    assert (wider[per_layer > 0] > per_layer[per_layer > 0]).all(), (per_layer, wider)


S_LAST_BITS = 300 - 32 * 9       # the bits of the last word that stand for steps


# ------------------------------------------------------------------------------------------------------------------ spots.py

def test_energies_for_range(synth):
    lo, hi, spacing = 52.0, 97.0, 4.0
    e = spots.energies_for_range(synth, lo, hi, spacing)
    assert e.dtype == np.float32 and e.size == 12 and (np.diff(e) > 0).all()
    idx = np.interp(e, synth.energiesPerU, np.arange(synth.nEnergies))
    peak = np.interp(idx, np.arange(synth.nEnergies), synth.peakDepths)
    assert abs(peak[-1] - hi) <= 1e-3 and lo - 1e-3 <= peak[0] <= lo + spacing
    np.testing.assert_allclose(np.diff(peak), spacing, atol=1e-3)
    assert spots.energies_for_range(synth, 60.0, 60.0, 3.0).size == 1
    with pytest.raises(ValueError):
        spots.energies_for_range(synth, 60.0, 50.0, 3.0)


def test_spot_grid_covers_the_ray_box():
    field_info = {"ray_res": [0.5, 0.75, -1.0], "ray_offset": [-40.0, -30.0, 110.0]}
    target_info = {"ray_lo": [79, 36], "ray_hi": [145, 67]}
    for pitch, margin in ((5.0, 0.0), ((7.0, 5.0), 6.0), (3.0, 2.5)):
        nx, ny, ox, oy = spots.spot_grid_for(field_info, target_info, pitch, margin)
        px, py = (pitch, pitch) if np.isscalar(pitch) else pitch
        for a, (n, o, p) in enumerate(((nx, ox, px), (ny, oy, py))):
            lo = field_info["ray_offset"][a] + field_info["ray_res"][a] * target_info["ray_lo"][a] - margin
            hi = field_info["ray_offset"][a] + field_info["ray_res"][a] * target_info["ray_hi"][a] + margin
            assert n >= 1 and o <= lo + 1e-9 and o + (n - 1) * p >= hi - 1e-9
            assert (n - 1) * p < (hi - lo) + p                        # and no wider than it has to be


def test_oracle_trace_of_two_slabs_in_water(orc, synth):
    """Scene U (a parallel beam square onto a water box) with the hollow target of target_scenes.two_slabs: the peaks of layers 3 and 4
    fall into the gap on every ray, those of layers 2 and 5 into the two parts. Margins of 8 mm either way reach across."""
    scn = TS.scene(synth, "U")
    dose = np.zeros(scn.dose_shape, dtype=np.float32)
    of = orc.run_field(scn, scn.beams[0], dose, options=TS.options(), keep_layers=True, dose_dims=scn.dose_dims)
    assert of.status == 0, of.error
    g = T.geometry_of(of.info, scn.beams[0])
    wepl = of.get("wepl").reshape(g.S, g.H, g.W)
    peaks = of.get("layer_plan").reshape(-1, 8)[:, 2].copy()
    of.close()
    mask = TS.two_slabs(scn, g, wepl, peaks)
    _, _, _, sel0 = T.select(g, mask, wepl, peaks)
    n0 = sel0.sum(axis=(1, 2))
    assert n0[2] > 0 and n0[3] == 0 and n0[4] == 0 and n0[5] > 0, n0
    prox = T.select(g, mask, wepl, peaks, 0.0, 8.0, 0.0)[3].sum(axis=(1, 2))
    dist = T.select(g, mask, wepl, peaks, 0.0, 0.0, 8.0)[3].sum(axis=(1, 2))
    both = T.select(g, mask, wepl, peaks, 0.0, 8.0, 8.0)[3].sum(axis=(1, 2))
    assert prox[3] == 0 and prox[4] > 0 and dist[3] > 0 and dist[4] == 0 and both[3] > 0 and both[4] > 0, (prox, dist, both)
