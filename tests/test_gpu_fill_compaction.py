"""GPU tests of k_fill's lane placement ("Lane placement").

The fill deals a tile's rays to the lanes of its block by segments of SEG consecutive rays, the segments with a live ray first, and
a wave without a live ray only stores. Which lane walks which ray changes nothing in the per-ray arithmetic, so a field created
under RTD_NO_FILL_COMPACT (the identity placement, same kernel) must agree with a default field of the same beam TO THE BIT, in
everything the fill writes and in everything computed from it: no tolerance anywhere in this file."""
import numpy as np
import pytest

from gpu_support import FieldRig, options
from raytracedicom_amd import abi, luts, scenarios

pytestmark = pytest.mark.gpu

SEG = 16                # rtd_fill.hpp: kFillSeg
SEGS_PER_WAVE = 64 // SEG
SEGS_PER_TILE = 256 // SEG

_FETCHED = ("idd", "rsigma", "first_passive", "tile_radius", "active", "bev", "eff_radius", "layer_plan", "ray_weights")


def _thinned(scn, share, seed=5):
    """The scenario with a seeded random share of its beam's spot weights set to 0."""
    if share:
        w = scn.beams[0].spotWeights
        w[np.random.default_rng(seed).random(w.shape) < share] = 0.0
    return scn


def _scene(synth, k):
    if k == 1:
        return scenarios.hetero_ct(synth, n=96, spots=(5, 3), pitch=(7.0, 5.0), n_layers=3)
    if k == 2:
        return _thinned(scenarios.hetero_ct(synth, n=96, spots=(6, 6), pitch=5.0, n_layers=4), 0.5)
    if k == 3:
        return _thinned(scenarios.hetero_ct(synth, n=96, spots=(3, 7), pitch=(9.0, 4.0), n_layers=3, ray_spacing=(0.75, 1.5)), 0.3)
    if k == 4:
        return _thinned(scenarios.hetero_ct(synth, n=96, spots=(6, 6), pitch=5.0, n_layers=2, angles=[30.0]), 0.4)
    if k == 5:
        return scenarios.hetero_ct(synth, n=96, spots=(12, 4), pitch=6.0, n_layers=2)
    if k == 6:
        return scenarios.water_cube(synth, n=64, n_layers=3, spots=9, pitch=5.0)
    if k == 8:
        scn = scenarios.hetero_ct(synth, n=96, spots=(5, 5), pitch=6.0, n_layers=2)
        scn.beams[0].spotWeights[:] = 1e-3                            # every ray weight below the cut-off of 1
        return scn
    raise ValueError(k)


def _compute(rig, beam, **env):
    """One field of the beam, created with the given RTD_* switches in the environment, computed into a zeroed volume: everything
    the comparison looks at."""
    f = rig.field(beam, **env)
    dose, info, _ = rig.compute(f)
    out = {"info": info, "dose": dose}
    for nm in _FETCHED:
        out[nm] = f.fetch(nm).copy()
    # idd and rsigma: the steps the fill walks, [entry step, the layer's last step) — it writes nothing outside them
    W, H, L = info["ray_dims"]
    plan = out["layer_plan"].reshape(L, 8)
    for nm in ("idd", "rsigma"):
        v = out[nm].reshape(L, beam.tracerSteps, H, W)
        out[nm] = np.concatenate([v[l, info["beam_first_inside"]:int(plan[l, 5])].ravel() for l in range(L)])
    return out


def _both_layouts(engine, scn, opt):
    rig = FieldRig(engine, scn, opt)
    try:
        new = _compute(rig, scn.beams[0])
        old = _compute(rig, scn.beams[0], RTD_NO_FILL_COMPACT="1")
    finally:
        rig.close()
    assert new["info"] == old["info"]
    for nm in ("dose",) + _FETCHED:
        np.testing.assert_array_equal(new[nm], old[nm], err_msg=nm)
    return new


def _live_segments(out, cutoff=1.0):
    """Per (layer, tile): how many of the tile's segments hold a ray whose weight is not below the cut-off."""
    W, H, L = out["info"]["ray_dims"]
    live = out["ray_weights"].reshape(L, H // 8, 8, W // 32, 32 // SEG, SEG) >= cutoff
    return live.any(axis=5).sum(axis=(2, 4)).reshape(-1)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_heterogeneous_scenes(engine, synth, k):
    """Partly live tiles of every kind (test_scenes_cover_the_tile_states says which), oblique gantry, anisotropic ray spacing."""
    out = _both_layouts(engine, _scene(synth, k), options(1.0))
    assert out["dose"].max() > 0 and out["info"]["uniform_sigma"] == 0
    if k == 5:
        assert out["info"]["max_radius"] > 16                         # the second sweep launch runs behind this fill


def test_water_cube(engine, synth):
    """The uniform-sigma tracking of the sigma walk (sigMin / sigMax, nonUniform) and the separable superposition behind it."""
    out = _both_layouts(engine, _scene(synth, 6), options(1.0))
    assert out["dose"].max() > 0 and out["info"]["uniform_sigma"] == 1


def test_nuclear_corr(engine):
    """k_fill<*, true>: the halo's planes reach the comparison through the dose volume."""
    scn = scenarios.water_cube(luts.synth_luts(nuclear=True), n=64, n_layers=3, spots=7, pitch=6.0)
    out = _both_layouts(engine, scn, options(1.0, nuclear=abi.RTD_NUC_SOUKUP))
    assert out["dose"].max() > 0


def test_all_rays_below_the_cutoff(engine, synth):
    """Every wave is dead from the start: the fill only stores, and the result is zeros."""
    out = _both_layouts(engine, _scene(synth, 8), options(1.0))
    assert _live_segments(out).max() == 0
    assert out["dose"].max() == 0 and (out["idd"] == 0).all() and np.isinf(out["rsigma"]).all()


def test_scenes_cover_the_tile_states(engine, synth):
    """A condition on the inputs: scenes 1-5 together hold an empty tile, a tile with fewer live segments than one wave takes, a
    tile whose live segments do not fill whole waves, and a fully live tile — so that a later change of a scene cannot make the
    comparisons above pass over nothing."""
    counts = []
    with engine.Engine(0) as eng:
        eng.set_options(options(1.0))
        eng.set_luts(synth)
        for k in (1, 2, 3, 4, 5):
            scn = _scene(synth, k)
            eng.set_ct(scn.ct)
            f = eng.create_field(scn.beams[0], scn.dims)
            try:
                f.compute_bev()
                _, info = f.finish()
                counts.append(_live_segments({"info": info, "ray_weights": f.fetch("ray_weights")}))
            finally:
                f.destroy()
    n = np.concatenate(counts)
    print("live segments per (layer, tile):", dict(zip(*[a.tolist() for a in np.unique(n, return_counts=True)])))
    assert (n == 0).any()
    assert ((n > 0) & (n < SEGS_PER_WAVE)).any()
    assert ((n > SEGS_PER_WAVE) & (n % SEGS_PER_WAVE != 0)).any()
    assert (n == SEGS_PER_TILE).any()
