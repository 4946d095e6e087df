"""GPU tests of the sigma record a field keeps between computes ("The sigma record").

The first compute that reuses a field's trace records what k_fill's sigma walk computes without looking at the spot weights; the
computes after it replay the record under their own weights. Nothing is reordered: every comparison here is bitwise
(assert_array_equal, floats through their bit patterns), against a field created under RTD_NO_SIGMA_REUSE (every compute walks) and
against one created under RTD_NO_TRACE_REUSE (every compute traces, plans and walks).

idd and rsigma are compared over the steps the fill writes, [beam_first_inside, afterLast of the layer), and bev over the slices the
superposition writes, [beam_first_inside, beam_first_calculated_passive): outside of them a buffer holds what it held before."""
import math

import numpy as np
import pytest

from gpu_support import FieldRig, bits, hetero_scene, options, rig_fixture
from raytracedicom_amd import abi, luts, scenarios

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


def _written(out, nm):
    """The part of a fetched array that the compute wrote, as bit patterns where it holds floats."""
    a = out[nm]
    if nm in ("idd", "rsigma", "bev"):
        info = out["info"]
        first = info["beam_first_inside"]
        if nm == "bev":
            S = a.size // ((info["ray_dims"][0] + 64) * (info["ray_dims"][1] + 64))
            return bits(a.reshape(S, -1)[first:max(info["beam_first_calculated_passive"], first)])
        W, H, L = info["ray_dims"]
        plan = out["layer_plan"].reshape(L, 8)
        a = a.reshape(L, -1, H, W)
        return np.concatenate([bits(a[l, first:max(int(plan[l, 5]), first)]).reshape(-1) for l in range(L)])
    return bits(a) if a.dtype == np.float32 else a


def _same(a, b, names=_FETCHED):
    assert a["info"] == b["info"]
    np.testing.assert_array_equal(bits(a["dose"]), bits(b["dose"]), err_msg="dose")
    for nm in names:
        np.testing.assert_array_equal(_written(a, nm), _written(b, nm), err_msg=nm)


def _runs(rig, beam, n, expect, **env):
    """n computes of one field with a finish in between -> their results, after the check of what sigma_reused read."""
    f = rig.field(beam, **env)
    runs = [_compute(rig, f) for _ in range(n)]
    assert tuple(r for r, _ in runs) == tuple(expect)
    return f, [out for _, out in runs]


def _against_walking(rig, beam, outs, **env):
    """The results against a field that reuses its trace but walks, and against one that traces, plans and walks every time."""
    _, walked = _runs(rig, beam, 2, (0, 0), **dict(env, RTD_NO_SIGMA_REUSE="1"))
    _, traced = _runs(rig, beam, 1, (0,), **dict(env, RTD_NO_TRACE_REUSE="1"))
    for out in outs + walked[1:] + traced:
        _same(out, walked[0])


def _missing(synth, n=128):
    """A beam 1 m beside the volume: every sample is BORDER zero, the field is empty."""
    ct, voxel = scenarios.hetero_phantom(n)
    beam = scenarios.make_field(synth, n, voxel, (872.0, -128.0, -106.0), 0.0, 7, 6.0, 3, 5)
    return scenarios.Scenario("beam beside the volume", synth, ct, (voxel,) * 3, [beam])


def _set_weights(rig, f, w):
    dW = rig.eng.device_alloc(w.nbytes)
    try:
        rig.eng.to_device(dW, w)
        f.set_spot_weights(dW)
    finally:
        rig.eng.sync()
        rig.eng.device_free(dW)


@pytest.mark.parametrize("case", ["across", "diagonal", "along", "water", "missing"])
def test_four_computes(rig_of, synth, case):
    """Walked, recorded and replayed, replayed, replayed: the three sampling geometries (0 degrees; 37 degrees with a finite source
    distance; 90 degrees), water (still detected uniform, still on the uniform path) and an empty field."""
    if case == "water":
        scn = scenarios.water_cube(synth, n=64, n_layers=3, spots=7, pitch=6.0)
    elif case == "missing":
        scn = _missing(synth)
    else:
        deg, dist = {"across": (0.0, (math.inf, math.inf)), "diagonal": (37.0, (2000.0, 2500.0)), "along": (90.0, (math.inf, math.inf))}[case]
        scn = hetero_scene(synth, 128, [deg], source_dist=dist, spots=7, pitch=6.0)
    rig = rig_of(scn, options(1.0))
    f, outs = _runs(rig, scn.beams[0], 4, (0, 1, 2, 2))
    assert int(f.fetch("trace_reused")[0]) == 1
    _against_walking(rig, scn.beams[0], outs)
    for out in outs:
        if case == "water":
            assert out["info"]["uniform_sigma"] == 1 and out["dose"].max() > 0
        elif case == "missing":
            assert out["dose"].max() == 0 and out["info"]["live_steps"] == 0
        else:
            assert out["info"]["uniform_sigma"] == 0 and out["dose"].max() > 0


@pytest.mark.parametrize("cutoff", [0.0, 1.0])
def test_revive_and_kill(rig_of, synth, cutoff):
    """The record is made under weights that kill two spot rows (below a cut-off of 1), then replayed under weights that revive
    them and kill two others, then under weights with every spot alive: each result equals a fresh field with those weights. What
    the record holds for a ray must not depend on the weight the ray had when it was recorded."""
    scn = hetero_scene(synth, 128, [15.0], spots=7, pitch=6.0)
    b = scn.beams[0]
    w3 = b.spotWeights.copy()
    w1, w2 = w3.copy(), w3.copy()
    w1[:, :2, :] = 0.5
    w2[:, -2:, :] = 0.5
    rig = rig_of(scn, options(cutoff))
    f = rig.field(b.replace(spotWeights=w1))
    assert _compute(rig, f)[0] == 0
    r, first = _compute(rig, f, _FETCHED + ("ray_weights",))
    assert r == 1
    seen = {}
    for name, w in (("w1", w1), ("w2", w2), ("w3", w3)):
        if name != "w1":
            _set_weights(rig, f, w)
        r, got = _compute(rig, f, _FETCHED + ("ray_weights",))
        assert r == 2
        r0, ref = _compute(rig, rig.field(b.replace(spotWeights=w)), _FETCHED + ("ray_weights",))
        assert r0 == 0
        _same(got, ref, _FETCHED + ("ray_weights",))
        seen[name] = got
    _same(first, seen["w1"])
    assert not np.array_equal(seen["w1"]["dose"], seen["w2"]["dose"]) and not np.array_equal(seen["w2"]["dose"], seen["w3"]["dose"])
    if cutoff == 1.0:
        # a whole 32 x 8 tile without a live ray while the record was made, with live rays when it is replayed
        W, H, L = first["info"]["ray_dims"]
        live = {k: (v["ray_weights"].reshape(L, H // 8, 8, W // 32, 32) >= cutoff).any(axis=(2, 4)) for k, v in seen.items()}
        assert (~live["w1"] & live["w2"]).any() and (~live["w2"] & live["w3"]).any()
        assert not np.array_equal(seen["w1"]["first_passive"], seen["w2"]["first_passive"])


def test_negative_sigma_sq(rig_of, synth, orc):
    """With the walk going on far behind the peak (bp_depth_cutoff 1.3) sigma^2 falls below zero on live rays: their 1/sigma is
    stored as NaN (the reciprocal of the root of a negative number), not as the +inf of a dead ray. Bit for bit, NaNs included."""
    scn = hetero_scene(synth, 128, [0.0], spots=7, pitch=6.0)
    b = scn.beams[0]
    opt = options(1.0)
    opt.bp_depth_cutoff = 1.3
    of = orc.run_field(scn, b, np.zeros_like(scn.ct), options=opt, keep_layers=True)
    assert of.status == 0, of.error
    W, H, L = of.info["ray_dims"]
    plan = of.get("layer_plan").reshape(L, 8)
    rs = of.get("rsigma").reshape(L, b.tracerSteps, H, W)
    first = of.info["beam_first_inside"]
    n_negative = sum(int(np.isnan(rs[l, first:int(plan[l, 5])]).sum()) for l in range(L))
    assert n_negative > 0                                             # the oracle: live (ray, step) with sigma^2 < 0 exist
    rig = rig_of(scn, opt)
    _, outs = _runs(rig, b, 3, (0, 1, 2))
    _, walked = _runs(rig, b, 1, (0,), RTD_NO_SIGMA_REUSE="1")
    g = walked[0]["rsigma"].reshape(L, b.tracerSteps, H, W)
    assert sum(int(np.isnan(g[l, first:int(plan[l, 5])]).sum()) for l in range(L)) == n_negative
    for out in outs:
        np.testing.assert_array_equal(_written(out, "rsigma").view(np.uint32), _written(walked[0], "rsigma").view(np.uint32))
        _same(out, walked[0])


@pytest.mark.parametrize("case", ["set_luts", "set_options", "set_ct"])
def test_epoch(rig_of, synth, case):
    """A change of LUTs, options or CT drops the record with the trace: the next compute walks, the one after it records, and both
    equal a field that computes for the first time under the new inputs. A field keeps the options it was created under, so for the
    field that exists already rtd_set_options (another cut-off) is an epoch change only, and the field it is compared with was created
    before the call; the new cut-off itself is in effect for a field created after the call, which is checked against its walking
    twin as well."""
    scn = hetero_scene(synth, 128, [10.0], spots=7, pitch=6.0)
    b = scn.beams[0]
    rig = rig_of(scn, options(1.0))
    f, before = _runs(rig, b, 3, (0, 1, 2))
    fresh = rig.field(b)                                              # (a field keeps the options it was created under)
    if case == "set_luts":
        rig.eng.set_luts(scn.luts)
    elif case == "set_options":
        rig.eng.set_options(options(0.5))
    else:
        ct2 = scn.ct.copy()
        ct2[:, :, : scn.ct.shape[2] // 2] *= 0.9                       # a lighter half: other WEPL, other sigma chain
        rig.eng.set_ct(ct2)
    r0, ref = _compute(rig, fresh)
    assert r0 == 0
    after = [_compute(rig, f) for _ in range(3)]
    assert [r for r, _ in after] == [0, 1, 2]
    for _, out in after:
        _same(out, ref)
    assert (case == "set_ct") == (not np.array_equal(before[2]["dose"], ref["dose"]))
    if case == "set_options":
        _, later = _runs(rig, b, 3, (0, 1, 2))                        # created under the cut-off of 0.5
        _, walked = _runs(rig, b, 1, (0,), RTD_NO_SIGMA_REUSE="1")
        for out in later:
            _same(out, walked[0])
        assert not np.array_equal(later[0]["first_passive"], ref["first_passive"])   # rays between the two cut-offs are alive now


@pytest.mark.parametrize("switch", ["RTD_NO_FILL_COMPACT", "RTD_SEPARATE_KS_PLAN"])
def test_under_switches(rig_of, synth, switch):
    """The identity lane placement, and the superposition's plan as its own launch: the replay is equal under both."""
    scn = hetero_scene(synth, 128, [20.0], spots=7, pitch=6.0)
    rig = rig_of(scn, options(1.0))
    _, outs = _runs(rig, scn.beams[0], 3, (0, 1, 2), **{switch: "1"})
    _against_walking(rig, scn.beams[0], outs, **{switch: "1"})
    _, plain = _runs(rig, scn.beams[0], 1, (0,))
    _same(outs[2], plain[0])


@pytest.mark.parametrize("case", ["nuclear_corr", "rows_above_64", "RTD_SEPARATE_PLAN"])
def test_fallback_configurations(rig_of, synth, case):
    """What never reuses its trace never records: sigma_reused stays 0 and the results stand."""
    env = {}
    if case == "nuclear_corr":
        scn = scenarios.water_cube(luts.synth_luts(nuclear=True), n=64, n_layers=3, spots=7, pitch=6.0)
        rig = rig_of(scn, options(1.0, nuclear=abi.RTD_NUC_SOUKUP))
    elif case == "rows_above_64":
        scn = hetero_scene(synth, 128, [0.0], spots=(5, 70), pitch=(8.0, 1.5), layers=2)
        rig = rig_of(scn, options(1.0))
    else:
        scn = hetero_scene(synth, 128, [0.0], spots=7, pitch=6.0)
        rig = rig_of(scn, options(1.0))
        env = {"RTD_SEPARATE_PLAN": "1"}
    f, outs = _runs(rig, scn.beams[0], 3, (0, 0, 0), **env)
    assert int(f.fetch("trace_reused")[0]) == 0
    for out in outs[1:]:
        _same(out, outs[0])


def test_dose_influence(rig_of, synth):
    """The batches of a dose-influence matrix replay (the first one records): the CSC is identical to the walking field's."""
    scn = hetero_scene(synth, 96, [30.0], spots=5, pitch=8.0, layers=2)
    b = scn.beams[0]
    rig = rig_of(scn, options(0.0))
    mats = []
    for env, expect in (({}, 2), ({"RTD_NO_SIGMA_REUSE": "1"}, 0)):
        f = rig.field(b, **env)
        _, before = _compute(rig, f)
        d = f.dose_influence(0.0)
        assert d.nnz > 0
        assert int(f.fetch("sigma_reused")[0]) == expect              # (the restoring forward at the field's own weights)
        for nm in _FETCHED:
            np.testing.assert_array_equal(_written(dict(before, **{nm: f.fetch(nm)}), nm), _written(before, nm), err_msg=nm)
        mats.append(d)
    for a, c in [(mats[0].indptr, mats[1].indptr), (mats[0].indices, mats[1].indices), (bits(mats[0].data), bits(mats[1].data))]:
        np.testing.assert_array_equal(a, c)


def test_release(rig_of, synth):
    """A released field's record goes with it: the field of the same shape that takes its workspace over, with other energies,
    walks first, records its own and equals a field that never reuses."""
    scn = hetero_scene(synth, 128, [0.0], spots=7, pitch=6.0)
    b = scn.beams[0]
    rig = rig_of(scn, options(1.0))
    f, _ = _runs(rig, b, 3, (0, 1, 2))
    rig.fields.remove(f)
    f.release()
    b2 = b.replace(beamEnergies=(b.beamEnergies * np.float32(0.93)).astype(np.float32))
    _, outs = _runs(rig, b2, 3, (0, 1, 2))
    _, traced = _runs(rig, b2, 2, (0, 0), RTD_NO_TRACE_REUSE="1")
    for out in outs + traced[1:]:
        _same(out, traced[0])
    _, other = _runs(rig, b, 1, (0,), RTD_NO_TRACE_REUSE="1")
    assert not np.array_equal(other[0]["dose"], traced[0]["dose"])
