"""GPU tests of the trace and plan a field keeps between computes ("What a field keeps between computes").

A compute under the CT, LUTs and options of a finished compute of the same field launches neither the tracer nor the scan nor the
plan. The change reorders no arithmetic: every comparison here is bitwise (assert_array_equal), against the earlier computes of the
same field and against a field created under RTD_NO_TRACE_REUSE (every compute traces and plans again)."""
import math

import numpy as np
import pytest

from gpu_support import FieldRig, hetero_scene, options, rig_fixture
from raytracedicom_amd import abi, luts, scenarios

pytestmark = pytest.mark.gpu

_FETCHED = ("bev", "tile_radius", "eff_radius", "layer_plan", "first_passive", "first_inside", "first_outside", "wepl_min", "density", "wepl")


def _missing(synth, n=128):
    """A beam 1 m beside the volume: every sample is BORDER zero, the field is empty."""
    ct, voxel = scenarios.hetero_phantom(n)
    beam = scenarios.make_field(synth, n, voxel, (872.0, -128.0, -106.0), 0.0, 7, 6.0, 3, 5)
    return scenarios.Scenario("beam beside the volume", synth, ct, (voxel,) * 3, [beam])


rig_of = rig_fixture(FieldRig)


def _compute(rig, f, names=_FETCHED):
    """One compute with a finish: (trace_reused, {dose, info, timing, the fetched arrays})."""
    dose, info, timing = rig.compute(f)
    out = {"info": info, "timing": timing, "dose": dose}
    for nm in names:
        out[nm] = f.fetch(nm).copy()
    return int(f.fetch("trace_reused")[0]), out


def _same(a, b, names=_FETCHED):
    assert a["info"] == b["info"]
    for nm in ("dose",) + tuple(names):
        np.testing.assert_array_equal(a[nm], b[nm], err_msg=nm)


def _three_computes(rig, beam, expect=(0, 1, 1), **env):
    """Three computes of one field with a finish in between, compared with each other and with a field that never reuses."""
    f = rig.field(beam, **env)
    runs = [_compute(rig, f) for _ in range(3)]
    assert tuple(r for r, _ in runs) == tuple(expect)
    env = dict(env, RTD_NO_TRACE_REUSE="1")
    g = rig.field(beam, **env)
    refs = [_compute(rig, g) for _ in range(2)]
    assert [r for r, _ in refs] == [0, 0]
    for _, out in runs + refs[1:]:
        _same(out, refs[0][1])
    return runs[0][1]


@pytest.mark.parametrize("case", ["across", "diagonal", "along", "water", "missing"])
def test_reused_equals_traced(rig_of, synth, case):
    """The three sampling kernels (0 degrees; 37 degrees with a finite source distance; 90 degrees), the known-uniform path (water)
    and an empty field (the beam misses the volume)."""
    if case == "water":
        scn = scenarios.water_cube(synth, n=128, n_layers=3, spots=9, pitch=5.0)
    elif case == "missing":
        scn = _missing(synth)
    else:
        deg, dist = {"across": (0.0, (math.inf, math.inf)), "diagonal": (37.0, (2000.0, 2500.0)), "along": (90.0, (math.inf, math.inf))}[case]
        scn = hetero_scene(synth, 128, [deg], source_dist=dist, spots=7, pitch=6.0)
    rig = rig_of(scn, options(1.0))
    out = _three_computes(rig, scn.beams[0])
    if case == "water":
        assert out["info"]["uniform_sigma"] == 1 and out["dose"].max() > 0
    elif case == "missing":
        assert out["dose"].max() == 0 and out["info"]["live_steps"] == 0
    else:
        assert out["info"]["uniform_sigma"] == 0 and out["dose"].max() > 0


def test_separate_ks_plan_reuses(rig_of, synth):
    """RTD_SEPARATE_KS_PLAN moves the superposition's plan only: the trace is reused under it."""
    scn = hetero_scene(synth, 128, [20.0], spots=7, pitch=6.0)
    _three_computes(rig_of(scn, options(1.0)), scn.beams[0], RTD_SEPARATE_KS_PLAN="1")


@pytest.mark.parametrize("case", ["nuclear_corr", "rows_above_64", "RTD_SEPARATE_PLAN"])
def test_fallback_configurations(rig_of, synth, case):
    """What falls back to the full sequence, deliberately: every compute traces (trace_reused = 0) and the results stand."""
    if case == "nuclear_corr":
        nl = luts.synth_luts(nuclear=True)
        scn = scenarios.water_cube(nl, n=64, n_layers=3, spots=7, pitch=6.0)
        rig = rig_of(scn, options(1.0, nuclear=abi.RTD_NUC_SOUKUP))
        _three_computes(rig, scn.beams[0], expect=(0, 0, 0))
    elif case == "rows_above_64":
        scn = hetero_scene(synth, 128, [0.0], spots=(5, 70), pitch=(8.0, 1.5), layers=2)
        _three_computes(rig_of(scn, options(1.0)), scn.beams[0], expect=(0, 0, 0))
    else:
        scn = hetero_scene(synth, 128, [0.0], spots=7, pitch=6.0)
        _three_computes(rig_of(scn, options(1.0)), scn.beams[0], expect=(0, 0, 0), RTD_SEPARATE_PLAN="1")


@pytest.mark.parametrize("cutoff", [0.0, 1.0])
def test_reweighting(rig_of, synth, cutoff):
    """After rtd_field_set_spot_weights the next compute reuses the trace and equals a fresh field with those weights."""
    scn = hetero_scene(synth, 128, [15.0], spots=7, pitch=6.0)
    b = scn.beams[0]
    rig = rig_of(scn, options(cutoff))
    f = rig.field(b)
    assert _compute(rig, f)[0] == 0
    w = (b.spotWeights * np.random.default_rng(9).random(b.spotWeights.shape)).astype(np.float32)
    w[:, :2, :] = 0.5                                                 # below a cut-off of 1: those rays die
    dW = rig.eng.device_alloc(w.nbytes)
    try:
        rig.eng.to_device(dW, w)
        f.set_spot_weights(dW)
    finally:
        rig.eng.sync()
        rig.eng.device_free(dW)
    names = tuple(n for n in _FETCHED if n != "bev")                  # (slices outside [entry, passive) of a BEV buffer hold what earlier computes left)
    reused, got = _compute(rig, f, names)
    assert reused == 1
    r2, ref = _compute(rig, rig.field(b.replace(spotWeights=w)), names)
    assert r2 == 0
    _same(got, ref, names)
    assert not np.array_equal(got["dose"], _compute(rig, rig.field(b), names)[1]["dose"])


@pytest.mark.parametrize("case", ["other_device_ct", "same_pointer", "set_luts", "set_options"])
def test_invalidation(rig_of, synth, case):
    """Every rtd_set_ct*, LUT or options call drops the trace: the next compute traces again and equals a fresh field under the new
    inputs; the compute after it reuses again."""
    scn = hetero_scene(synth, 128, [10.0], spots=7, pitch=6.0)
    b = scn.beams[0]
    rig = rig_of(scn, options(1.0), set_ct=False)
    n = scn.ct.size * 4
    ct2 = scn.ct.copy()
    ct2[:, :, : scn.ct.shape[2] // 2] *= 0.9                           # a lighter half: other WEPL, other entry sigma chain
    dA, dB = rig.eng.device_alloc(n), rig.eng.device_alloc(n)
    try:
        rig.eng.to_device(dA, scn.ct)
        rig.eng.to_device(dB, ct2)
        rig.eng.set_ct_device(dA, scn.dims)
        f = rig.field(b)
        assert _compute(rig, f)[0] == 0
        r1, before = _compute(rig, f)
        assert r1 == 1
        changed = True
        if case == "other_device_ct":
            rig.eng.set_ct_device(dB, scn.dims)
        elif case == "same_pointer":
            rig.eng.sync()
            rig.eng.to_device(dA, ct2)                                # rewritten in place, then announced
            rig.eng.set_ct_device(dA, scn.dims)
        elif case == "set_luts":
            rig.eng.set_luts(scn.luts)
            changed = False
        else:
            rig.eng.set_options(options(1.0))                              # (a field keeps the options it was created under: the same values)
            changed = False
        names = tuple(nm for nm in _FETCHED if nm != "bev")
        r2, after = _compute(rig, f, names)
        assert r2 == 0
        fresh = rig.field(b)
        r3, ref = _compute(rig, fresh, names)
        assert r3 == 0
        _same(after, ref, names)
        assert changed == (not np.array_equal(after["wepl"], before["wepl"]))
        assert changed == (not np.array_equal(after["dose"], before["dose"]))
        r4, again = _compute(rig, f, names)
        assert r4 == 1
        _same(again, ref, names)
        r5, again = _compute(rig, f, names)
        assert r5 == 1
        _same(again, ref, names)
    finally:
        rig.eng.sync()
        for fld in list(rig.fields):
            fld.destroy()
        rig.fields.clear()
        rig.eng.device_free(dA)
        rig.eng.device_free(dB)


def test_dose_influence(rig_of, synth):
    """The matrix is the same with and without reuse (its batches are re-weighted computes of one field), and the field's state
    afterwards is that of a compute at its own weights."""
    scn = hetero_scene(synth, 96, [30.0], spots=5, pitch=8.0, layers=2)
    b = scn.beams[0]
    rig = rig_of(scn, options(0.0))
    mats, states = [], []
    for env in ({}, {"RTD_NO_TRACE_REUSE": "1"}):
        f = rig.field(b, **env)
        _, before = _compute(rig, f)
        d = f.dose_influence(0.0)
        assert d.nnz > 0
        assert int(f.fetch("trace_reused")[0]) == (0 if env else 1)   # (the restoring forward at the field's own weights)
        np.testing.assert_array_equal(f.fetch("bev"), before["bev"])
        rig.eng.device_zero(rig.dDose, rig.nb)
        f.transfer(rig.dDose)
        rig.eng.sync()
        dose = np.empty(rig.shape, dtype=np.float32)
        rig.eng.to_host(dose, rig.dDose)
        np.testing.assert_array_equal(dose, before["dose"])
        for nm in _FETCHED:
            np.testing.assert_array_equal(f.fetch(nm), before[nm], err_msg=nm)
        mats.append(d)
        states.append(before)
    for a, c in [(mats[0].indptr, mats[1].indptr), (mats[0].indices, mats[1].indices), (mats[0].data, mats[1].data)]:
        np.testing.assert_array_equal(a, c)
    _same(states[0], states[1])


def test_two_computes_in_flight(rig_of, synth):
    """Two launches with no finish between them: the second one traces again (nothing has been seen finished), the finish behind it
    makes its trace usable, the compute after that reuses it and records the sigma walk, the one after that replays the record."""
    scn = hetero_scene(synth, 96, [30.0], spots=5, pitch=8.0, layers=2)
    b = scn.beams[0]
    rig = rig_of(scn, options(1.0))
    f = rig.field(b)

    def flags():
        return int(f.fetch("trace_reused")[0]), int(f.fetch("sigma_reused")[0])
    f.compute_bev()
    f.compute_bev()
    assert flags() == (0, 0)
    f.finish()
    _, third = _compute(rig, f)
    assert flags() == (1, 1)
    _, fourth = _compute(rig, f)
    assert flags() == (1, 2)
    r, ref = _compute(rig, rig.field(b, RTD_NO_TRACE_REUSE="1"))
    assert r == 0 and ref["dose"].max() > 0
    _same(third, ref)
    _same(fourth, ref)


def test_gradient(rig_of, synth):
    """rtd_field_spot_gradient behind a reused forward equals the one behind a traced forward."""
    scn = hetero_scene(synth, 96, [30.0], spots=5, pitch=8.0, layers=2)
    b = scn.beams[0]
    rig = rig_of(scn, options(0.0))
    g = (np.random.default_rng(2).random(rig.shape) - 0.5).astype(np.float32)
    dG = rig.eng.device_alloc(rig.nb)
    dOut = rig.eng.device_alloc(b.spotWeights.nbytes)
    grads = []
    try:
        rig.eng.to_device(dG, g)
        for env, expect in (({}, 1), ({"RTD_NO_TRACE_REUSE": "1"}, 0)):
            f = rig.field(b, **env)
            _compute(rig, f)
            assert _compute(rig, f)[0] == expect
            f.spot_gradient(dG, dOut)
            out = np.empty(b.spotWeights.shape, dtype=np.float32)
            rig.eng.to_host(out, dOut)
            grads.append(out)
    finally:
        rig.eng.sync()
        rig.eng.device_free(dG)
        rig.eng.device_free(dOut)
    assert np.abs(grads[0]).max() > 0
    np.testing.assert_array_equal(grads[0], grads[1])


def test_timing_of_a_reused_compute(rig_of, synth):
    """No tracer stage; the six buckets still sum to total_ms (the 5 % rule of test_gpu_parity.py); all keys stay."""
    scn = scenarios.water_cube(synth, n=128, n_layers=4, spots=17, pitch=4.0)
    rig = rig_of(scn, options(1.0, timing=1))
    f = rig.field(scn.beams[0])
    r0, first = _compute(rig, f, ())
    r1, second = _compute(rig, f, ())
    assert (r0, r1) == (0, 1)
    assert first["timing"]["raytracing_ms"] > 0
    t = second["timing"]
    assert set(t) == set(first["timing"])
    assert t["raytracing_ms"] == 0
    buckets = ("raytracing_ms", "prepare_energy_loop_ms", "fill_idd_sigma_ms", "prepare_superp_ms", "superp_ms", "transforming_ms")
    print("timing of the reused compute:", {k: t[k] for k in buckets + ("total_ms",)})
    assert t["total_ms"] > 0 and t["prepare_energy_loop_ms"] > 0
    assert sum(t[k] for k in buckets) == pytest.approx(t["total_ms"], rel=0.05)


def test_two_streams(rig_of, synth):
    """Computed on stream A, finished, then on stream B: the second compute reuses what the first one left, with identical results."""
    import torch
    scn = hetero_scene(synth, 128, [37.0], source_dist=(2000.0, 2500.0), spots=7, pitch=6.0)
    rig = rig_of(scn, options(1.0))
    dev = torch.device("cuda", 0)
    sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    f = rig.field(scn.beams[0])
    try:
        rig.eng.set_stream(sa.cuda_stream)
        ra, a = _compute(rig, f)
        rig.eng.set_stream(sb.cuda_stream)
        rb, b = _compute(rig, f)
    finally:
        rig.eng.sync()
        rig.eng.set_stream(0)                                         # (the handle's own stream)
    assert (ra, rb) == (0, 1)
    assert a["dose"].max() > 0
    _same(a, b)
