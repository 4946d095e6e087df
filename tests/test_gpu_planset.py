"""GPU tests of the plan set (include/rtd.h: rtd_field_dose_influence_apply_set / _apply_t_set and rtd_planset_*)
through the C ABI. The contract is bits: every slot of the products is the restated tree (tests/tree_reference.py) of that plan's
vector alone, and every plan of a set is the plain optimiser on a plain objective with that plan's terms. Only bits and integers are
compared; no tolerance anywhere. Every case prints and asserts its own shape condition, so that it cannot pass hollow."""
import ctypes as C
import math

import numpy as np
import pytest

import optimizer_reference as R
import planset_reference as PR
from gpu_support import FieldRig, bits, hetero_scene, options, rig_fixture
from planset_rig import PlanSetRig, SetProducts
from raytracedicom_amd import abi, scenarios

pytestmark = pytest.mark.gpu

rig_of = rig_fixture(PlanSetRig)


# ---- 1., 2. The products with P right-hand sides ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def long_rows(engine, synth):
    """13 x 13 spots 2 mm apart in one layer (tests/test_gpu_plan_sizes.py::test_products_long_rows): rows of more than 128 entries."""
    scn = hetero_scene(synth, 64, (0.0,), spots=13, pitch=2.0, layers=1)
    rig = FieldRig(engine, scn, options(0.0))
    try:
        f = rig.field(scn.beams[0])
        d = f.dose_influence()
        _, info = f.finish()
        yield SetProducts(rig, f, d, info, 51)
    finally:
        rig.close()


# (3, 5) and (5, 7): strides that are no power of two take the scalar loads (rtd_planset.hpp, VEC = false), at 4 and 8 accumulators
@pytest.mark.parametrize("n_plans,stride", [(1, 1), (3, 4), (8, 8), (16, 16), (3, 5), (5, 7)])
def test_products_long_rows(long_rows, n_plans, stride):
    counts = np.bincount(long_rows.d.indices, minlength=long_rows.nvox)
    print("longest row %d entries; %d rows whose length is no multiple of 16; %d plans at stride %d"
          % (int(counts.max()), int(((counts % 16) != 0).sum()), n_plans, stride))
    assert counts.max() > 128, "no row of more than 128 entries: longest %d" % int(counts.max())
    assert ((counts > 16) & (counts % 16 != 0)).any(), "no row longer than 16 whose length is no multiple of 16"
    long_rows.check(n_plans, stride)


def _tripled(beam):
    """The beam on a dose grid of three voxels per CT voxel (dose voxels 3 i .. 3 i + 2 cover CT voxel i)."""
    t = beam.gantryToDoseIdx
    return beam.replace(gantryToDoseIdx=scenarios.Float3AffineTransform(3.0 * t.m, 3.0 * t.v + 1.0))


def test_products_long_columns(engine, synth):
    """The 192^3 case of tests/test_gpu_plan_sizes.py::test_products_large_box_and_long_columns, the same scene and transform: a column
    of more than 64 chunks (the second trip of the reduce) and partial last chunks; three plans at stride 4. Every one of that scene's
    nine spots meets the phantom, so the empty column comes from a second field on the same grid, under the same transform: 7 x 3 spots
    50 mm apart, whose outermost columns lie 22 mm outside the CT (tests/test_gpu_dose_influence_apply.py)."""
    scn = hetero_scene(synth, 64, (20.0,), spots=3, pitch=45.0, layers=1)
    wide = hetero_scene(synth, 64, (0.0,), spots=(7, 3), pitch=50.0, layers=1)
    rig = FieldRig(engine, scn, options(0.0), (192, 192, 192))
    try:
        f = rig.field(_tripled(scn.beams[0]))
        d = f.dose_influence()
        _, info = f.finish()
        lens = np.diff(d.indptr)
        chunks = -(-lens // 2048)
        print("%d entries, longest column %d, chunks per column %s, last chunk lengths %s" % (d.nnz, int(lens.max()), chunks.tolist(), (lens % 2048).tolist()))
        assert chunks.max() > 64, "no column of more than 64 chunks: %s" % chunks.tolist()
        assert ((lens > 0) & (lens % 2048 != 0)).any(), "no column with a partial last chunk: %s" % (lens % 2048).tolist()
        SetProducts(rig, f, d, info, 61).check(3, 4)
        fw = rig.field(_tripled(wide.beams[0]))
        dw = fw.dose_influence()
        _, infow = fw.finish()
        lens = np.diff(dw.indptr)
        print("the wide field: %d entries, column lengths %s" % (dw.nnz, lens.tolist()))
        assert (lens == 0).any() and lens.max() > 2048, "no empty column beside columns of several chunks: %s" % lens.tolist()
        SetProducts(rig, fw, dw, infow, 62).check(3, 4)
    finally:
        rig.close()


# ---- 3. - 7. The plan set against P plain optimisers ------------------------------------------------------------------------

def test_one_field_equals_three_plain_optimisers_and_blend(rig_of, synth):
    """P = 3 on one field: overdose weight x (1, 10, 0.1), target levels x (1, 0.9, 1.1), plan 2 from a constant 50; run(2); run(3) on
    the set against run(5) on three plain optimisers. Then the blend of the three best plans against its restatement."""
    rig = rig_of(hetero_scene(synth, 96, (30.0,)))
    variants = rig.variants((1.0, 10.0, 0.1), (1.0, 0.9, 1.1))
    s = rig.planset(variants)
    rig.set_plan_weights(s, 2, 50.0)
    plains = [rig.plain(v, start=50.0 if p == 2 else None) for p, v in enumerate(variants)]
    r0, h0 = s.result(0)
    assert r0["iterations"] == 0 and r0["best_iteration"] == -1 and r0["f_best"] == math.inf and h0.size == 0, "a fresh set: %r" % (r0,)
    s.run(2)
    s.run(3)
    hists = []
    for p, (opt, obj) in enumerate(plains):
        opt.run(5)
        rep, hist = rig.same_as_plain(s, p, opt, obj)
        print("plan %d: f %s, step %.6g, best iteration %d" % (p, " ".join("%.6g" % v for v in hist), rep["step"], rep["best_iteration"]))
        assert rep["iterations"] == 5 and hist.size == 5 and rep["guarded"] == 0 and np.all(np.isfinite(hist)), "plan %d: %r %r" % (p, rep, hist)
        hists.append(hist)
    for a in range(3):
        for b in range(a + 1, 3):
            assert not np.array_equal(hists[a], hists[b]), "plans %d and %d have one history: the variants changed nothing" % (a, b)
    # 7. the blend
    best = [s.weights(p, 0, best=True) for p in range(3)]
    got = s.blend((0.2, 0.5, 0.3), 0)
    want = PR.blend(best, (0.2, 0.5, 0.3))
    n = int((bits(got) != bits(want)).sum())
    assert n == 0 and got.max() > 0, "blend(0.2, 0.5, 0.3) differs from its restatement at %d of %d spots" % (n, got.size)
    assert not np.array_equal(got, best[0]) and not np.array_equal(got, best[1]), "the blend is one of its plans"
    one = s.blend((1, 0, 0), 0)
    assert np.array_equal(bits(one), bits(best[0])), "blend(1, 0, 0) is not plan 0's w_best: %d differ" % int((bits(one) != bits(best[0])).sum())
    cur = s.blend((0, 0, 1), 0, best=False)
    assert np.array_equal(bits(cur), bits(s.weights(2, 0))), "blend(0, 0, 1, best=False) is not plan 2's w"


def test_two_fields_eight_plans(rig_of, synth):
    """Two overlapping fields, P = 8, three iterations: every plan against its plain optimiser, and plan 0's and plan 7's volume
    after every iteration against a zeroed volume + apply(init = 0) per field at the weights that entered it (what field 1 added
    outside field 0's box an iteration earlier must be gone)."""
    rig = rig_of(hetero_scene(synth, 96, (0.0, 90.0)))
    n0 = np.bincount(rig.mats[0].indices, minlength=rig.nvox) > 0
    n1 = np.bincount(rig.mats[1].indices, minlength=rig.nvox) > 0
    print("voxels of field 0 only %d, of field 1 only %d, of both %d" % (int((n0 & ~n1).sum()), int((n1 & ~n0).sum()), int((n0 & n1).sum())))
    assert (n0 & n1).any() and (n1 & ~n0).any() and (n0 & ~n1).any(), "the fields must overlap and each reach where the other does not"
    wf = (1.0, 10.0, 0.1, 3.0, 0.3, 30.0, 1.0, 2.0)
    lf = (1.0, 0.9, 1.1, 1.0, 1.05, 0.95, 0.8, 1.2)
    variants = rig.variants(wf, lf)
    s = rig.planset(variants)
    dDose = rig.alloc(4 * rig.nvox)
    seen = {0: [], 7: []}
    for k in range(3):
        ws = {p: [s.weights(p, i) for i in range(2)] for p in seen}
        s.run(1)
        for p in seen:
            got = s.dose(p).reshape(-1)
            rig.dose_of(ws[p], dDose)
            want = rig.volume(dDose)
            n = int((bits(got) != bits(want)).sum())
            assert want.max() > 0 and n == 0, "iteration %d, plan %d: the volume is not the sum of the fields at %d voxels" % (k, p, n)
            seen[p].append(got)
    for p, vols in seen.items():
        assert not np.array_equal(vols[0], vols[1]) and not np.array_equal(vols[1], vols[2]), "plan %d's dose did not move" % p
    hists = []
    for p, v in enumerate(variants):
        opt, obj = rig.plain(v)
        opt.run(3)
        rep, hist = rig.same_as_plain(s, p, opt, obj)
        assert rep["iterations"] == 3 and hist.size == 3, "plan %d: %r" % (p, rep)
        hists.append(tuple(hist))
    assert len(set(hists)) == 8, "eight variants, %d different histories" % len(set(hists))


def test_guard_stays_in_its_plan(engine, rig_of, synth):
    """P = 3; plan 1 starts at weights of +inf: its dose is +inf wherever it has entries and its objective +inf in float64. (No finite
    float32 weights do that: a finite float32 dose squared is below 2^256, and a float64 sum of a few hundred thousand such terms
    stays far below 2^1024; only a dose that has itself overflowed float32 makes the objective infinite.) It takes
    the guard, alone; given finite weights it recovers, thrown out again it returns to its own w_best; plans 0 and 2 keep the bits of
    their plain optimisers throughout, and so does plan 1 of a plain optimiser treated the same way."""
    L = engine.lib()
    rig = rig_of(hetero_scene(synth, 64, (0.0,), spots=3, layers=1))
    variants = rig.variants((1.0, 10.0, 0.1), (1.0, 0.9, 1.1))
    s = rig.planset(variants)
    rig.set_plan_weights(s, 1, math.inf)
    plains = [rig.plain(v, start=math.inf if p == 1 else None) for p, v in enumerate(variants)]

    def both(fn):
        fn()
        for opt, _ in plains:
            opt.run(2)
        s.run(2)

    both(lambda: None)
    rep, hist = abi.RtdOptimizerReport(), np.zeros(2)
    st = L.rtd_planset_result(rig.eng._h, s._h, 1, C.byref(rep), hist.ctypes.data_as(C.POINTER(C.c_double)), 2)
    rp = abi.RtdOptimizerReport()
    stp = L.rtd_optimizer_result(rig.eng._h, plains[1][0]._h, C.byref(rp), None, 0)
    print("plan 1 from +inf: f %r, guarded %d, status %d (plain %d)" % (hist.tolist(), rep.guarded, st, stp))
    assert np.all(hist == math.inf), "plan 1's objective did not overflow to +inf: %r" % hist.tolist()
    assert rep.guarded == 2 and rep.f_best == math.inf and rep.iterations == 2, "plan 1 did not take the guard twice: %r" % rep.as_dict()
    assert st == stp == abi.RTD_ERR_INVALID_ARG and rep.as_dict() == rp.as_dict(), "an unusable start is reported as the plain optimiser reports it"
    for p in (0, 2):
        r, h = rig.same_as_plain(s, p, *plains[p], what="after plan 1's guards, ")
        assert r["guarded"] == 0 and np.all(np.isfinite(h)), "plan %d noticed plan 1's guard: %r %r" % (p, r, h)

    def finite():
        rig.set_plan_weights(s, 1, 50.0)
        rig.set_weights(plains[1][0], 50.0)

    def thrown():
        rig.set_plan_weights(s, 1, math.inf)
        rig.set_weights(plains[1][0], math.inf)

    both(finite)
    both(thrown)
    for p in range(3):
        r, h = rig.same_as_plain(s, p, *plains[p], what="at the end, ", bad_start=p == 1)
        assert r["iterations"] == 6, "plan %d: %r" % (p, r)
        if p == 1:
            print("plan 1: f %r, guarded %d" % (h.tolist(), r["guarded"]))
            assert r["guarded"] == 3 and np.all(np.isfinite(h[2:4])) and h[4] == math.inf and h[5] == r["f_best"], "plan 1: %r %r" % (r, h)
            assert np.all(np.isfinite(s.weights(1, 0))), "plan 1 did not come back to finite weights"
        else:
            assert r["guarded"] == 0 and np.all(np.isfinite(h)), "plan %d: %r %r" % (p, r, h)


def test_resident_means_resident(rig_of, synth):
    """run(6) = run(2) three times, bit for bit; run(5) captured into a graph on a caller's stream (which an allocation, a copy or a
    synchronisation inside run would fail) and replayed once gives the bits of the direct call. Under the machine's own queue setting."""
    import torch
    rig = rig_of(hetero_scene(synth, 96, (0.0,)))
    variants = rig.variants((1.0, 10.0, 0.1), (1.0, 0.9, 1.1))

    def fresh():
        s = rig.planset(variants)
        for p in range(3):
            rig.set_plan_weights(s, p, 0.0)
        return s

    a, b = fresh(), fresh()
    a.run(6)
    for _ in range(3):
        b.run(2)
        b.run(0)
    for p in range(3):
        ra, ha = a.result(p)
        rb, hb = b.result(p)
        assert ra == rb and ha.size == 6 and np.array_equal(bits(ha), bits(hb)), "plan %d: run(6) and 3 x run(2) differ: %r %r" % (p, ra, rb)
        for best in (False, True):
            assert np.array_equal(bits(a.weights(p, 0, best=best)), bits(b.weights(p, 0, best=best))), "plan %d: weights differ (best=%s)" % (p, best)
    # graph capture: one run(5) = 5 iterations of launches and nothing else (an allocation, a copy or a synchronisation fails the capture)
    direct, captured = fresh(), fresh()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    rig.eng.sync()
    rig.eng.set_stream(st.cuda_stream)
    with torch.cuda.stream(st):
        direct.run(5)
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            captured.run(5)
        g.replay()
    torch.cuda.synchronize()
    res = [(direct.result(p), captured.result(p)) for p in range(3)]
    rig.eng.set_stream(None)
    for p, ((rd, hd), (rg, hg)) in enumerate(res):
        assert rd == rg and hd.size == 5 and np.array_equal(bits(hd), bits(hg)), "plan %d: the replayed graph differs from the direct run: %r %r" % (p, rd, rg)
        assert np.array_equal(bits(hd), bits(a.result(p)[1][:5])), "plan %d: the direct run on a caller's stream differs from the engine's stream" % p
        assert np.array_equal(bits(direct.weights(p, 0)), bits(captured.weights(p, 0))), "plan %d: the replayed graph's weights differ" % p
        assert np.array_equal(bits(direct.dose(p)), bits(captured.dose(p))), "plan %d: the replayed graph's dose differs" % p


def test_refusals_leave_everything_usable(engine, synth):
    L = engine.lib()
    scn = hetero_scene(synth, 64, (0.0,), spots=3, layers=1)
    rig = PlanSetRig(engine, scn)
    try:
        eng, h, f = rig.eng, rig.eng._h, rig.fields[0]
        nT = len(rig.terms)
        arr = lambda *fs: (C.c_void_p * 17)(*[x._h for x in fs])   # noqa: E731

        def table(variants):
            flat = [abi.RtdObjectiveTerm(int(k), int(r), float(w), float(l)) for v in variants for (k, r, w, l) in v]
            return (abi.RtdObjectiveTerm * len(flat))(*flat)

        good = rig.variants((1.0, 2.0), (1.0, 1.0))
        out = C.c_void_p()
        create = lambda fields, n_fields, obj, tab, n_plans: L.rtd_planset_create(h, fields, n_fields, obj, tab, n_plans, None, C.byref(out))   # noqa: E731
        big = table(good * 9)
        assert create(arr(f), 1, rig.obj._h, big, 0) == abi.RTD_ERR_INVALID_ARG, "n_plans = 0"
        assert create(arr(f), 1, rig.obj._h, big, 17) == abi.RTD_ERR_INVALID_ARG, "n_plans = 17"
        assert create(arr(f), 1, rig.obj._h, None, 2) == abi.RTD_ERR_INVALID_ARG, "null variants"
        assert create(arr(f), 0, rig.obj._h, table(good), 2) == abi.RTD_ERR_INVALID_ARG, "no fields"
        for what, change in (("another kind", lambda t: (R.SQ_DEVIATION if t[0] != R.SQ_DEVIATION else R.MEAN, t[1], t[2], t[3])),
                             ("another roi", lambda t: (t[0], 1 - t[1], t[2], t[3])), ("a weight of 0", lambda t: (t[0], t[1], 0.0, t[3])),
                             ("a weight of inf", lambda t: (t[0], t[1], math.inf, t[3])), ("a level of nan", lambda t: (t[0], t[1], t[2], math.nan))):
            bad = [list(v) for v in good]
            bad[1][2] = change(bad[1][2])
            assert create(arr(f), 1, rig.obj._h, table(bad), 2) == abi.RTD_ERR_INVALID_ARG, what
        # an objective with a DVH term, one with an EUD term
        for add in ("dvh", "eud"):
            o = eng.create_objective(rig.dims)
            o.add_roi(rig.ref.rois[0])
            o.add_term(R.SQ_DEVIATION, 0, 1.0, rig.level)
            if add == "dvh":
                o.add_dvh_term(abi.RTD_OBJ_MAX_DVH, 0, 1.0, rig.level, 0.5)
                tab = table([[(R.SQ_DEVIATION, 0, 1.0, rig.level), (abi.RTD_OBJ_MAX_DVH, 0, 1.0, rig.level)]])
            else:
                o.add_eud_term(abi.RTD_OBJ_SQ_MAX_EUD, 0, 1.0, rig.level, 4.0)
                tab = table([[(R.SQ_DEVIATION, 0, 1.0, rig.level), (abi.RTD_OBJ_SQ_MAX_EUD, 0, 1.0, rig.level)]])
            assert create(arr(f), 1, o._h, tab, 1) == abi.RTD_ERR_INVALID_ARG, "an objective with a %s term" % add
            o.destroy()
        fresh = eng.create_field(scn.beams[0], rig.dims)              # no matrix
        assert create(arr(fresh), 1, rig.obj._h, table(good), 2) == abi.RTD_ERR_NOT_READY, "a field without a matrix"
        assert create(arr(f, fresh), 2, rig.obj._h, table(good), 2) == abi.RTD_ERR_NOT_READY, "a second field without a matrix"
        remote = eng.create_field(scn.beams[0], rig.dims, remote=True)
        assert create(arr(remote), 1, rig.obj._h, table(good), 2) == abi.RTD_ERR_INVALID_ARG, "a remote field"
        assert not out.value, "a refused create wrote a handle"
        # the products: a bad n_plans or plan_stride, and what the plain calls refuse
        nvox, nspot = rig.nvox, rig.sizes[0]
        dVol, dSp = rig.alloc(4 * nvox * 16), rig.alloc(4 * nspot * 16)
        ap, apt = L.rtd_field_dose_influence_apply_set, L.rtd_field_dose_influence_apply_t_set
        for n_plans, stride, what in ((0, 4, "n_plans = 0"), (17, 17, "n_plans = 17"), (4, 3, "stride < n_plans"), (4, 17, "stride = 17")):
            assert ap(h, f._h, dSp, dVol, n_plans, stride, 1) == abi.RTD_ERR_INVALID_ARG, "apply_set: " + what
            assert apt(h, f._h, dVol, dSp, n_plans, stride) == abi.RTD_ERR_INVALID_ARG, "apply_t_set: " + what
        assert ap(h, f._h, None, dVol, 2, 2, 1) == abi.RTD_ERR_INVALID_ARG and ap(h, f._h, dSp, None, 2, 2, 0) == abi.RTD_ERR_INVALID_ARG, "apply_set: null pointer"
        assert apt(h, f._h, None, dSp, 2, 2) == abi.RTD_ERR_INVALID_ARG and apt(h, f._h, dVol, None, 2, 2) == abi.RTD_ERR_INVALID_ARG, "apply_t_set: null pointer"
        assert ap(h, fresh._h, dSp, dVol, 2, 2, 1) == abi.RTD_ERR_NOT_READY and apt(h, fresh._h, dVol, dSp, 2, 2) == abi.RTD_ERR_NOT_READY, "no matrix"
        assert ap(h, remote._h, dSp, dVol, 2, 2, 1) == abi.RTD_ERR_INVALID_ARG and apt(h, remote._h, dVol, dSp, 2, 2) == abi.RTD_ERR_INVALID_ARG, "a remote field"
        fresh.destroy()
        remote.destroy()
        # everything is still usable: a set of two plans, its index checks, and the bits of the plain optimisers
        s = rig.planset(good)
        rep, dW = abi.RtdOptimizerReport(), rig.alloc(4 * nspot)
        assert L.rtd_planset_run(h, None, 1) == abi.RTD_ERR_INVALID_ARG, "run: null set"
        assert L.rtd_planset_set_weights(h, s._h, 2, 0, dW) == abi.RTD_ERR_INVALID_ARG and L.rtd_planset_set_weights(h, s._h, 0, 1, dW) == abi.RTD_ERR_INVALID_ARG, "set_weights: index"
        assert L.rtd_planset_set_weights(h, s._h, 0, 0, None) == abi.RTD_ERR_INVALID_ARG, "set_weights: null pointer"
        assert L.rtd_planset_weights(h, s._h, 2, 0, 0, dW) == abi.RTD_ERR_INVALID_ARG and L.rtd_planset_weights(h, s._h, 0, 1, 0, dW) == abi.RTD_ERR_INVALID_ARG, "weights: index"
        assert L.rtd_planset_result(h, s._h, 2, C.byref(rep), None, 0) == abi.RTD_ERR_INVALID_ARG, "result: plan index"
        assert L.rtd_planset_result(h, s._h, 0, C.byref(rep), None, 3) == abi.RTD_ERR_INVALID_ARG, "result: capacity without a buffer"
        assert L.rtd_planset_dose(h, s._h, 2, dVol) == abi.RTD_ERR_INVALID_ARG and L.rtd_planset_dose(h, s._h, 0, None) == abi.RTD_ERR_INVALID_ARG, "dose: index, null"
        assert L.rtd_planset_values(h, s._h, None) == abi.RTD_ERR_INVALID_ARG, "values: null"
        co = (C.c_double * 2)(0.5, -0.5)
        assert L.rtd_planset_blend(h, s._h, co, 0, 1, dW) == abi.RTD_ERR_INVALID_ARG, "blend: a negative coefficient"
        co = (C.c_double * 2)(0.5, 0.5)
        assert L.rtd_planset_blend(h, s._h, co, 1, 1, dW) == abi.RTD_ERR_INVALID_ARG, "blend: field index"
        assert L.rtd_planset_blend(h, s._h, co, 0, 1, dW) == abi.RTD_OK, "blend: a good call after the refusals"
        s.run(3)
        for p, v in enumerate(good):
            opt, obj = rig.plain(v)
            opt.run(3)
            r, _ = rig.same_as_plain(s, p, opt, obj)
            assert r["iterations"] == 3, "plan %d: %r" % (p, r)
        # a matrix replaced after the set was made (a threshold gives another matrix with another number of chunks), prepared again: the
        # set's chunk sums are sized for the matrix it was created on, so run refuses before its first launch, every time
        s2 = rig.planset(good)
        s2.run(1)
        before = f.dose_influence_device()[3]
        d2 = f.dose_influence(0.05)
        print("matrix replaced: %d entries, then %d" % (before, d2.nnz))
        assert 0 < d2.nnz < before, "the threshold did not change the matrix: %d then %d entries" % (before, d2.nnz)
        assert L.rtd_planset_run(h, s2._h, 1) == abi.RTD_ERR_NOT_READY, "run after the matrix was replaced, not prepared"
        f.dose_influence_prepare()
        assert L.rtd_planset_run(h, s2._h, 1) == abi.RTD_ERR_NOT_READY, "run after the matrix was replaced and prepared"
        f.dose_influence()                                            # the first matrix's entries again, but another matrix to the set
        f.dose_influence_prepare()
        assert L.rtd_planset_run(h, s2._h, 1) == abi.RTD_ERR_NOT_READY, "run after the matrix was computed again"
        assert L.rtd_planset_run(h, s._h, 1) == abi.RTD_ERR_NOT_READY, "the other set of the same field"
        assert s2.result(0)[0]["iterations"] == 1 and s.result(0)[0]["iterations"] == 3, "a refused run advanced a set"
        s3 = rig.planset(good)                                        # a new set on the new matrix works
        s3.run(2)
        assert s3.result(1)[0]["iterations"] == 2 and np.all(np.isfinite(s3.result(1)[1])), "a set created on the new matrix"
        # an ROI added to the objective after the set was made, with voxels the union did not have, and the objective evaluated since
        # (which rebuilds its tables, with more blocks and the same number of terms): the set's block sums are sized for the objective
        # it was created on, so run refuses before its first launch
        union = np.zeros(rig.nvox, dtype=bool)
        for r in rig.ref.rois:
            union[r] = True
        extra = np.flatnonzero(~union)[:4096]
        dG2 = rig.alloc(4 * nvox)
        blocks_before = -(-int(union.sum()) // 256)
        rig.obj.add_roi(extra)
        assert L.rtd_planset_run(h, s3._h, 1) == abi.RTD_ERR_NOT_READY, "run after an ROI was added, the objective not evaluated since"
        vals = rig.obj.eval(dVol, dG2)
        blocks_after = -(-(int(union.sum()) + extra.size) // 256)
        print("ROI of %d new voxels added and the objective evaluated: %d -> %d blocks of union voxels, %d terms" % (extra.size, blocks_before, blocks_after, vals.size - 1))
        assert extra.size == 4096 and blocks_after > blocks_before and vals.size - 1 == nT, "the ROI did not grow the union: %d -> %d blocks" % (blocks_before, blocks_after)
        assert L.rtd_planset_run(h, s3._h, 1) == abi.RTD_ERR_NOT_READY, "run after an ROI was added and the objective evaluated"
        assert s3.result(0)[0]["iterations"] == 2, "a refused run advanced the set"
        # a term added to the objective after the set was made: run refuses before its first launch, the set's state stands
        rig.obj.add_term(R.MEAN, 1, 1.0, 0.0)
        assert L.rtd_planset_run(h, s3._h, 1) == abi.RTD_ERR_NOT_READY, "run after the objective changed"
        assert s3.result(0)[0]["iterations"] == 2, "a refused run advanced the set"
        assert nT == 4, "the rig's objective has %d terms" % nT
    finally:
        rig.close()
