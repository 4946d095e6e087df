"""GPU tests of the dose-volume entry points (rtd_objective_add_dvh_term, rtd_objective_dose_at_volume, rtd_objective_dvh; include/rtd.h,
DESIGN.md section 13) through the C ABI, against their numpy restatement (tests/dvh_reference.py), on the 96^3, 75-spot heterogeneous
field of the optimiser tests.

Bounds (derived, not measured). Dose at volume and the histogram are exact: bits and integers. Values and gradient of eval: as in
test_gpu_objective.py (a float64 sum of N non-negative numbers in any order: N * 2^-52 relative; the gradient one float32 rounding of a
float64 sum of at most 64 products), given that the device and the restatement select the same D, which the first test establishes."""
import ctypes as C
import math

import numpy as np
import pytest

import dvh_reference as D
import optimizer_reference as R
from gpu_plan_rigs import OptimizerRig
from gpu_support import bits, hetero_scene, rig_fixture
from raytracedicom_amd import abi

pytestmark = pytest.mark.gpu

NAN_BITS = np.uint32(0x7FC00123)
FRACTIONS = (None, 0.02, 0.5, 0.95, 0.98, 1.0)        # None: 1 / N of the ROI


class DvhRig(OptimizerRig):
    """The engine, fields and matrices of the optimiser tests' rig, with objectives of this file's own making beside them."""

    def __init__(self, engine, scn):
        super().__init__(engine, scn)
        self.objs = []
        self.dose_true = self.matvec(np.concatenate([w.reshape(-1) for w in self.w_true]))
        self.has = sum(np.bincount(d.indices, minlength=self.nvox) for d in self.mats) > 0
        self.target = self.dose_true > 0.5 * self.dose_true.max()
        self.other = self.has & ~self.target

    def objective(self, rois, terms):
        """terms: (kind, roi, weight, level) or, for the DVH kinds, (kind, roi, weight, level, fraction) -> (device, restated)."""
        obj, ref = self.eng.create_objective(self.dims), D.DvhReferenceObjective(self.nvox)
        self.objs.append(obj)
        for k, m in enumerate(rois):
            assert obj.add_roi(m) == k == ref.add_roi(m)
        for t in terms:
            for o in (obj, ref):
                (o.add_dvh_term if len(t) == 5 else o.add_term)(*t)
        return obj, ref

    def optimizer_of(self, obj, start=None):
        o = self.eng.create_optimizer(self.fields, obj, None)
        self.opts.append(o)
        if start is not None:
            self.set_weights(o, start)
        return o

    def upload(self, vol):
        p = self.alloc(4 * self.nvox, zero=False)
        self.eng.to_device(p, np.ascontiguousarray(vol, dtype=np.float32).reshape(-1))
        return p

    def field_dose(self):
        """The dose of w_true through apply, on the device and on the host."""
        p = self.alloc(4 * self.nvox)
        self.dose_of(self.w_true, p)
        return p, self.volume(p)

    def close(self):
        for o in self.opts:
            o.destroy()
        self.opts = []
        for o in self.objs:
            o.destroy()
        super().close()


rig_of = rig_fixture(DvhRig)


def _four_rois(rig):
    """The target, the voxels with rows (which contain it), one voxel, and scattered voxels that cut across the others."""
    one = np.zeros(rig.nvox, dtype=bool)
    one[int(np.flatnonzero(rig.target)[7])] = True
    scattered = np.random.default_rng(31).random(rig.nvox) < 0.03
    rois = [rig.target, rig.has, one, scattered]
    sizes = [int(m.sum()) for m in rois]
    assert any(n % 256 for n in sizes) and sizes[2] == 1 and (rig.target & scattered).any() and (scattered & ~rig.has).any()
    return rois, sizes


def _queries(sizes):
    return [(r, 1.0 / n if v is None else v) for r, n in enumerate(sizes) for v in FRACTIONS]


def test_dose_at_volume_is_the_kth_largest_bit_for_bit(engine, rig_of, synth):
    """Every ROI x fraction in one call, on the field's dose and on a volume of 16 distinct values (ties everywhere); the same bits
    from a second call, from a second engine and from a replayed graph; 64 queries in one call."""
    import torch
    scn = hetero_scene(synth, 96, (0.0,))
    rig = rig_of(scn)
    rois, sizes = _four_rois(rig)
    obj, ref = rig.objective(rois, [])
    qs = _queries(sizes)
    assert len(qs) == 24
    dField, field = rig.field_dose()
    levels = (np.float32(0.125) * np.arange(16, dtype=np.float32))
    ties = levels[np.random.default_rng(32).integers(0, 16, rig.nvox)]
    assert field[rig.target].min() > 0 and np.unique(field[rig.has]).size > 1000
    got = {}
    for name, dev, vol in (("field", dField, field), ("ties", rig.upload(ties), ties)):
        want = ref.dose_at_volume(vol, qs)
        got[name] = obj.dose_at_volume(dev, qs)
        for (r, v), a, b in zip(qs, got[name], want):
            print("%s: ROI %d (N %d), v %.6g, k %d: device %.9g restated %.9g" % (name, r, sizes[r], v, D.rank(v, sizes[r]), a, b))
        assert got[name].dtype == np.float32 and np.array_equal(bits(got[name]), bits(want)), name
        assert np.array_equal(bits(obj.dose_at_volume(dev, qs)), bits(want))              # the histograms were left clear
    for r, n in enumerate(sizes):                                                           # v = 1 the minimum, 1 / N the maximum
        dv = field[rois[r].reshape(-1)]
        assert got["field"][6 * r] == dv.max() and got["field"][6 * r + 5] == dv.min()
    many = [(r % 4, (1 + r) / 64.0) for r in range(64)]
    assert np.array_equal(bits(obj.dose_at_volume(dField, many)), bits(ref.dose_at_volume(field, many)))
    # a second engine
    other = rig_of(scn)
    obj2, _ = other.objective(rois, [])
    dField2, field2 = other.field_dose()
    assert np.array_equal(bits(field2), bits(field))
    assert np.array_equal(bits(obj2.dose_at_volume(dField2, qs)), bits(got["field"]))
    # a graph: the call is launches only
    dOut = rig.alloc(4 * 64)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    rig.eng.sync()
    rig.eng.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            assert obj.dose_at_volume(dField, qs, dev_out=dOut) is None
        g.replay()
    torch.cuda.synchronize()
    rig.eng.set_stream(None)
    out = np.empty(64, dtype=np.float32)
    rig.eng.to_host(out, dOut)
    assert np.array_equal(bits(out[:24]), bits(got["field"]))


def test_cumulative_histogram_is_exact(rig_of, synth):
    """counts[roi][b] = #(double(d) >= (b * dose_max) / n_bins), as integers: on the field's dose with voxels set to the float32
    nearest to edges (just below, on or just above them) and doses above dose_max; on a volume whose values are edges exactly."""
    rig = rig_of(hetero_scene(synth, 96, (0.0,)))
    rois, sizes = _four_rois(rig)
    obj, ref = rig.objective(rois, [])
    _, field = rig.field_dose()
    top = float(field.max())
    tgt = np.flatnonzero(rig.has)[::5]                                # voxels of ROI 1 (some of ROIs 0 and 3 among them) that get planted values
    assert tgt.size >= 320
    for n_bins, dose_max in ((100, 0.6 * top), (4096, 1.01 * top), (1, top), (333, 0.37 * top)):
        vol = field.copy()
        edges = np.arange(n_bins, dtype=np.float64) * dose_max / n_bins
        pick = np.random.default_rng(n_bins).integers(0, n_bins, 200)
        vol[tgt[:200]] = edges[pick].astype(np.float32)
        vol[tgt[200:260]] = np.nextafter(edges[pick[:60]].astype(np.float32), np.float32(np.inf))
        vol[tgt[260:320]] = np.nextafter(edges[pick[:60]].astype(np.float32), np.float32(-np.inf))
        assert (vol[rig.has] > dose_max).any() == (dose_max < top)
        got = obj.dvh(rig.upload(vol), n_bins, dose_max)
        want = ref.dvh(vol, n_bins, dose_max)
        assert got.shape == (4, n_bins) and got.dtype == np.uint32
        np.testing.assert_array_equal(got, want)
        assert list(got[:, 0]) == sizes or (vol < 0).any()
    sixteenths = (np.float32(0.0625) * np.random.default_rng(5).integers(0, 24, rig.nvox).astype(np.float32))   # 0 .. 1.4375: on the edges of 16 bins over [0, 1), and above
    got = obj.dvh(rig.upload(sixteenths), 16, 1.0)
    np.testing.assert_array_equal(got, ref.dvh(sixteenths, 16, 1.0))
    for r, m in enumerate(rois):
        np.testing.assert_array_equal(got[r], (sixteenths[m][:, None].astype(np.float64) >= (np.arange(16) / 16.0)[None, :]).sum(0))


def _eval(rig, obj, dDose):
    dG = rig.alloc(4 * rig.nvox, zero=False)
    rig.eng.to_device(dG, np.full(rig.nvox, NAN_BITS, dtype=np.uint32))
    values = obj.eval(dDose, dG)
    return values, rig.volume(dG)


def test_eval_with_mixed_terms_on_overlapping_rois(rig_of, synth):
    rig = rig_of(hetero_scene(synth, 96, (0.0,)))
    rois, sizes = _four_rois(rig)
    dField, field = rig.field_dose()
    # the dose of a plan in the making: the field's dose, modulated so that both DVH constraints are violated
    rng = np.random.default_rng(33)
    dose = (field * (0.7 + 0.5 * rng.random(rig.nvox))).astype(np.float32)
    dDose = rig.upload(dose)
    L = float(field[rig.target].mean())
    probe = D.DvhReferenceObjective(rig.nvox)
    for m in rois:
        probe.add_roi(m)
    d25, d002 = (float(x) for x in probe.dose_at_volume(dose, [(1, 0.25), (3, 0.002)]))
    assert d25 > 0 and d002 > 0                                       # levels at half of these: both MAX_DVH statements are violated
    terms = [(R.SQ_DEVIATION, 0, 1.0, L), (D.MIN_DVH, 0, 5.0, 0.95 * L, 0.98), (D.MAX_DVH, 1, 3.0, 0.5 * d25, 0.25), (R.SQ_OVERDOSE, 1, 1.0, 0.5 * L),
             (D.MAX_DVH, 3, 2.0, 0.5 * d002, 0.002), (R.MEAN, 3, 1e-3 * L, 0.0), (D.MIN_DVH, 2, 1.0, 2.0 * L, 1.0), (D.MAX_DVH, 0, 1.0, 10.0 * L, 0.5)]
    obj, ref = rig.objective(rois, terms)
    values, g = _eval(rig, obj, dDose)
    v2, g2 = _eval(rig, obj, dDose)
    assert np.array_equal(bits(values), bits(v2)) and np.array_equal(bits(g), bits(g2))
    rv, rg, gabs = ref.eval(dose)
    union = ref.union()
    assert np.all(bits(g)[~union] == NAN_BITS) and 0 < union.sum() < rig.nvox
    assert rv[8] == 0.0 and np.all(rv[1:8] > 0)                      # the last term is satisfied, the others cost
    nt = [sizes[t[1]] for t in terms]
    for t, n in enumerate(nt):
        rel = abs(values[1 + t] - rv[1 + t]) / rv[1 + t] if rv[1 + t] else abs(values[1 + t])
        print("term %d (kind %d): N %d, gpu %.17g ref %.17g, relative difference %.3g of the bound %.3g"
              % (t, terms[t][0], n, values[1 + t], rv[1 + t], rel, n * 2.0 ** -52))
        assert rel <= n * 2.0 ** -52, t
    assert abs(values[0] - rv[0]) <= (max(nt) + len(terms)) * 2.0 ** -52 * rv[0]
    err = np.abs(g[union].astype(np.float64) - rg[union])
    bound = 2.0 ** -24 * np.abs(rg[union]) + 64 * 2.0 ** -52 * gabs[union]
    print("gradient: worst |gpu - ref| / bound = %.3g over %d voxels" % (float(np.max(err / np.maximum(bound, 1e-300))), int(union.sum())))
    assert np.all(err <= bound) and np.abs(rg[union]).max() > 0
    # the plain kinds are what they were: alone, and beside a DVH term on a ROI disjoint from theirs
    disjoint = ~rig.has
    disjoint[: rig.nvox // 2] = False
    disjoint &= ~rois[3]
    plain = [(R.SQ_DEVIATION, 0, 1.0, L), (R.SQ_UNDERDOSE, 0, 5.0, 0.95 * L), (R.SQ_OVERDOSE, 1, 1.0, 0.3 * L), (R.MEAN, 3, 1e-3 * L, 0.0)]
    five = rois + [disjoint]
    alone, _ = rig.objective(five, plain)
    beside, _ = rig.objective(five, plain + [(D.MAX_DVH, 4, 1.0, -1.0, 0.5)])
    va, ga = _eval(rig, alone, dDose)
    vb, gb = _eval(rig, beside, dDose)
    theirs = rig.has | rois[3]
    assert disjoint.sum() > 1000 and not (disjoint & theirs).any()
    assert np.array_equal(bits(va[1:5]), bits(vb[1:5])) and np.array_equal(bits(ga[theirs]), bits(gb[theirs]))
    assert vb[5] > 0 and vb[0] == va[0] + vb[5] and np.all(gb[disjoint & (dose <= 0)] > 0)


def test_refusals_leave_the_objective_usable(engine):
    L = engine.lib()
    eng = engine.Engine(0)
    try:
        obj = eng.create_objective((4, 4, 4))
        h, o = eng._h, obj._h
        assert obj.add_roi(np.array([0, 5, 63])) == 0
        dD, dOut, dCnt = eng.device_alloc(4 * 64), eng.device_alloc(4 * 64), eng.device_alloc(4 * 4096)
        dose = np.zeros(64, dtype=np.float32)
        dose[[0, 5, 63]] = (3.0, 1.0, 2.0)
        eng.to_device(dD, dose)
        T, Q, P = abi.RtdObjectiveDvhTerm, abi.RtdDvhQuery, abi.RtdObjectiveTerm
        nan, inf = float("nan"), float("inf")
        for bad in (T(0, 0, 1.0, 1.0, 0.5), T(3, 0, 1.0, 1.0, 0.5), T(6, 0, 1.0, 1.0, 0.5), T(-1, 0, 1.0, 1.0, 0.5), T(4, 1, 1.0, 1.0, 0.5),
                    T(5, -1, 1.0, 1.0, 0.5), T(4, 0, 0.0, 1.0, 0.5), T(4, 0, -1.0, 1.0, 0.5), T(4, 0, nan, 1.0, 0.5), T(4, 0, inf, 1.0, 0.5),
                    T(4, 0, 1.0, nan, 0.5), T(5, 0, 1.0, inf, 0.5), T(4, 0, 1.0, 1.0, 0.0), T(4, 0, 1.0, 1.0, -0.5), T(5, 0, 1.0, 1.0, 1.0000001),
                    T(4, 0, 1.0, 1.0, nan)):
            assert L.rtd_objective_add_dvh_term(h, o, C.byref(bad)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_add_dvh_term(h, o, None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_add_dvh_term(h, None, C.byref(T(4, 0, 1.0, 1.0, 0.5))) == abi.RTD_ERR_INVALID_ARG
        for kind in (4, 5):                                           # the plain entry point keeps refusing the DVH kinds
            assert L.rtd_objective_add_term(h, o, C.byref(P(kind, 0, 1.0, 1.0))) == abi.RTD_ERR_INVALID_ARG
        dV = eng.device_alloc(8 * 65)
        assert L.rtd_objective_eval(h, o, dD, dV, dOut) == abi.RTD_ERR_INVALID_ARG          # still no terms
        q1 = (Q * 65)(*[Q(0, 0, 0.5)] * 65)
        assert L.rtd_objective_dose_at_volume(h, o, dD, q1, 0, dOut) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_dose_at_volume(h, o, dD, q1, 65, dOut) == abi.RTD_ERR_INVALID_ARG
        for args in ((None, q1, 1, dOut), (dD, None, 1, dOut), (dD, q1, 1, None)):
            assert L.rtd_objective_dose_at_volume(h, o, *args) == abi.RTD_ERR_INVALID_ARG
        for bad in (Q(1, 0, 0.5), Q(-1, 0, 0.5), Q(0, 0, 0.0), Q(0, 0, 1.5), Q(0, 0, nan)):
            assert L.rtd_objective_dose_at_volume(h, o, dD, (Q * 2)(Q(0, 0, 0.5), bad), 2, dOut) == abi.RTD_ERR_INVALID_ARG
        for args in ((None, 8, 4.0, dCnt), (dD, 8, 4.0, None), (dD, 0, 4.0, dCnt), (dD, 4097, 4.0, dCnt), (dD, 8, 0.0, dCnt), (dD, 8, -1.0, dCnt),
                     (dD, 8, inf, dCnt), (dD, 8, nan, dCnt)):
            assert L.rtd_objective_dvh(h, o, *args) == abi.RTD_ERR_INVALID_ARG
        # usable after all of them
        assert list(obj.dose_at_volume(dD, [(0, 1.0 / 3), (0, 0.5), (0, 1.0)])) == [3.0, 2.0, 1.0]
        assert list(obj.dvh(dD, 4, 4.0)[0]) == [3, 3, 2, 1]
        ok = T(abi.RTD_OBJ_MAX_DVH, 0, 3.0, 0.5, 0.5)                 # D = 2: the voxels at 1 and 2 pay (0.5^2 + 1.5^2) * 3 / 3
        plain = P(abi.RTD_OBJ_SQ_DEVIATION, 0, 3.0, 2.0)
        for i in range(64):
            assert (L.rtd_objective_add_dvh_term(h, o, C.byref(ok)) if i % 2 else L.rtd_objective_add_term(h, o, C.byref(plain))) == abi.RTD_OK
        assert L.rtd_objective_add_dvh_term(h, o, C.byref(ok)) == abi.RTD_ERR_INVALID_ARG   # the 65th, through either door
        assert L.rtd_objective_add_term(h, o, C.byref(plain)) == abi.RTD_ERR_INVALID_ARG
        dG = eng.device_alloc(4 * 64)
        eng.device_zero(dG, 4 * 64)
        assert L.rtd_objective_eval(h, o, dD, dV, dG) == abi.RTD_OK
        vals = np.empty(65, dtype=np.float64)
        eng.to_host(vals, dV)
        g = np.empty(64, dtype=np.float32)
        eng.to_host(g, dG)
        assert np.all(vals[1::2] == 2.0) and np.all(vals[2::2] == 2.5) and vals[0] == 32 * 4.5
        assert np.array_equal(np.flatnonzero(g), [0, 5, 63]) and list(g[[0, 5, 63]]) == [32 * 2.0, 32 * (-2.0 + 1.0), 32 * 3.0]
        obj.destroy()
        for p in (dD, dOut, dCnt, dV, dG):
            eng.device_free(p)
    finally:
        eng.close()


def _plan(rig):
    """The target at the mean L of the dose of w_true there, 98 % of it at 95 % of L at least, and at most a quarter of the surrounding
    rows above HALF of what w_true gives a quarter of them: a statement the plan that meets the target violates."""
    L = float(rig.dose_true[rig.target].mean())
    d25 = float(np.sort(rig.dose_true[rig.other].astype(np.float32))[::-1][D.rank(0.25, int(rig.other.sum())) - 1])
    assert 0 < d25 < L
    return rig.objective([rig.target, rig.other], [(R.SQ_DEVIATION, 0, 1.0, L), (D.MIN_DVH, 0, 5.0, 0.95 * L, 0.98), (D.MAX_DVH, 1, 3.0, 0.5 * d25, 0.25)])


def test_optimizer_iterations_against_the_restatement(rig_of, synth):
    """Iterations 0, 1 and 2 of the resident loop on a target term + MIN_DVH on the target + MAX_DVH on the surrounding rows, the
    restatement fed the device's own dose and gradient: f within the summation bound, alpha within (n + 2) * 2^-52 relative (as
    test_gpu_optimizer.py derives it), the weights bit for bit."""
    rig = rig_of(hetero_scene(synth, 96, (30.0,)))
    obj, ref = _plan(rig)
    f, n = rig.fields[0], rig.sizes[0]
    opt = rig.optimizer_of(obj)
    dG, dGrad = rig.alloc(4 * rig.nvox), rig.alloc(4 * n)
    w_prev = grad_prev = None
    nmax = max(r.size for r in ref.rois)
    for k in range(3):
        w = rig.weights(opt)[0].reshape(-1)
        opt.run(1)
        rep, hist = opt.result()
        dose = rig.volume(opt.dose())
        vals = obj.eval(opt.dose(), dG)
        f.dose_influence_apply_t(dG, dGrad)
        grad = np.empty(n, dtype=np.float32)
        rig.eng.to_host(grad, dGrad)
        assert rep["iterations"] == k + 1 and hist[k] == rep["f_last"] == vals[0]
        rv = ref.eval(dose)[0]
        print("iteration %d: terms on the device %s, restated %s" % (k, vals[1:], rv[1:]))
        assert rv[0] > 0 and abs(hist[k] - rv[0]) <= (nmax + 4) * 2.0 ** -52 * rv[0]
        a_ref = R.step_length(w, w_prev, grad, grad_prev, k > 0)
        rel = abs(rep["step"] - a_ref) / a_ref
        print("iteration %d: f %.9g, alpha %.17g on the device, %.17g restated: relative difference %.3g of the bound %.3g"
              % (k, hist[k], rep["step"], a_ref, rel, (n + 2) * 2.0 ** -52))
        assert a_ref > 0 and rel <= (n + 2) * 2.0 ** -52
        w_new = rig.weights(opt)[0].reshape(-1)
        assert np.array_equal(bits(w_new), bits(R.update(w, grad, rep["step"]))) and not np.array_equal(w_new, w)
        w_prev, grad_prev = w, grad


def test_optimizer_with_dvh_terms_stays_resident_and_converges(rig_of, synth):
    """run(30) = 3 x run(10) bit for bit; run(5) captured into a graph and replayed gives the bits of the direct call; and thirty
    iterations from w = 0 reduce the objective to within a factor 2 of what the restatement with float64 host products of the same
    matrix reaches in thirty (float32 products may send a non-monotone iteration along another path; both ratios are printed)."""
    import torch
    rig = rig_of(hetero_scene(synth, 96, (0.0,)))
    obj, ref = _plan(rig)
    a, b = rig.optimizer_of(obj, start=0.0), rig.optimizer_of(obj, start=0.0)
    a.run(30)
    ra, ha = a.result()
    for _ in range(3):
        b.run(10)
    rb, hb = b.result()
    assert ra == rb and ha.size == 30 and np.array_equal(bits(ha), bits(hb))
    for best in (False, True):
        assert np.array_equal(bits(rig.weights(a, best)[0]), bits(rig.weights(b, best)[0]))
    direct, captured = rig.optimizer_of(obj, start=0.0), rig.optimizer_of(obj, start=0.0)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    rig.eng.sync()
    rig.eng.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        direct.run(5)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            captured.run(5)
        g.replay()
    torch.cuda.synchronize()
    rd, hd = direct.result()
    rg, hg = captured.result()
    rig.eng.set_stream(None)
    assert rd == rg and hd.size == 5 and np.array_equal(bits(hd), bits(hg)) and np.array_equal(bits(hd), bits(ha[:5]))
    assert np.array_equal(bits(rig.weights(direct)[0]), bits(rig.weights(captured)[0]))
    host = R.ReferenceOptimizer(ref, rig.matvec, rig.rmatvec, np.zeros(rig.sizes[0])).run(30)
    dev_ratio, host_ratio = ra["f_best"] / ha[0], host.f_best / host.history[0]
    print("device: f_0 %.6g, f_best %.6g at iteration %d, ratio %.4g; restated with float64 products: f_0 %.6g, f_best %.6g at iteration %d, ratio %.4g"
          % (ha[0], ra["f_best"], ra["best_iteration"], dev_ratio, host.history[0], host.f_best, host.best_iteration, host_ratio))
    print("device history:", " ".join("%.4g" % v for v in ha))
    print("restated history:", " ".join("%.4g" % v for v in host.history))
    assert ra["guarded"] == 0 and math.isfinite(ra["f_best"]) and ra["f_best"] == ha.min()
    assert dev_ratio <= 2.0 * host_ratio
    # the OAR statement itself, on the best iterate's dose
    dDose = rig.alloc(4 * rig.nvox)
    rig.dose_of(rig.weights(a, best=True), dDose)
    d_target, d_oar = obj.dose_at_volume(dDose, [(0, 0.98), (1, 0.25)])
    print("at w_best: D98 of the target %.4g (asked: >= %.4g), D25 of the surrounding rows %.4g (asked: <= %.4g)"
          % (d_target, ref.terms[1][3], d_oar, ref.terms[2][3]))
