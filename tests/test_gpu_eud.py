"""GPU tests of the EUD entry points (rtd_objective_add_eud_term, rtd_objective_eud; include/rtd.h) through the
C ABI, against their numpy restatement (tests/eud_reference.py), on the 96^3, 75-spot heterogeneous field of the optimiser tests.

The bound (derived, not measured). The device and the restatement follow the same steps in float64; they differ in the order of the
sum and in pow. With u = 2^-52:
  * a sum of N positive float64 numbers differs from the exact sum, in any order, by at most N u relative;
  * pow: the ROCm installation's headers and documents give no ulp figure for the device library's float64 pow (the only figures in
    its OpenCL header are those of the half_ and native_ functions), so p = 16 ulp is taken, the limit OpenCL sets for pow. The
    restatement's own pow (the host C library's, below 1 ulp) is well inside what is left of that.
So S = sum p_i / N carries dS = (N + p) u relative (every p_i within p u, the sum within N u, the division within u, counted into
p); E = L pow(S, 1 / a) carries dE = dS / |a| + (p + 2) u (the power divides the relative error of S by |a|; 1 / a, the pow and the
product with L are one rounding, p ulp and one rounding). A term's value weight y^2 with y = E - L carries 2 dE E / |y| + 4 u
relative: the subtraction turns the error dE E of E into a relative error dE E / |y| of y, twice in the square, and the products
round. The tests therefore keep |E - L| >= 0.1 L for terms that are not satisfied. K = ((2 weight y) E) / ((L N) S) carries
dE E / |y| + dE + dS + 6 u, and K (p_i / x_i) adds p + 2 ulp: dG = dE E / |y| + dE + dS + (p + 8) u relative per contribution.
The other kinds are as in test_gpu_dvh.py: N u on a value; the gradient one float32 rounding of a float64 sum of at most 64 products.
A float32 rounding is 2^-24 relative or, for the subnormal gradients that K (p / x) reaches at voxels with 1e-5 of the level, half a
subnormal step, 2^-150.
Every comparison prints measured error over bound."""
import ctypes as C
import math

import numpy as np
import pytest

import eud_reference as E
import optimizer_reference as R
from gpu_plan_rigs import OptimizerRig
from gpu_support import bits, hetero_scene, rig_fixture
from raytracedicom_amd import abi, robust

pytestmark = pytest.mark.gpu

NAN_BITS = np.uint32(0x7FC00123)
U = 2.0 ** -52
P_ULP = 16.0
CHUNK = 2048                                          # kEudChunk of rtd_eud.hpp
EXPONENTS = (-20.0, -1.0, 0.0625, 1.0, 2.0, 8.0, 64.0)


def d_s(n):
    return (n + P_ULP) * U


def d_e(n, a):
    return d_s(n) / abs(a) + (P_ULP + 2) * U


def d_value(n, a, e, level):
    return 2.0 * d_e(n, a) * e / abs(e - level) + 4 * U


def d_grad(n, a, e, level):
    return d_e(n, a) * e / abs(e - level) + d_e(n, a) + d_s(n) + (P_ULP + 8) * U


class EudRig(OptimizerRig):
    """The engine, fields and matrices of the optimiser tests' rig, with objectives of this file's own making beside them and, on
    demand, two more scenarios (the patient displaced by +-5 mm across the beam) for the robust test."""

    def __init__(self, engine, scn):
        super().__init__(engine, scn)
        self.scn = scn
        self.objs = []
        self.extra = []
        self.dose_true = self.matvec(np.concatenate([w.reshape(-1) for w in self.w_true]))
        self.has = sum(np.bincount(d.indices, minlength=self.nvox) for d in self.mats) > 0
        self.target = self.dose_true > 0.5 * self.dose_true.max()
        self.other = self.has & ~self.target

    def objective(self, rois, terms):
        """terms: (kind, roi, weight, level), (kind, roi, weight, level, fraction) for the DVH kinds or (kind, roi, weight, level,
        exponent) for the EUD kinds -> (device, restated)."""
        obj, ref = self.eng.create_objective(self.dims), E.EudReferenceObjective(self.nvox)
        self.objs.append(obj)
        for k, m in enumerate(rois):
            assert obj.add_roi(m) == k == ref.add_roi(m)
        for t in terms:
            for o in (obj, ref):
                (o.add_term if len(t) == 4 else o.add_eud_term if t[0] >= E.SQ_EUD else o.add_dvh_term)(*t)
        return obj, ref

    def optimizer_of(self, obj, start=None):
        o = self.eng.create_optimizer(self.fields, obj, None)
        self.opts.append(o)
        if start is not None:
            self.set_weights(o, start)
        return o

    def three_scenarios(self):
        if not self.extra:
            for beams in robust.scenario_beams(self.scn.beams, [(5.0, 0.0, 0.0), (-5.0, 0.0, 0.0)]):
                fs = [self.eng.create_field(b, self.dims) for b in beams]
                for f in fs:
                    f.dose_influence()
                self.extra.append(fs)
        return [self.fields] + self.extra

    def upload(self, vol):
        p = self.alloc(4 * self.nvox, zero=False)
        self.eng.to_device(p, np.ascontiguousarray(vol, dtype=np.float32).reshape(-1))
        return p

    def field_dose(self):
        """The dose of w_true through apply, on the device and on the host."""
        p = self.alloc(4 * self.nvox)
        self.dose_of(self.w_true, p)
        return p, self.volume(p)

    def plan(self):
        """Test 3's objective: the target at the mean L of the dose of w_true there, its cold-spot dose (a = -10) at 95 % of L at
        least, and the near-maximum (a = 8) of the other voxels with rows at most 0.8 of what w_true gives them: a statement the plan
        that meets the target violates."""
        L = float(self.dose_true[self.target].mean())
        e_other = E.geud(self.dose_true[self.other], L, 8.0)[0]
        assert 0 < e_other < L
        return self.objective([self.target, self.other], [(R.SQ_DEVIATION, 0, 1.0, L), (E.SQ_MIN_EUD, 0, 5.0, 0.95 * L, -10.0),
                                                          (E.SQ_MAX_EUD, 1, 3.0, 0.8 * e_other, 8.0)])

    def close(self):
        for o in self.opts:
            o.destroy()
        self.opts = []
        for o in self.objs:
            o.destroy()
        for fs in self.extra:
            for f in fs:
                f.destroy()
        super().close()


rig_of = rig_fixture(EudRig)


def _rois(rig):
    """The target, the voxels with rows (which contain it), one voxel, scattered voxels (3 %) that cut across the others and include
    voxels without dose, the whole grid, and three ROIs of one voxel less than a chunk, a chunk and one voxel more."""
    one = np.zeros(rig.nvox, dtype=bool)
    one[int(np.flatnonzero(rig.target)[7])] = True
    scattered = np.random.default_rng(31).random(rig.nvox) < 0.03
    whole = np.ones(rig.nvox, dtype=bool)
    hv = np.flatnonzero(rig.has)
    assert hv.size > 3 * CHUNK
    chunks = []
    for lo, n in ((0, CHUNK - 1), (100, CHUNK), (hv.size - CHUNK - 1, CHUNK + 1)):
        m = np.zeros(rig.nvox, dtype=bool)
        m[hv[lo:lo + n]] = True
        chunks.append(m)
    rois = [rig.target, rig.has, one, scattered, whole] + chunks
    sizes = [int(m.sum()) for m in rois]
    assert sizes[2] == 1 and sizes[5:] == [CHUNK - 1, CHUNK, CHUNK + 1] and (scattered & ~rig.has).any() and (rig.target & scattered).any()
    assert (sizes[4] + CHUNK - 1) // CHUNK == 432                    # more chunks than k_eud_finish has threads: its strided loop wraps
    return rois, sizes


def _eval(rig, obj, dDose):
    dG = rig.alloc(4 * rig.nvox, zero=False)
    rig.eng.to_device(dG, np.full(rig.nvox, NAN_BITS, dtype=np.uint32))
    values = obj.eval(dDose, dG)
    return values, rig.volume(dG)


def test_eud_against_the_restatement(engine, rig_of, synth):
    """Every ROI x exponent in one call (56 queries), on the field's dose and on a volume with planted values above 2^15 L, negative
    values and exact zeros: within dE of the restatement. The same bits from a second call, a second engine and a replayed graph. A
    NaN inside ROIs makes exactly those ROIs' results NaN and leaves the others' bits alone."""
    import torch
    scn = hetero_scene(synth, 96, (0.0,))
    rig = rig_of(scn)
    rois, sizes = _rois(rig)
    obj, ref = rig.objective(rois, [])
    dField, field = rig.field_dose()
    L = float(field[rig.target].mean())
    qs = [(r, L, a) for r in range(len(rois)) for a in EXPONENTS]
    assert len(qs) == 56
    hv = np.flatnonzero(rig.has)
    planted = field.copy()
    planted[hv[0::7][:60]] = np.float32(2.0 ** 16 * L)
    planted[hv[3::7][:60]] = np.float32(-L)
    planted[hv[5::7][:60]] = 0.0
    assert np.isfinite(planted).all() and (field[rois[3]] == 0).any() and (planted[rois[5]] > 2.0 ** 15 * L).any() and (planted[rois[5]] < 0).any()
    got = {}
    for name, dev, vol in (("field", dField, field), ("planted", rig.upload(planted), planted)):
        want = ref.eud(vol, qs)
        got[name] = obj.eud(dev, qs)
        assert got[name].dtype == np.float64 and got[name].shape == (56,)
        worst = 0.0
        for (r, _, a), x, y in zip(qs, got[name], want):
            rel, bound = abs(x - y) / y, d_e(sizes[r], a)
            worst = max(worst, rel / bound)
            print("%s: ROI %d (N %d), a %g: device %.17g restated %.17g, relative difference %.3g of the bound %.3g" % (name, r, sizes[r], a, x, y, rel, bound))
            assert y > 0 and rel <= bound, (name, r, a)
        print("%s: worst error over bound %.3g" % (name, worst))
        assert np.array_equal(bits(obj.eud(dev, qs)), bits(got[name]))                    # a second call
    for r in range(len(rois)):                                                              # ordered in a, between the clamped extremes
        e = got["field"][7 * r:7 * r + 7]
        assert np.all(np.diff(e) >= -8 * d_e(sizes[r], 0.0625) * e[:-1]), r
    # a second engine
    other = rig_of(scn)
    obj2, _ = other.objective(rois, [])
    dField2, field2 = other.field_dose()
    assert np.array_equal(bits(field2), bits(field))
    assert np.array_equal(bits(obj2.eud(dField2, qs)), bits(got["field"]))
    # a graph: the call is launches only
    dOut = rig.alloc(8 * 64)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    rig.eng.sync()
    rig.eng.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            assert obj.eud(dField, qs, dev_out=dOut) is None
        g.replay()
    torch.cuda.synchronize()
    rig.eng.set_stream(None)
    out = np.empty(64, dtype=np.float64)
    rig.eng.to_host(out, dOut)
    assert np.array_equal(bits(out[:56]), bits(got["field"]))
    # one NaN: in the last voxel with rows, which the last chunk ROI, the voxels with rows and the whole grid hold
    v = int(hv[-1])
    holds = [bool(m[v]) for m in rois]
    assert holds[1] and holds[4] and holds[7] and not holds[2] and not holds[5] and not holds[6]
    with_nan = field.copy()
    with_nan[v] = np.nan
    e = obj.eud(rig.upload(with_nan), qs)
    for q, (r, _, a) in enumerate(qs):
        assert math.isnan(e[q]) if holds[r] else bits(e[q:q + 1])[0] == bits(got["field"][q:q + 1])[0], (r, a)


def test_eval_with_mixed_terms_on_overlapping_rois(rig_of, synth):
    """All three EUD kinds (one satisfied) beside SQ_DEVIATION, MEAN and a MIN_DVH term on the target, the voxels with rows, one voxel
    and the scattered voxels; the scattered ROI holds voxels without dose (clamped low) and planted ones above 2^15 L (clamped high)."""
    rig = rig_of(hetero_scene(synth, 96, (0.0,)))
    rois, sizes = _rois(rig)
    rois, sizes = rois[:4], sizes[:4]
    _, field = rig.field_dose()
    L = float(field[rig.target].mean())
    rng = np.random.default_rng(33)
    dose = (field * (0.7 + 0.5 * rng.random(rig.nvox))).astype(np.float32)
    only3 = np.flatnonzero(rois[3] & ~rig.has)                        # voxels of the scattered ROI alone: no dose, no other term
    assert only3.size > 100 and not dose[only3].any()
    high = only3[:5]
    dose[high] = np.float32(2.0 ** 16 * L)
    dDose = rig.upload(dose)
    probe = E.EudReferenceObjective(rig.nvox)
    for m in rois:
        probe.add_roi(m)
    e_t, e_has, e_sc, e_one = probe.eud(dose, [(0, L, -10.0), (1, L, 8.0), (3, L, 2.0), (2, L, 8.0)])
    terms = [(R.SQ_DEVIATION, 0, 1.0, L), (E.SQ_MIN_EUD, 0, 5.0, e_t / 0.8, -10.0), (R.MEAN, 3, 1e-3 * L, 0.0), (E.SQ_MAX_EUD, 1, 3.0, 0.5 * e_has, 8.0),
             (E.MIN_DVH, 0, 5.0, 0.95 * L, 0.98), (E.SQ_EUD, 3, 2.0, L, 2.0), (E.SQ_MAX_EUD, 2, 1.0, 10.0 * L, 8.0)]
    eud_terms = [t for t in range(len(terms)) if len(terms[t]) == 5 and terms[t][0] >= E.SQ_EUD]
    assert eud_terms == [1, 3, 5, 6] and e_one < 10.0 * L and abs(e_sc - L) >= 0.1 * L
    obj, ref = rig.objective(rois, terms)
    values, g = _eval(rig, obj, dDose)
    v2, g2 = _eval(rig, obj, dDose)
    assert np.array_equal(bits(values), bits(v2)) and np.array_equal(bits(g), bits(g2))
    rv, rg, gabs = ref.eval(dose)
    union = ref.union()
    assert np.all(bits(g)[~union] == NAN_BITS) and 0 < union.sum() < rig.nvox
    assert rv[7] == 0.0 and values[7] == 0.0 and not np.signbit(values[7]) and np.all(rv[1:7] > 0)
    d64 = dose.astype(np.float64)
    total, bg = 0.0, 64 * U
    for t, term in enumerate(terms):
        n = sizes[term[1]]
        if t in eud_terms:
            e = ref.eud_term(d64, t)[2]
            bound = d_value(n, term[4], e, term[3]) if rv[1 + t] else 0.0
            if rv[1 + t]:
                assert abs(e - term[3]) >= 0.1 * term[3], t
                bg = max(bg, d_grad(n, term[4], e, term[3]))
        else:
            bound = n * U
        rel = abs(values[1 + t] - rv[1 + t]) / rv[1 + t] if rv[1 + t] else abs(values[1 + t])
        print("term %d (kind %d): N %d, gpu %.17g ref %.17g, relative difference %.3g of the bound %.3g" % (t, term[0], n, values[1 + t], rv[1 + t], rel, bound))
        assert rel <= bound, t
        total += bound * rv[1 + t]
    assert abs(values[0] - rv[0]) <= total + len(terms) * U * rv[0]
    err = np.abs(g[union].astype(np.float64) - rg[union])
    bound = 2.0 ** -24 * gabs[union] + 2.0 ** -150 + bg * gabs[union]   # (2^-150: half a step of the float32 subnormals, which far voxels reach)
    print("gradient: worst |gpu - ref| / bound = %.3g over %d voxels (relative part of the bound %.3g)"
          % (float(np.max(err / np.maximum(bound, 1e-300))), int(union.sum()), bg))
    uidx = np.flatnonzero(union)
    for j in np.argsort(err / np.maximum(bound, 1e-300))[::-1][:3]:
        v = int(uidx[j])
        print("  worst voxel %d (in ROIs %s): dose %.9g = %.6g L, gpu %.9g ref %.17g, |difference| %.3g of the bound %.3g"
              % (v, [r for r, m in enumerate(rois) if m.reshape(-1)[v]], dose[v], dose[v] / L, g[v], rg[v], err[j], bound[j]))
    assert np.all(err <= bound) and np.abs(rg[union]).max() > 0
    # clamped voxels and the satisfied term: exactly what the other terms give
    plain, _ = rig.objective(rois, [terms[0], terms[2], terms[4]])
    _, gp = _eval(rig, plain, dDose)
    assert np.array_equal(bits(g[only3]), bits(gp[only3])) and np.all(g[only3] == np.float32(1e-3 * L / sizes[3]))
    unsatisfied, _ = rig.objective(rois, terms[:6])
    vu, gu = _eval(rig, unsatisfied, dDose)
    assert np.array_equal(bits(gu), bits(g)) and np.array_equal(bits(vu), bits(values[:7]))
    inside3 = np.flatnonzero(rois[3] & rig.target)
    assert not np.array_equal(bits(g[inside3]), bits(gp[inside3]))     # (where nothing is clamped the EUD terms do act)


def test_optimizer_iterations_against_the_restatement(rig_of, synth):
    """Iterations 0, 1 and 2 of the resident loop on test 3's objective from the fields' own weights, the restatement fed the device's
    own dose and gradient: the terms within their bounds, alpha within (n + 2) * 2^-52 relative (as test_gpu_optimizer.py derives it),
    the weights bit for bit; the voxel gradient equals the restatement's float32 one except where the two float64 sums round to
    different neighbours (counted, and one ulp apart at the most)."""
    rig = rig_of(hetero_scene(synth, 96, (0.0,)))
    obj, ref = rig.plan()
    f, n = rig.fields[0], rig.sizes[0]
    opt = rig.optimizer_of(obj)
    dG, dGrad = rig.alloc(4 * rig.nvox), rig.alloc(4 * n)
    w_prev = grad_prev = None
    sizes = [r.size for r in ref.rois]
    for k in range(3):
        w = rig.weights(opt)[0].reshape(-1)
        opt.run(1)
        rep, hist = opt.result()
        dose = rig.volume(opt.dose())
        vals = obj.eval(opt.dose(), dG)
        g = rig.volume(dG)
        f.dose_influence_apply_t(dG, dGrad)
        grad = np.empty(n, dtype=np.float32)
        rig.eng.to_host(grad, dGrad)
        assert rep["iterations"] == k + 1 and hist[k] == rep["f_last"] == vals[0]
        rv, rg, _ = ref.eval(dose)
        d64 = dose.astype(np.float64)
        total = sizes[0] * U * rv[1]
        for t in (1, 2):
            e, (_, roi, _, level), a = ref.eud_term(d64, t)[2], ref.terms[t], ref.expo[t]
            if rv[1 + t]:
                bound = d_value(sizes[roi], a, e, level)              # (the iterate decides how far E is from the level: the bound follows it)
                print("iteration %d, term %d: E %.9g, level %.9g, |E - level| / level %.3g" % (k, t, e, level, abs(e - level) / level))
                assert abs(vals[1 + t] - rv[1 + t]) <= bound * rv[1 + t], (k, t)
                total += bound * rv[1 + t]
            else:
                assert vals[1 + t] == 0.0, (k, t)
        print("iteration %d: terms on the device %s, restated %s" % (k, vals[1:], rv[1:]))
        assert rv[0] > 0 and abs(hist[k] - rv[0]) <= total + 4 * U * rv[0]
        union = ref.union()
        g32 = rg.astype(np.float32)
        differ = bits(g32[union]) != bits(g[union])
        ulps = np.abs(bits(g32[union]).astype(np.int64) - bits(g[union]).astype(np.int64))
        print("iteration %d: the voxel gradient differs from the restatement's float32 one at %d of %d voxels (one ulp each)"
              % (k, int(differ.sum()), int(union.sum())))
        assert ulps.max() <= 1 and int(differ.sum()) == int((ulps == 1).sum())
        a_ref = R.step_length(w, w_prev, grad, grad_prev, k > 0)
        rel = abs(rep["step"] - a_ref) / a_ref
        print("iteration %d: f %.9g, alpha %.17g on the device, %.17g restated: relative difference %.3g of the bound %.3g"
              % (k, hist[k], rep["step"], a_ref, rel, (n + 2) * U))
        assert a_ref > 0 and rel <= (n + 2) * U
        w_new = rig.weights(opt)[0].reshape(-1)
        assert np.array_equal(bits(w_new), bits(R.update(w, grad, rep["step"]))) and not np.array_equal(w_new, w)
        w_prev, grad_prev = w, grad


def test_optimizer_with_eud_terms_stays_resident_and_converges(rig_of, synth):
    """From w = 0: run(30) = 3 x run(10) bit for bit; run(5) captured into a graph and replayed gives the bits of the direct call; and
    thirty iterations reduce the objective to within a factor 2 of what the restatement with float64 host products of the same matrix
    reaches in thirty (section 13's convention; both ratios are printed)."""
    import torch
    rig = rig_of(hetero_scene(synth, 96, (0.0,)))
    obj, ref = rig.plan()
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
    # the two statements themselves, on the best iterate's dose
    dDose = rig.alloc(4 * rig.nvox)
    rig.dose_of(rig.weights(a, best=True), dDose)
    L = ref.terms[0][3]
    e_target, e_other = obj.eud(dDose, [(0, L, -10.0), (1, L, 8.0)])
    print("at w_best: gEUD(a = -10) of the target %.4g (asked: >= %.4g), gEUD(a = 8) of the other voxels with rows %.4g (asked: <= %.4g)"
          % (e_target, ref.terms[1][3], e_other, ref.terms[2][3]))


def test_robust_evaluates_per_scenario_and_voxelwise_refuses(engine, rig_of, synth):
    """A scenario-wise worst-case optimiser over three scenarios with test 3's objective: scenario_values()[s] is rtd_objective_eval
    on scenario_dose(s), bit for bit. The voxel-wise composite has no EUD: both of its entry points refuse the objective."""
    rig = rig_of(hetero_scene(synth, 96, (0.0,)))
    obj, _ = rig.plan()
    sf = rig.three_scenarios()
    opt = rig.eng.create_robust_optimizer(sf, obj, abi.RTD_ROBUST_WORST_CASE, None)
    rig.opts.append(opt)
    dG = rig.alloc(4 * rig.nvox)
    for k in range(2):
        opt.run(1)
        vals, lam, worst = opt.scenario_values()
        rep, hist = opt.result()
        mine = np.array([obj.eval(opt.scenario_dose(s), dG)[0] for s in range(3)])
        print("iteration %d: scenario values %s, worst %d" % (k, vals, worst))
        assert np.array_equal(bits(mine), bits(vals)) and np.all(np.isfinite(vals)) and len(set(vals)) == 3
        assert worst == int(np.argmax(vals)) and hist[k] == vals[worst] and rep["guarded"] == 0
    with pytest.raises(engine.RtdError) as ei:
        rig.eng.create_voxelwise_optimizer(sf, obj)
    assert ei.value.status == abi.RTD_ERR_INVALID_ARG and "has no voxel-wise worst case" in str(ei.value)
    doses = [opt.scenario_dose(s) for s in range(3)]
    grads = [rig.alloc(4 * rig.nvox) for _ in range(3)]
    with pytest.raises(engine.RtdError) as ei:
        obj.eval_voxelwise(doses, grads)
    assert ei.value.status == abi.RTD_ERR_INVALID_ARG and "has no voxel-wise worst case" in str(ei.value)
    assert np.array_equal(bits(np.array([obj.eval(d, dG)[0] for d in doses])), bits(mine))      # usable afterwards


def test_refusals_leave_the_objective_usable(engine):
    L = engine.lib()
    eng = engine.Engine(0)
    try:
        obj = eng.create_objective((4, 4, 4))
        h, o = eng._h, obj._h
        assert obj.add_roi(np.array([0, 5, 63])) == 0
        dD, dOut = eng.device_alloc(4 * 64), eng.device_alloc(8 * 64)
        dose = np.zeros(64, dtype=np.float32)
        dose[[0, 5, 63]] = (3.0, 1.0, 2.0)
        eng.to_device(dD, dose)
        T, Q, P, V = abi.RtdObjectiveEudTerm, abi.RtdEudQuery, abi.RtdObjectiveTerm, abi.RtdObjectiveDvhTerm
        nan, inf = float("nan"), float("inf")
        for bad in (T(5, 0, 1.0, 1.0, 2.0, 0.0), T(9, 0, 1.0, 1.0, 2.0, 0.0), T(0, 0, 1.0, 1.0, 2.0, 0.0), T(-1, 0, 1.0, 1.0, 2.0, 0.0),      # the kind
                    T(6, 1, 1.0, 1.0, 2.0, 0.0), T(7, -1, 1.0, 1.0, 2.0, 0.0),                                                                # the ROI
                    T(6, 0, 0.0, 1.0, 2.0, 0.0), T(6, 0, -1.0, 1.0, 2.0, 0.0), T(6, 0, nan, 1.0, 2.0, 0.0), T(8, 0, inf, 1.0, 2.0, 0.0),      # the weight
                    T(6, 0, 1.0, 0.0, 2.0, 0.0), T(6, 0, 1.0, -1.0, 2.0, 0.0), T(7, 0, 1.0, nan, 2.0, 0.0), T(6, 0, 1.0, inf, 2.0, 0.0),      # the level
                    T(6, 0, 1.0, 1.0, 0.0, 0.0), T(6, 0, 1.0, 1.0, 0.06, 0.0), T(6, 0, 1.0, 1.0, -0.06, 0.0), T(6, 0, 1.0, 1.0, 64.5, 0.0),   # the exponent
                    T(8, 0, 1.0, 1.0, -65.0, 0.0), T(6, 0, 1.0, 1.0, nan, 0.0), T(6, 0, 1.0, 1.0, inf, 0.0), T(6, 0, 1.0, 1.0, -inf, 0.0),
                    T(6, 0, 1.0, 1.0, 2.0, 1.0), T(6, 0, 1.0, 1.0, 2.0, nan)):                                                                # reserved
            assert L.rtd_objective_add_eud_term(h, o, C.byref(bad)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_add_eud_term(h, o, None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_add_eud_term(h, None, C.byref(T(6, 0, 1.0, 1.0, 2.0, 0.0))) == abi.RTD_ERR_INVALID_ARG
        for kind in (6, 7, 8):                                        # the two older entry points refuse the EUD kinds
            assert L.rtd_objective_add_term(h, o, C.byref(P(kind, 0, 1.0, 1.0))) == abi.RTD_ERR_INVALID_ARG
            assert L.rtd_objective_add_dvh_term(h, o, C.byref(V(kind, 0, 1.0, 1.0, 0.5))) == abi.RTD_ERR_INVALID_ARG
        dV = eng.device_alloc(8 * 65)
        dG = eng.device_alloc(4 * 64)
        eng.device_zero(dG, 4 * 64)
        assert L.rtd_objective_eval(h, o, dD, dV, dG) == abi.RTD_ERR_INVALID_ARG            # still no terms
        q1 = (Q * 65)(*[Q(0, 0, 1.0, 2.0)] * 65)
        assert L.rtd_objective_eud(h, o, dD, q1, 0, dOut) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_eud(h, o, dD, q1, 65, dOut) == abi.RTD_ERR_INVALID_ARG
        for args in ((None, q1, 1, dOut), (dD, None, 1, dOut), (dD, q1, 1, None)):
            assert L.rtd_objective_eud(h, o, *args) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_eud(h, None, dD, q1, 1, dOut) == abi.RTD_ERR_INVALID_ARG
        for bad in (Q(1, 0, 1.0, 2.0), Q(-1, 0, 1.0, 2.0), Q(0, 1, 1.0, 2.0), Q(0, 0, 0.0, 2.0), Q(0, 0, -1.0, 2.0), Q(0, 0, nan, 2.0), Q(0, 0, inf, 2.0),
                    Q(0, 0, 1.0, 0.0), Q(0, 0, 1.0, 0.0624), Q(0, 0, 1.0, 64.0001), Q(0, 0, 1.0, -100.0), Q(0, 0, 1.0, nan), Q(0, 0, 1.0, -inf)):
            assert L.rtd_objective_eud(h, o, dD, (Q * 2)(Q(0, 0, 1.0, 2.0), bad), 2, dOut) == abi.RTD_ERR_INVALID_ARG
        # usable after all of them; the ends of the exponent's range are inside it. The doses 3, 1, 2: the mean is 2 whatever L,
        # 3^(1 / 64) = 1.0173 at a = -64 and 3 * 3^(-1 / 64) = 2.949 at a = 64 to within the 2^+-64 the other voxels add
        e = obj.eud(dD, [(0, 1.0, 1.0), (0, 2.0, 1.0), (0, 1.0, 0.0625), (0, 1.0, -64.0), (0, 1.0, 64.0)])
        assert abs(e[0] - 2.0) <= 2.0 * d_e(3, 1.0) and abs(e[1] - 2.0) <= 2.0 * d_e(3, 1.0) and 1.0 < e[2] < 2.0
        assert abs(e[3] - 3.0 ** (1 / 64.0)) <= 1e-12 and abs(e[4] - 3.0 * 3.0 ** (-1 / 64.0)) <= 1e-12
        ok = T(abi.RTD_OBJ_SQ_MAX_EUD, 0, 3.0, 1.0, 1.0, 0.0)         # E = 2, y = 1, value 3, K = (6 * 2) / (3 * 2) = 2, p / x = 1
        plain = P(abi.RTD_OBJ_SQ_DEVIATION, 0, 3.0, 2.5)              # x = 0.5, -1.5, -0.5: value 2.75 * 3 / 3, c = 2
        for i in range(64):
            assert (L.rtd_objective_add_eud_term(h, o, C.byref(ok)) if i % 2 else L.rtd_objective_add_term(h, o, C.byref(plain))) == abi.RTD_OK
        assert L.rtd_objective_add_eud_term(h, o, C.byref(ok)) == abi.RTD_ERR_INVALID_ARG   # the 65th, through any door
        assert L.rtd_objective_add_term(h, o, C.byref(plain)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_eval(h, o, dD, dV, dG) == abi.RTD_OK
        vals = np.empty(65, dtype=np.float64)
        eng.to_host(vals, dV)
        g = np.empty(64, dtype=np.float32)
        eng.to_host(g, dG)
        # the plain terms exactly; the EUD terms within their bound (pow(2, 1) need not be 2 to the bit), which float32 g does not see
        assert np.all(vals[1::2] == 2.75) and np.all(np.abs(vals[2::2] - 3.0) <= 3.0 * d_value(3, 1.0, 2.0, 1.0)) and len(set(vals[2::2])) == 1
        assert abs(vals[0] - 32 * 5.75) <= 64 * 3.0 * d_value(3, 1.0, 2.0, 1.0)
        assert np.array_equal(np.flatnonzero(g), [0, 5, 63]) and list(g[[0, 5, 63]]) == [32 * (1.0 + 2.0), 32 * (-3.0 + 2.0), 32 * (-1.0 + 2.0)]
        obj.destroy()
        for p in (dD, dOut, dV, dG):
            eng.device_free(p)
    finally:
        eng.close()
