"""GPU tests of the voxel-wise worst case over error scenarios (rtd_objective_eval_voxelwise, rtd_scenario_dose_extremes,
rtd_optimizer_create_voxelwise; include/rtd.h) through the C ABI, against the numpy restatement
(tests/voxelwise_reference.py). The evaluation on crafted volumes of a small grid; the optimiser on the rig of the robust tests (the
96^3 heterogeneous phantom, five scenarios).

Bounds (derived, not measured; those of tests/test_gpu_objective.py). Values: a term is a float64 sum of N non-negative numbers in
some order, so |gpu - ref| <= N * 2^-52 * ref; the objective adds T terms more. Gradient: one rounding to float32 (2^-24 relative) of
a float64 sum of at most 64 separately rounded products: 64 * 2^-52 * sum_t |c_t x_t| covers any order and both sides."""
import ctypes as C
import math

import numpy as np
import pytest

import optimizer_reference as R
import robust_reference as Q
import voxelwise_reference as V
from gpu_plan_rigs import RobustRig, same
from gpu_support import bits, hetero_scene, switches
from raytracedicom_amd import abi

pytestmark = pytest.mark.gpu

DIMS = (40, 9, 7)                        # x, y, z
NVOX = int(np.prod(DIMS))                # 2520: no multiple of 256
SMAX = abi.RTD_ROBUST_MAX_SCENARIOS
NAN_BITS = np.uint32(0x7FC00123)
SENTINEL = np.uint32(0x7FC00777)

# Union positions: voxel 5 is position 0, voxel 200 + k position 1 + k. ROI 2 is the positions 128 .. 191: one wave of block 0, so
# that every other wave skips its two terms by the ballot. The union has 982 voxels: the last block holds 214, its last wave 22.
ROIS = (np.arange(200, 800), np.concatenate([[5], np.arange(600, 1150), [NVOX - 1]]), np.arange(327, 391), np.arange(1200, 1230))
TERMS = [(R.SQ_DEVIATION, 0, 1.0, 1.0), (R.SQ_UNDERDOSE, 0, 5.0, 0.95), (R.SQ_OVERDOSE, 1, 1.0, 0.3), (R.MEAN, 1, 1e-3, 0.0),
         (R.SQ_OVERDOSE, 2, 2.0, 1.2), (R.SQ_DEVIATION, 2, 0.5, 0.7)]
TIE, EQUAL, ZEROS, EQUIDISTANT, NAN_AT = 700, 701, 702, 703, 650     # voxels of ROI 0 and ROI 1 both


def _doses(S, nan=False):
    d = (2.0 * np.random.default_rng(8).random((SMAX, NVOX))).astype(np.float32)[:S].copy()
    d[:, TIE] = 1.7                      # the maximum is held by every scenario but 0: s_hi = 1 (0 with one scenario)
    d[0, TIE] = 0.2
    d[:, EQUAL] = 1.3                    # all equal: one scenario holds both extremes, one sum
    d[:, ZEROS] = 0.0                    # -0 against +0: equal, so scenario 0, with its sign
    d[0, ZEROS] = -0.0
    d[:, EQUIDISTANT] = 1.0              # 0.5 and 1.5 around the SQ_DEVIATION level 1.0: |hi - level| >= |lo - level| takes hi
    d[0, EQUIDISTANT] = 0.5
    d[min(1, S - 1), EQUIDISTANT] = 1.5 if S > 1 else 0.5
    if nan:
        d[min(2, S - 1), NAN_AT] = NAN_BITS.view(np.float32)
    return d


class Case:
    def __init__(self, engine):
        self.eng = engine.Engine(0)
        self.obj, self.ref = self.eng.create_objective(DIMS), R.ReferenceObjective(NVOX)
        for k, idx in enumerate(ROIS):
            assert self.obj.add_roi(idx.astype(np.int32)) == k == self.ref.add_roi(idx)
        for t in TERMS:
            self.obj.add_term(*t)
            self.ref.add_term(*t)
        self.dD = [self.eng.device_alloc(4 * NVOX) for _ in range(SMAX)]
        self.dG = [self.eng.device_alloc(4 * NVOX) for _ in range(SMAX)]
        self.dV, self.dA = self.eng.device_alloc(8 * (1 + abi.RTD_OBJ_MAX_TERMS)), self.eng.device_alloc(4)
        self.dLo, self.dHi = self.eng.device_alloc(4 * NVOX), self.eng.device_alloc(4 * NVOX)

    def load(self, d):
        for s in range(d.shape[0]):
            self.eng.to_device(self.dD[s], d[s])
            self.eng.to_device(self.dG[s], np.full(NVOX, SENTINEL, dtype=np.uint32))

    def fetch(self, ptr, dtype=np.float32, n=NVOX):
        out = np.empty(n, dtype=dtype)
        self.eng.to_host(out, ptr)
        return out

    def eval(self, d):
        S = d.shape[0]
        self.load(d)
        values, active = self.obj.eval_voxelwise(self.dD[:S], self.dG[:S])
        return values, active, np.stack([self.fetch(self.dG[s]) for s in range(S)])

    def close(self):
        for p in self.dD + self.dG + [self.dV, self.dA, self.dLo, self.dHi]:
            self.eng.device_free(p)
        self.obj.destroy()
        self.eng.close()


@pytest.fixture(scope="module")
def case(engine):
    c = Case(engine)
    yield c
    c.close()


@pytest.mark.parametrize("S", [1, 2, 5, 32])
def test_eval_voxelwise_against_the_restatement(case, S):
    d = _doses(S)
    values, active, g = case.eval(d)
    rv, G, ractive, Gabs = V.eval_voxelwise(case.ref, d)
    union = case.ref.union()
    assert union.sum() == 982 and np.all(bits(g)[:, ~union] == SENTINEL)              # nothing is written outside the union
    assert not np.any(bits(g)[:, union] == SENTINEL)                                  # and all S volumes at every voxel of it
    g32 = G.astype(np.float32)
    assert np.array_equal(g[:, union] != 0, g32[:, union] != 0) and not g32[:, ~union].any()
    assert np.all(bits(g)[:, union][g[:, union] == 0] == 0)                           # what is not received is +0
    assert active == ractive and active == sum(1 << s for s in range(S) if np.any(g[s][union] != 0))
    lo, s_lo, hi, s_hi = V.extremes(d)
    if S > 1:
        assert (s_hi[TIE], s_lo[TIE]) == (1, 0) and g[1][TIE] != 0 and g[0][TIE] != 0 and not g[2:, TIE].any()
        assert (s_hi[EQUAL], s_lo[EQUAL]) == (0, 0) and g[0][EQUAL] != 0 and not g[1:, EQUAL].any()
        assert (s_hi[ZEROS], s_lo[ZEROS]) == (0, 0) and g[0][ZEROS] != 0 and not g[1:, ZEROS].any()
        # equidistant: SQ_DEVIATION takes hi (scenario 1); SQ_UNDERDOSE at 0.95 sees lo = 0.5 (scenario 0)
        c_dev, c_under, c_over, wn = 2.0 * 1.0 / 600, 2.0 * 5.0 / 600, 2.0 * 1.0 / 552, 1e-3 / 552
        assert g[1][EQUIDISTANT] == np.float32(((0.0 + c_dev * (1.5 - 1.0)) + c_over * (1.5 - 0.3)) + wn)
        assert g[0][EQUIDISTANT] == np.float32(0.0 + c_under * (0.5 - 0.95))
    sizes = [int(case.ref.rois[roi].size) for _, roi, _, _ in TERMS]
    for t, n in enumerate(sizes):
        rel = abs(values[1 + t] - rv[1 + t]) / rv[1 + t]
        print("S %d, term %d: N %d, gpu %.17g ref %.17g, relative difference %.3g of the bound %.3g" % (S, t, n, values[1 + t], rv[1 + t], rel, n * 2.0 ** -52))
        assert rv[1 + t] > 0 and rel <= n * 2.0 ** -52, t
    relF = abs(values[0] - rv[0]) / rv[0]
    print("S %d: F gpu %.17g ref %.17g, relative difference %.3g of the bound %.3g" % (S, values[0], rv[0], relF, (max(sizes) + len(TERMS)) * 2.0 ** -52))
    assert relF <= (max(sizes) + len(TERMS)) * 2.0 ** -52
    nz = g32 != 0
    err = np.abs(g[nz].astype(np.float64) - G[nz])
    bound = 2.0 ** -24 * np.abs(G[nz]) + 64 * 2.0 ** -52 * Gabs[nz]
    print("S %d: gradient: worst |gpu - ref| / bound = %.3g over %d entries, active mask 0x%x" % (S, float(np.max(err / bound)), int(nz.sum()), active))
    assert np.all(err <= bound) and nz.sum() >= union.sum() - ROIS[3].size
    if S == 1:                                                                         # one scenario: rtd_objective_eval to the bit
        case.eng.to_device(case.dG[1], np.full(NVOX, SENTINEL, dtype=np.uint32))
        plain = case.obj.eval(case.dD[0], case.dG[1])
        assert np.array_equal(bits(plain), bits(values)) and np.array_equal(bits(case.fetch(case.dG[1])), bits(g[0]))
    else:                                                                              # the composite is at least every scenario's own value
        fs = np.array([case.ref.eval(d[s])[0][0] for s in range(S)])
        assert np.all(values[0] >= fs * (1.0 - 600 * 2.0 ** -52))


@pytest.mark.parametrize("S", [1, 5, 32])
def test_eval_voxelwise_with_a_nan(case, S):
    d = _doses(S, nan=True)
    values, active, g = case.eval(d)
    rv, G, ractive, _ = V.eval_voxelwise(case.ref, d)
    s = min(2, S - 1)
    assert math.isnan(values[0]) and math.isnan(rv[0]) and (active >> s) & 1 and active == ractive
    assert math.isnan(g[s][NAN_AT]) and not np.delete(g[:, NAN_AT], s).any()
    assert np.array_equal(np.isnan(values), np.isnan(rv)) and np.isnan(values[1:]).sum() == 4    # the four terms of ROI 0 and ROI 1
    union = case.ref.union()
    assert np.array_equal(g[:, union] != 0, G.astype(np.float32)[:, union] != 0) and np.all(bits(g)[:, ~union] == SENTINEL)


@pytest.mark.parametrize("S", [1, 2, 5, 32])
def test_dose_extremes(case, S):
    for nan in (False, True):
        d = _doses(S, nan=nan)
        case.load(d)
        for p in (case.dLo, case.dHi):
            case.eng.to_device(p, np.full(NVOX, SENTINEL, dtype=np.uint32))
        case.eng.dose_extremes(case.dD[:S], NVOX, case.dLo, case.dHi)
        lo, s_lo, hi, s_hi = V.extremes(d)
        assert np.array_equal(bits(case.fetch(case.dLo)), bits(lo)) and np.array_equal(bits(case.fetch(case.dHi)), bits(hi))
        if nan:
            assert bits(lo)[NAN_AT] == NAN_BITS and bits(hi)[NAN_AT] == NAN_BITS
        assert np.signbit(lo[ZEROS]) and np.signbit(hi[ZEROS])
    # either output may be NULL; a shorter range leaves the rest alone
    for p in (case.dLo, case.dHi):
        case.eng.to_device(p, np.full(NVOX, SENTINEL, dtype=np.uint32))
    case.eng.dose_extremes(case.dD[:S], 300, None, case.dHi)
    case.eng.dose_extremes(case.dD[:S], 257, case.dLo, None)
    got_lo, got_hi = case.fetch(case.dLo), case.fetch(case.dHi)
    assert np.array_equal(bits(got_hi)[:300], bits(hi)[:300]) and np.all(bits(got_hi)[300:] == SENTINEL)
    assert np.array_equal(bits(got_lo)[:257], bits(lo)[:257]) and np.all(bits(got_lo)[257:] == SENTINEL)


def test_eval_and_extremes_capture(case):
    """rtd_objective_eval_voxelwise and rtd_scenario_dose_extremes captured into a graph on a caller's stream and replayed once give
    the bits of the direct calls."""
    import torch
    S = 5
    d = _doses(S)
    values, active, g = case.eval(d)
    case.eng.dose_extremes(case.dD[:S], NVOX, case.dLo, case.dHi)
    lo, hi = case.fetch(case.dLo), case.fetch(case.dHi)
    case.load(d)
    for p in (case.dLo, case.dHi):
        case.eng.device_zero(p, 4 * NVOX)
    case.eng.device_zero(case.dV, 8 * (1 + len(TERMS)))
    case.eng.to_device(case.dA, np.full(1, 0xFFFFFFFF, dtype=np.uint32))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    case.eng.sync()
    case.eng.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                case.obj.eval_voxelwise(case.dD[:S], case.dG[:S], dev_values=case.dV, dev_active=case.dA)
                case.eng.dose_extremes(case.dD[:S], NVOX, case.dLo, case.dHi)
            graph.replay()
        torch.cuda.synchronize()
    finally:
        case.eng.set_stream(None)
    assert np.array_equal(bits(case.fetch(case.dV, np.float64, 1 + len(TERMS))), bits(values))
    assert int(case.fetch(case.dA, np.uint32, 1)[0]) == active
    assert np.array_equal(bits(np.stack([case.fetch(case.dG[k]) for k in range(S)])), bits(g))
    assert np.array_equal(bits(case.fetch(case.dLo)), bits(lo)) and np.array_equal(bits(case.fetch(case.dHi)), bits(hi))


# ---- the optimiser ----

def _vox(rig, start=None, scen=None, obj=None, no_batch=False):
    sf = rig.sfields if scen is None else [rig.sfields[s] for s in scen]
    with switches(**({"RTD_ROBUST_NO_BATCH": "1"} if no_batch else {})):
        o = rig.eng.create_voxelwise_optimizer(sf, rig.obj if obj is None else obj)
    rig.opts.append(o)
    if start is not None:
        rig.set_weights(o, start)
    return o


def _retire(rig):
    """Destroys the optimisers a test made on a shared rig."""
    for o in rig.opts:
        o.destroy()
    rig.opts = []


@pytest.fixture(scope="module")
def rig2(engine, synth):
    """Two crossing fields, five scenarios."""
    r = RobustRig(engine, hetero_scene(synth, 96, (0.0, 90.0)))
    yield r
    r.close()


@pytest.fixture(scope="module")
def rig1(engine, synth):
    """One field, five scenarios."""
    r = RobustRig(engine, hetero_scene(synth, 96, (0.0,)))
    yield r
    r.close()


def test_one_scenario_is_the_plain_optimiser(rig2):
    """S = 1: after 10 iterations history, w, w_best and the report are those of rtd_optimizer_create, bit for bit."""
    rig = rig2
    try:
        plain = rig.eng.create_optimizer(rig.fields, rig.obj, None)
        rig.opts.append(plain)
        one = _vox(rig, scen=[0])
        plain.run(10)
        one.run(10)
        rep, hist = same(rig, plain, one)
        assert rep["iterations"] == 10 and hist.size == 10 and np.all(np.isfinite(hist)) and hist.min() < hist[0]
        assert np.array_equal(bits(rig.volume(plain.dose())), bits(rig.volume(one.dose())))
        v, l, worst = one.scenario_values()
        assert v.size == 1 and v[0] == rep["f_last"] and l[0] == 1.0 and worst == 0 and one.scenario_dose(0) == one.dose()
    finally:
        _retire(rig)


def test_the_iteration_against_the_restatement(rig2):
    """Two crossing fields, five scenarios, iterations 0, 1 and 2. Every scenario volume is "zero, then apply(init = 0) per field".
    rtd_objective_eval_voxelwise on the optimiser's volumes into the test's own g volumes gives F, the active word and g_s, which are
    the restatement's on the same float32 volumes (F within the summation bound, the word and the zero pattern of g_s exactly); F,
    lambda and the worst scenario of the record are those bit for bit; the combined gradient of apply_t on those g_s (through the
    weights it produces), the step length (summed in the device's order) and the updated weights match bit for bit."""
    rig = rig2
    try:
        opt = _vox(rig)
        S = rig.S
        dDose, dGrad = rig.alloc(4 * rig.nvox), rig.alloc(4 * max(rig.sizes))
        dG = [rig.alloc(4 * rig.nvox) for _ in range(S)]
        w_prev = grad_prev = None
        for k in range(3):
            ws, w = rig.weights(opt), rig.all_weights(opt)
            opt.run(1)
            rep, hist = opt.result()
            vals, lam, worst = opt.scenario_values()
            ptrs = [opt.scenario_dose(s) for s in range(S)]
            d = np.stack([rig.volume(p) for p in ptrs])
            for s in range(S):
                rig.scenario_dose_of(s, ws, dDose)
                assert d[s].max() > 0 and np.array_equal(bits(d[s]), bits(rig.volume(dDose))), (k, s)
            values, active = rig.obj.eval_voxelwise(ptrs, dG)
            g = np.stack([rig.volume(p) for p in dG])
            rv, G, ractive, _ = V.eval_voxelwise(rig.ref, d)
            assert active == ractive and np.array_equal(g != 0, G.astype(np.float32) != 0)
            assert abs(values[0] - rv[0]) <= (rig.nvox + 4) * 2.0 ** -52 * rv[0]
            f_ref, lam_ref, worst_ref = V.decide(values[0], active, S)
            assert np.array_equal(bits(f_ref), bits(vals)) and np.array_equal(bits(lam_ref), bits(lam)) and worst_ref == worst
            assert bits(np.array([values[0]]))[0] == bits(hist[k:k + 1])[0] and hist[k] == rep["f_last"] and rep["guarded"] == 0
            grads = []
            for s in range(S):
                out = []
                for f, n in zip(rig.sfields[s], rig.sizes):
                    f.dose_influence_apply_t(dG[s], dGrad)
                    part = np.empty(n, dtype=np.float32)
                    rig.eng.to_host(part, dGrad)
                    out.append(part)
                grads.append(np.concatenate(out))
            grad = V.combine(grads, lam_ref, rig.n)
            a_ref = Q.step_length_tree(w, w_prev, grad, grad_prev, k > 0)
            print("iteration %d: F %.9g (restated %.9g), active 0x%x, lambda %s, worst %d, alpha %.17g on the device, %.17g restated"
                  % (k, hist[k], rv[0], active, lam, worst, rep["step"], a_ref))
            assert bin(active).count("1") >= 2                             # more than one scenario supplies an extreme somewhere
            assert a_ref > 0 and rep["step"] == a_ref
            w_new = rig.all_weights(opt)
            assert np.array_equal(bits(w_new), bits(R.update(w, grad, rep["step"]))) and not np.array_equal(w_new, w)
            w_prev, grad_prev = w, grad
    finally:
        _retire(rig)


def test_batched_equals_unbatched(rig2):
    """The same twelve iterations with RTD_ROBUST_NO_BATCH set before creation: the same history, weights, record and scenario doses."""
    rig = rig2
    try:
        a, b = _vox(rig, start=0.0), _vox(rig, start=0.0, no_batch=True)
        a.run(12)
        b.run(12)
        rep, hist = same(rig, a, b)
        assert rep["iterations"] == 12 and np.all(np.isfinite(hist)) and rep["f_best"] < hist[0]
        va, vb = a.scenario_values(), b.scenario_values()
        assert np.array_equal(bits(va[0]), bits(vb[0])) and np.array_equal(bits(va[1]), bits(vb[1])) and va[2] == vb[2]
        for s in range(rig.S):
            assert np.array_equal(bits(rig.volume(a.scenario_dose(s))), bits(rig.volume(b.scenario_dose(s))))
    finally:
        _retire(rig)


def test_reproducible_and_capturable(engine, synth, rig1):
    """run(30) = run(10) three times; a second engine gives the same history; run(5) captured into a graph on a caller's stream and
    replayed once gives the bits of the direct call."""
    import torch
    rig = rig1
    other = None
    try:
        a, b = _vox(rig, start=0.0), _vox(rig, start=0.0)
        a.run(30)
        for _ in range(3):
            b.run(10)
            b.run(0)
        ra, ha = same(rig, a, b)
        assert ha.size == 30
        other = RobustRig(engine, hetero_scene(synth, 96, (0.0,)))
        c = _vox(other, start=0.0)
        c.run(30)
        rc, hc = c.result()
        assert rc == ra and np.array_equal(bits(hc), bits(ha))
        direct, captured = _vox(rig, start=0.0), _vox(rig, start=0.0)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        rig.eng.sync()
        rig.eng.set_stream(s.cuda_stream)
        try:
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
        finally:
            rig.eng.set_stream(None)
        assert rd == rg and hd.size == 5 and np.array_equal(bits(hd), bits(hg)) and np.array_equal(bits(hd), bits(ha[:5]))
        assert np.array_equal(bits(rig.weights(direct)[0]), bits(rig.weights(captured)[0]))
    finally:
        _retire(rig)
        if other is not None:
            other.close()


def test_guard(engine, synth):
    """Weights of +inf give an F that is not finite: the guard is taken, the next iterate is w_best and reproduces F_best bit for bit."""
    rig = RobustRig(engine, hetero_scene(synth, 64, (0.0,), spots=3, layers=1))
    try:
        opt = _vox(rig)
        opt.run(5)
        r5, h5 = opt.result()
        assert r5["guarded"] == 0 and np.all(np.isfinite(h5)) and r5["f_best"] == h5.min()
        best5 = rig.weights(opt, best=True)[0]
        rig.set_weights(opt, math.inf)
        opt.run(2)
        r7, h7 = opt.result()
        assert not math.isfinite(h7[5]) and r7["guarded"] == 1 and h7[6] == r7["f_best"] == r5["f_best"] and math.isfinite(r7["step"])
        assert np.array_equal(bits(rig.weights(opt, best=True)[0]), bits(best5))
        vals, lam, worst = opt.scenario_values()
        assert np.all(vals == h7[6]) and lam[worst] == 1.0
        opt.run(3)
        r10, h10 = opt.result()
        assert np.all(np.isfinite(h10[6:])) and r10["f_best"] == np.where(np.isfinite(h10), h10, np.inf).min()
        for best in (False, True):
            w = rig.weights(opt, best=best)[0]
            assert np.all(np.isfinite(w)) and np.all(w >= 0)
    finally:
        rig.close()


ITERATIONS = 40
TARGET_HALF_WIDTH_MM = 8.0


def test_the_point_of_it(rig1):
    """The rig and margin_objective(8.0) of tests/test_gpu_robust.py::test_the_point_of_it, ITERATIONS iterations from w = 0 of the
    plain optimiser on scenario 0 and of the voxel-wise one. The composite objective (rtd_objective_eval_voxelwise on the five
    scenario volumes built with apply) at the voxel-wise plan's w_best over that at the nominal plan's w_best must be below 1 and at
    most twice the ratio of the same two runs in the numpy restatement with float64 products of the matrices copied from the device
    (the margin of test_gpu_robust's test and of section 13's convergence test, for their reason: Barzilai-Borwein histories are not
    monotone, and float32 products may send one along another path). The restatement's own ratio must be below 1."""
    rig = rig1
    try:
        zeros = np.zeros(rig.n)
        obj, ref = rig.margin_objective(TARGET_HALF_WIDTH_MM)
        plain = rig.eng.create_optimizer(rig.fields, obj, None)
        rig.opts.append(plain)
        rig.set_weights(plain, 0.0)
        vox = _vox(rig, start=0.0, obj=obj)
        for o in (plain, vox):
            o.run(ITERATIONS)
        dD = [rig.alloc(4 * rig.nvox) for _ in range(rig.S)]
        dG = [rig.alloc(4 * rig.nvox) for _ in range(rig.S)]

        def device_composite(o):
            ws = rig.weights(o, best=True)
            for s in range(rig.S):
                rig.scenario_dose_of(s, ws, dD[s])
            return obj.eval_voxelwise(dD, dG)[0][0]
        d_nom, d_vox = device_composite(plain), device_composite(vox)
        rep = vox.result()[0]
        assert d_vox == rep["f_best"] and rep["guarded"] == 0
        mv, rmv = rig.host_products()
        r_nom = R.ReferenceOptimizer(ref, mv[0], rmv[0], zeros).run(ITERATIONS)
        r_vox = V.VoxelwiseReferenceOptimizer(ref, mv, rmv, zeros).run(ITERATIONS)
        h_nom, h_vox = r_vox.composite(r_nom.w_best), r_vox.composite(r_vox.w_best)
        dev, res = d_vox / d_nom, h_vox / h_nom
        print("composite objective, nominal plan: %.9g on the device, %.9g restated" % (d_nom, h_nom))
        print("composite objective, voxel-wise plan: %.9g on the device, %.9g restated" % (d_vox, h_vox))
        print("composite objective, voxel-wise plan / nominal plan: %.4f on the device, %.4f restated" % (dev, res))
        assert res < 1.0
        assert dev < 1.0 and dev <= 2.0 * res
    finally:
        _retire(rig)


def test_refusals(engine, synth):
    L = engine.lib()
    scn = hetero_scene(synth, 64, (0.0, 90.0), spots=3, layers=1)
    rig = RobustRig(engine, scn)
    try:
        eng, h = rig.eng, rig.eng._h
        BAD, NR, OK = abi.RTD_ERR_INVALID_ARG, abi.RTD_ERR_NOT_READY, abi.RTD_OK
        o, out = rig.obj._h, C.c_void_p()
        ptrs = lambda *p: (C.c_void_p * 33)(*p)   # noqa: E731
        dD = [rig.alloc(4 * rig.nvox) for _ in range(2)]
        dG = [rig.alloc(4 * rig.nvox) for _ in range(2)]
        dV, dA, dLo = rig.alloc(8 * 65), rig.alloc(4), rig.alloc(4 * rig.nvox)
        doses, grads = ptrs(*dD), ptrs(*dG)
        # rtd_objective_eval_voxelwise
        ev = L.rtd_objective_eval_voxelwise
        assert ev(h, None, doses, 2, dV, grads, dA) == BAD
        assert ev(h, o, None, 2, dV, grads, dA) == BAD
        assert ev(h, o, doses, 2, None, grads, dA) == BAD
        assert ev(h, o, doses, 2, dV, None, dA) == BAD
        assert ev(h, o, doses, 2, dV, grads, None) == BAD
        assert ev(h, o, ptrs(dD[0], None), 2, dV, grads, dA) == BAD
        assert ev(h, o, doses, 2, dV, ptrs(None, dG[1]), dA) == BAD
        assert ev(h, o, doses, 0, dV, grads, dA) == BAD
        assert ev(h, o, ptrs(*([dD[0]] * 33)), 33, dV, ptrs(*([dG[0]] * 33)), dA) == BAD
        empty = eng.create_objective(rig.dims)
        empty.add_roi(np.arange(10))
        assert ev(h, empty._h, doses, 2, dV, grads, dA) == BAD
        dvh = rig.dvh_objective()[0]
        assert ev(h, dvh._h, doses, 2, dV, grads, dA) == BAD
        assert dvh.eval(dD[0], dG[0])[0] > 0                               # the DVH objective is what it was
        values, active = rig.obj.eval_voxelwise(dD, dG)                    # usable after the refusals: zero doses
        assert values[0] == rig.obj.eval(dD[0], dG[0])[0] and active == 1
        # rtd_scenario_dose_extremes
        ex = L.rtd_scenario_dose_extremes
        assert ex(h, None, 2, rig.nvox, dLo, dLo) == BAD
        assert ex(h, ptrs(dD[0], None), 2, rig.nvox, dLo, None) == BAD
        assert ex(h, doses, 0, rig.nvox, dLo, None) == BAD
        assert ex(h, ptrs(*([dD[0]] * 33)), 33, rig.nvox, dLo, None) == BAD
        assert ex(h, doses, 2, 0, dLo, None) == BAD
        assert ex(h, doses, 2, rig.nvox, None, None) == BAD
        assert ex(h, doses, 2, rig.nvox, dLo, None) == OK and not rig.volume(dLo).any()
        # rtd_optimizer_create_voxelwise: what rtd_optimizer_create_robust refuses, and DVH terms
        fresh = eng.create_field(scn.beams[0], rig.dims)                   # no matrix
        remote = eng.create_field(scn.beams[0], rig.dims, remote=True)
        coarse = eng.create_field(scn.beams[0], (32, 32, 32))
        coarse.dose_influence()
        other_shape = eng.create_field(hetero_scene(synth, 64, (0.0,), spots=4, layers=1).beams[0], rig.dims)
        other_shape.dose_influence()
        f = rig.sfields
        arr = lambda *fs: (C.c_void_p * 80)(*[x._h for x in fs])   # noqa: E731
        create = L.rtd_optimizer_create_voxelwise
        good = arr(*f[0], *f[1])
        assert create(h, None, 2, 2, o, None, C.byref(out)) == BAD
        assert create(h, good, 2, 2, None, None, C.byref(out)) == BAD
        assert create(h, good, 2, 2, o, None, None) == BAD
        assert create(h, good, 2, 0, o, None, C.byref(out)) == BAD
        assert create(h, good, 2, 33, o, None, C.byref(out)) == BAD
        assert create(h, good, 0, 2, o, None, C.byref(out)) == BAD
        assert create(h, good, 17, 2, o, None, C.byref(out)) == BAD
        assert create(h, arr(f[0][0], f[0][1], remote, f[1][1]), 2, 2, o, None, C.byref(out)) == BAD
        assert create(h, arr(f[0][0], f[0][1], f[1][0], f[0][1]), 2, 2, o, None, C.byref(out)) == BAD      # listed twice, across scenarios
        assert create(h, arr(f[0][0], f[0][0], f[1][0], f[1][1]), 2, 2, o, None, C.byref(out)) == BAD      # and within one
        assert create(h, arr(f[0][0], f[0][1], other_shape, f[1][1]), 2, 2, o, None, C.byref(out)) == BAD  # another spot map
        assert create(h, arr(f[0][0], f[0][1], coarse, f[1][1]), 2, 2, o, None, C.byref(out)) == BAD       # another dose grid
        assert create(h, arr(f[0][0], f[0][1], fresh, f[1][1]), 2, 2, o, None, C.byref(out)) == NR
        small = eng.create_objective((32, 32, 32))
        small.add_term(R.SQ_DEVIATION, small.add_roi(np.arange(10)), 1.0, 1.0)
        assert create(h, good, 2, 2, small._h, None, C.byref(out)) == BAD
        assert create(h, good, 2, 2, empty._h, None, C.byref(out)) == BAD
        assert create(h, good, 2, 2, dvh._h, None, C.byref(out)) == BAD
        bad = abi.default_optimizer_options()
        bad.step_min = 0.0
        assert create(h, good, 2, 2, o, C.byref(bad), C.byref(out)) == BAD
        assert not out.value
        with pytest.raises(ValueError):
            eng.create_voxelwise_optimizer([f[0], f[1][:1]], rig.obj)
        # the mode of rtd_robust_options is what it was: 2 is still no mode
        ro = abi.RtdRobustOptions()
        ro.mode, ro.n_scenarios = 2, 2
        assert L.rtd_optimizer_create_robust(h, good, 2, C.byref(ro), o, None, C.byref(out)) == BAD and not out.value
        for x in (small, empty):
            x.destroy()
        for x in (fresh, remote, coarse, other_shape):
            x.destroy()
        # everything is still usable
        opt, rob = _vox(rig), rig.robust(abi.RTD_ROBUST_WORST_CASE, obj=dvh)
        p = C.c_void_p()
        assert L.rtd_optimizer_scenario_dose(h, opt._h, 5, C.byref(p)) == BAD
        assert L.rtd_optimizer_scenario_dose(h, opt._h, 4, C.byref(p)) == OK and p.value
        v, lam, worst = opt.scenario_values()
        assert list(v) == [0.0] * 5
        for x in (opt, rob):
            x.run(3)
            rep, hist = x.result()
            assert rep["iterations"] == 3 and np.all(np.isfinite(hist))
        v, lam, worst = opt.scenario_values()
        assert np.all(v == opt.result()[1][-1]) and set(lam) <= {0.0, 1.0} and lam[worst] == 1.0 and not lam[:worst].any()
    finally:
        rig.close()
