"""GPU tests of the resident spot-weight optimiser (rtd_optimizer_*, include/rtd.h) through the C ABI, against the numpy restatement
of its iteration (tests/optimizer_reference.py). Scenarios as the dose-influence tests build them; ray_weight_cutoff = 0 throughout."""
import ctypes as C
import math

import numpy as np
import pytest

import optimizer_reference as R
from gpu_plan_rigs import OptimizerRig
from gpu_support import bits, hetero_scene, rig_fixture
from raytracedicom_amd import abi

pytestmark = pytest.mark.gpu

rig_of = rig_fixture(OptimizerRig)


def test_one_iteration_against_the_restatement(rig_of, synth):
    """Iterations 0, 1 and 2 (the first rule, then Barzilai-Borwein twice), the restatement fed the device's own dose and gradient:
    f within the summation bound of the objective, alpha within (n + 2) * 2^-52 relative (two float64 dot products of n entries and
    a quotient), the new weights equal to P(w - float32(alpha) * grad) bit for bit at the device's alpha."""
    rig = rig_of(hetero_scene(synth, 96, (30.0,)))
    f, n = rig.fields[0], rig.sizes[0]
    opt = rig.optimizer()
    dG, dGrad = rig.alloc(4 * rig.nvox), rig.alloc(4 * n)
    w_prev = grad_prev = None
    nmax = max(r.size for r in rig.ref.rois)
    f_best = math.inf
    for k in range(3):
        w = rig.weights(opt)[0].reshape(-1)
        opt.run(1)
        rep, hist = opt.result()
        dose = rig.volume(opt.dose())
        vals = rig.obj.eval(opt.dose(), dG)                           # the device's own g and grad, once more (same bits: deterministic)
        f.dose_influence_apply_t(dG, dGrad)
        grad = np.empty(n, dtype=np.float32)
        rig.eng.to_host(grad, dGrad)
        assert rep["iterations"] == k + 1 and hist.size == k + 1 and hist[k] == rep["f_last"] == vals[0]
        f_ref = rig.ref.eval(dose)[0][0]
        assert abs(hist[k] - f_ref) <= (nmax + 4) * 2.0 ** -52 * f_ref
        f_best = min(f_best, hist[k])
        assert rep["f_best"] == f_best and hist[rep["best_iteration"]] == f_best and rep["guarded"] == 0
        a_ref = R.step_length(w, w_prev, grad, grad_prev, k > 0)
        rel = abs(rep["step"] - a_ref) / a_ref
        print("iteration %d: f %.9g, alpha %.17g on the device, %.17g restated: relative difference %.3g of the bound %.3g"
              % (k, hist[k], rep["step"], a_ref, rel, (n + 2) * 2.0 ** -52))
        assert a_ref > 0 and rel <= (n + 2) * 2.0 ** -52
        w_new = rig.weights(opt)[0].reshape(-1)
        assert np.array_equal(bits(w_new), bits(R.update(w, grad, rep["step"])))
        assert not np.array_equal(w_new, w)
        w_prev, grad_prev = w, grad


def test_dose_is_the_sum_of_the_fields_every_iteration(rig_of, synth):
    """Two overlapping fields (0 and 90 degrees): after each of three iterations the optimiser's volume equals, bit for bit, a zeroed
    volume followed by apply(init = 0) of the fields in list order at the weights that entered the iteration (what field 1 added
    outside field 0's box an iteration earlier must be gone)."""
    rig = rig_of(hetero_scene(synth, 96, (0.0, 90.0)))
    n0 = np.bincount(rig.mats[0].indices, minlength=rig.nvox) > 0
    n1 = np.bincount(rig.mats[1].indices, minlength=rig.nvox) > 0
    assert (n0 & n1).any() and (n1 & ~n0).any() and (n0 & ~n1).any()
    opt = rig.optimizer()
    dDose = rig.alloc(4 * rig.nvox)
    seen = []
    for k in range(3):
        ws = rig.weights(opt)
        opt.run(1)
        got = rig.volume(opt.dose())
        rig.dose_of(ws, dDose)
        want = rig.volume(dDose)
        assert want.max() > 0 and np.array_equal(bits(got), bits(want)), k
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


def test_convergence_from_zero(rig_of, synth):
    """Thirty iterations from w = 0 on the plan objective: f_best at no more than half of f_0 (the project's bar for thirty steps of
    this loop), the best-iterate bookkeeping exact, the weights feasible, and w_best reproducing f_best bit for bit through apply +
    eval. The restatement with float64 products runs beside it: printed, not bounded (Barzilai-Borwein amplifies last-bit differences)."""
    rig = rig_of(hetero_scene(synth, 96, (0.0,)))
    opt = rig.optimizer(start=0.0)
    opt.run(30)
    rep, hist = opt.result()
    ref = R.ReferenceOptimizer(rig.ref, rig.matvec, rig.rmatvec, np.zeros(rig.sizes[0])).run(30)
    print("device: f_0 %.6g, f_best %.6g at iteration %d (ratio %.4g); restatement: f_best %.6g at iteration %d (ratio %.4g)"
          % (hist[0], rep["f_best"], rep["best_iteration"], rep["f_best"] / hist[0], ref.f_best, ref.best_iteration, ref.f_best / ref.history[0]))
    print("device history:", " ".join("%.4g" % v for v in hist))
    print("restated history:", " ".join("%.4g" % v for v in ref.history))
    assert rep["iterations"] == 30 and hist.size == 30 and rep["f_last"] == hist[-1]
    fin = np.where(np.isfinite(hist), hist, np.inf)
    assert rep["f_best"] == fin.min() and rep["best_iteration"] == int(np.argmin(fin))
    assert rep["f_best"] <= 0.5 * hist[0]
    for best in (False, True):
        w = rig.weights(opt, best=best)[0]
        assert np.all(np.isfinite(w)) and np.all(w >= 0)
    dDose, dG = rig.alloc(4 * rig.nvox), rig.alloc(4 * rig.nvox)
    rig.dose_of(rig.weights(opt, best=True), dDose)
    assert rig.obj.eval(dDose, dG)[0] == rep["f_best"]


def test_resident_means_resident(engine, rig_of, synth):
    """run(30) = run(10) three times, bit for bit; a second engine gives the same history; run(5) captured into a graph on a caller's
    stream and replayed once gives the bits of the direct call."""
    import torch
    scn = hetero_scene(synth, 96, (0.0,))
    rig = rig_of(scn)
    a, b = rig.optimizer(start=0.0), rig.optimizer(start=0.0)
    a.run(30)
    ra, ha = a.result()
    for _ in range(3):
        b.run(10)
        b.run(0)
    rb, hb = b.result()
    assert ra == rb and np.array_equal(bits(ha), bits(hb)) and ha.size == 30
    for best in (False, True):
        assert np.array_equal(bits(rig.weights(a, best)[0]), bits(rig.weights(b, best)[0]))
    other = rig_of(scn)
    c = other.optimizer(start=0.0)
    c.run(30)
    rc, hc = c.result()
    assert rc == ra and np.array_equal(bits(hc), bits(ha))
    # graph capture: one run(5) = 5 iterations of launches, nothing else
    direct, captured = rig.optimizer(start=0.0), rig.optimizer(start=0.0)
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


def test_errors_stationary_start_and_guard(engine, synth):
    L = engine.lib()
    scn = hetero_scene(synth, 64, (0.0,), spots=3, layers=1)
    rig = OptimizerRig(engine, scn)
    try:
        eng, h = rig.eng, rig.eng._h
        f = rig.fields[0]
        fresh = eng.create_field(scn.beams[0], rig.dims)              # no matrix
        remote = eng.create_field(scn.beams[0], rig.dims, remote=True)
        coarse = eng.create_field(scn.beams[0], (32, 32, 32))
        arr = lambda *fs: (C.c_void_p * 17)(*[x._h for x in fs])   # noqa: E731
        o, out = rig.obj._h, C.c_void_p()
        create = L.rtd_optimizer_create
        assert create(h, arr(fresh), 1, o, None, C.byref(out)) == abi.RTD_ERR_NOT_READY
        assert create(h, arr(f, fresh), 2, o, None, C.byref(out)) == abi.RTD_ERR_NOT_READY
        assert create(h, arr(remote), 1, o, None, C.byref(out)) == abi.RTD_ERR_INVALID_ARG
        assert create(h, None, 1, o, None, C.byref(out)) == abi.RTD_ERR_INVALID_ARG
        assert create(h, arr(f), 1, None, None, C.byref(out)) == abi.RTD_ERR_INVALID_ARG
        assert create(h, arr(f), 1, o, None, None) == abi.RTD_ERR_INVALID_ARG
        assert create(h, arr(f), 0, o, None, C.byref(out)) == abi.RTD_ERR_INVALID_ARG
        assert create(h, arr(*([f] * 17)), 17, o, None, C.byref(out)) == abi.RTD_ERR_INVALID_ARG
        assert create(h, arr(f, coarse), 2, o, None, C.byref(out)) == abi.RTD_ERR_INVALID_ARG      # two dose grids
        small = eng.create_objective((32, 32, 32))
        small.add_term(R.SQ_DEVIATION, small.add_roi(np.arange(10)), 1.0, 1.0)
        assert create(h, arr(f), 1, small._h, None, C.byref(out)) == abi.RTD_ERR_INVALID_ARG       # an objective on other dims
        empty = eng.create_objective(rig.dims)
        empty.add_roi(np.arange(10))
        assert create(h, arr(f), 1, empty._h, None, C.byref(out)) == abi.RTD_ERR_INVALID_ARG       # no terms
        bad = abi.default_optimizer_options()
        bad.step_min = 0.0
        assert create(h, arr(f), 1, o, C.byref(bad), C.byref(out)) == abi.RTD_ERR_INVALID_ARG
        assert not out.value
        for x in (small, empty):
            x.destroy()
        for x in (fresh, remote, coarse):
            x.destroy()
        opt = rig.optimizer()                                         # everything is still usable
        rep = abi.RtdOptimizerReport()
        p = C.c_void_p()
        dW = rig.alloc(4 * rig.sizes[0])
        assert L.rtd_optimizer_run(h, None, 1) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_set_weights(h, opt._h, 0, None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_set_weights(h, opt._h, 1, dW) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_weights(h, opt._h, 0, None, 0) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_weights(h, opt._h, 1, dW, 0) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_result(h, opt._h, None, None, 0) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_result(h, opt._h, C.byref(rep), None, 3) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_dose(h, opt._h, None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_dose(h, opt._h, C.byref(p)) == abi.RTD_OK and p.value
        r0, h0 = opt.result()
        assert r0["iterations"] == 0 and r0["best_iteration"] == -1 and r0["f_best"] == math.inf and h0.size == 0
        opt.run(5)
        r5, h5 = opt.result()
        assert r5["iterations"] == 5 and np.all(np.isfinite(h5)) and r5["f_best"] == h5.min()
        best5 = rig.weights(opt, best=True)[0]
        # weights of 1e30 (w_best is kept): whether or not float32 overflows on the way, the iteration comes back
        rig.set_weights(opt, 1e30)
        opt.run(2)
        r7, h7 = opt.result()
        print("after weights of 1e30: f %.6g then %.6g, guards taken %d" % (h7[5], h7[6], r7["guarded"]))
        assert math.isfinite(h7[6]) and not np.isnan(rig.weights(opt)[0]).any() and r7["f_best"] <= r5["f_best"]
        if r7["best_iteration"] == r5["best_iteration"]:
            assert np.array_equal(bits(rig.weights(opt, best=True)[0]), bits(best5))
        # weights of +inf: the dose and f are not finite, the guard of step 7 is taken: w = w_best, and the next f is f_best again
        rig.set_weights(opt, math.inf)
        opt.run(2)
        r9, h9 = opt.result()
        assert not math.isfinite(h9[7]) and r9["guarded"] == r7["guarded"] + 1
        assert h9[8] == r9["f_best"] and r9["f_best"] <= r5["f_best"] and math.isfinite(r9["step"])
        for best in (False, True):
            w = rig.weights(opt, best=best)[0]
            assert np.all(np.isfinite(w)) and np.all(w >= 0)
        opt.run(3)
        r12, h12 = opt.result()
        assert np.all(np.isfinite(h12[8:])) and r12["f_best"] == np.where(np.isfinite(h12), h12, np.inf).min()
        # a start that is itself not finite is reported, and the optimiser stays usable
        nf = rig.optimizer(start=math.inf)
        nf.run(1)
        st = L.rtd_optimizer_result(h, nf._h, C.byref(rep), None, 0)
        assert st == abi.RTD_ERR_INVALID_ARG and rep.iterations == 1 and rep.guarded == 1 and rep.f_best == math.inf
    finally:
        rig.close()
    # a stationary start: w = 0 under a pure overdose penalty
    rig = OptimizerRig(engine, scn, pure_overdose=True)
    try:
        opt = rig.optimizer(start=0.0)
        opt.run(1)
        r1, h1 = opt.result()
        assert r1["step"] == 0.0 and h1[0] == 0.0
        opt.run(4)
        r5, h5 = opt.result()
        w = rig.weights(opt)[0]
        assert np.all(h5 == 0.0) and np.array_equal(bits(w), bits(np.zeros_like(w))) and r5["best_iteration"] == 0 and r5["guarded"] == 0
    finally:
        rig.close()
