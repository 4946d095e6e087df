"""GPU tests of the resident L-BFGS optimiser with its line search on the device (rtd_optimizer_create_lbfgs, include/rtd.h;
DESIGN.md section 27) through the C ABI, against the numpy restatement that sums in the device's order (tests/lbfgs_reference.py).
ray_weight_cutoff = 0 throughout."""
import ctypes as C
import math

import numpy as np
import pytest

import dvh_reference as D
import lbfgs_reference as LB
import optimizer_reference as R
from gpu_support import bits, hetero_scene, rig_fixture, worst_ratio
from lbfgs_rig import LbfgsRig, chunk_scene, lbfgs_options, step_and_compare
from raytracedicom_amd import abi, rbe as rbe_models

pytestmark = pytest.mark.gpu

rig_of = rig_fixture(LbfgsRig)


def _start(rig):
    return np.concatenate([np.asarray(b.spotWeights, dtype=np.float32).reshape(-1) for b in (f._beam for f in rig.fields)])


def test_step_by_step_against_the_restatement(rig_of, synth):
    """Iterations 0 .. 4 at m = 3 (no pair, then one, two, three, then the ring wraps), the restatement fed the device's own d0, d1
    and grad: bit for bit with the tree-order restatement, the inner products within (n + 2) 2^-52 sum |a| |b| of plain float64."""
    rig = rig_of(hetero_scene(synth, 96, (30.0,)))
    opt = rig.lbfgs(memory=3)
    w0 = _start(rig)
    ref = rig.restatement(w0, memory=3)
    d0 = rig.product(w0)                                              # the run starts with d0 = sum_f Dij_f w_f
    moved = 0
    for k in range(5):
        out, d0 = step_and_compare(rig, opt, ref, k, d0)
        moved += out["k"] >= 0
    assert moved >= 4 and ref.count == 3, (moved, ref.count)


def test_several_chunks(rig_of, synth):
    """n = 10 480: six chunks in two blocks of the wide reduction and of the direction kernel, a last chunk of 240 entries, the field
    boundary (5115) inside a block of the update; two crossing fields, so the dose update runs over the union of two boxes."""
    rig = rig_of(chunk_scene(synth))
    n, n0 = rig.n, rig.sizes[0]
    n_ch = LB.n_chunks(n)
    print("n = %d concatenated weights (%s), %d chunks, the last of %d entries; %d blocks of 256" % (n, rig.sizes, n_ch, n - (n_ch - 1) * 2048, -(-n // 256)))
    assert n == 10480 and n_ch == 6 and n - (n_ch - 1) * 2048 == 240 and n0 % 256 != 0
    opt = rig.lbfgs(memory=3)
    w0 = _start(rig)
    ref = rig.restatement(w0, memory=3)
    d0 = rig.product(w0)
    for k in range(3):
        out, d0 = step_and_compare(rig, opt, ref, k, d0)
        assert out["k"] >= 0
        w_new, w_old = ref.w, ref.w_prev
        assert not np.array_equal(w_new[n0 - 8:n0], w_old[n0 - 8:n0]) and not np.array_equal(w_new[n0:n0 + 8], w_old[n0:n0 + 8])
        assert not np.array_equal(w_new[-240:], w_old[-240:])
    assert rig.peek(opt)["n_chunks"] == 6


def test_dose_bookkeeping(rig_of, synth):
    """Two crossing fields (0 and 90 degrees). After every unit step the tracked dose is zero + apply(init = 0) of the current weights
    bit for bit (what field 1 added outside field 0's box must be gone); after c consecutive backtracked steps it is within
    c * 2 * 2^-24 * dose plus the product's own tree bound. The natural run takes unit steps only, so the first scale is the first rule's times a power
    of 4 found on the restatement, at which the run contains backtracked steps as well as unit steps."""
    rig = rig_of(hetero_scene(synth, 96, (0.0, 90.0)))
    n0 = np.bincount(rig.mats[0].indices, minlength=rig.nvox) > 0
    n1 = np.bincount(rig.mats[1].indices, minlength=rig.nvox) > 0
    assert (n0 & n1).any() and (n1 & ~n0).any() and (n0 & ~n1).any()
    w0 = _start(rig)
    # the natural run takes unit steps only: the first rule's scale times 4, 16, ... until the restatement's run overshoots and backtracks
    first = rig.restatement(w0).step()["delta"][-1]
    scale, marks = first, []
    for j in range(1, 24):
        ref = rig.restatement(w0, initial_step=first * 4.0 ** j)
        marks = [ref.step()["k"] for _ in range(8)]
        if any(k > 0 for k in marks) and any(k == 0 for k in marks):
            scale = first * 4.0 ** j
            break
    print("the first rule gives %.6g; restatement at initial_step %.6g: accepted trials %s" % (first, scale, marks))
    assert any(k > 0 for k in marks) and any(k == 0 for k in marks), marks
    opt = rig.lbfgs(initial_step=scale)
    kinds, consecutive = [], 0
    for k in range(8):
        opt.run(1)
        lb = opt.lbfgs_report()
        got = rig.volume(opt.dose())
        w = rig.all_weights(opt)
        want = rig.product(w)
        kinds.append(lb["last_trial"])
        if lb["last_trial"] == 0:
            consecutive = 0
            assert want.max() > 0 and np.array_equal(bits(got), bits(want)), "iteration %d: %d voxels differ after a unit step" % (k, int((got != want).sum()))
        elif lb["last_trial"] > 0:
            consecutive += 1
            bound = rig.product_bound(w, consecutive)
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            print("iteration %d: backtracked (k = %d, %d in a row): worst error / bound %.3g" % (k, lb["last_trial"], consecutive, worst_ratio(err, bound)))
            assert np.all(err <= bound), "iteration %d: %d voxels beyond the bound" % (k, int((err > bound).sum()))
            assert np.all(got[bound == 0] == 0)
    print("device: accepted trials %s" % kinds)
    assert any(k > 0 for k in kinds) and any(k == 0 for k in kinds), kinds


def test_convergence_from_zero(rig_of, synth):
    """Thirty iterations from w = 0 on the plan objective: f_best at no more than half of f_0 (the project's bar for thirty steps),
    the best-iterate bookkeeping exact, the weights feasible; after a unit step history[k + 1] is the accepted F_0 bit for bit; no
    accepted step raises the history by more than one float32 rounding of the dose can. The spectral optimiser runs beside it:
    printed and recorded, not asserted."""
    rig = rig_of(hetero_scene(synth, 96, (0.0,)))
    opt = rig.lbfgs(start=0.0)
    f_trial, trial, doses, entered = [], [], [], []
    for k in range(30):
        entered.append(rig.all_weights(opt))
        opt.run(1)
        lb = opt.lbfgs_report()
        trial.append(lb["last_trial"])
        f_trial.append(lb["trial_values"][max(lb["last_trial"], 0)])
        doses.append(rig.volume(opt.dose()) if lb["last_trial"] > 0 else None)
    entered.append(rig.all_weights(opt))
    opt.run(1)                                                        # (history[30]: the objective the thirtieth step led to)
    rep, hist = opt.result()
    lb = opt.lbfgs_report()
    spectral = rig.optimizer(start=0.0)
    spectral.run(30)
    srep, shist = spectral.result()
    print("L-BFGS:   f_0 %.6g, f_best %.6g at iteration %d (ratio %.4g); unit %d, backtracked %d (halvings %d), resets %d, stalls %d"
          % (hist[0], rep["f_best"], rep["best_iteration"], rep["f_best"] / hist[0], lb["unit_steps"], lb["backtracked_steps"], lb["halvings"],
             lb["resets"], lb["stalls"]))
    print("spectral: f_0 %.6g, f_best %.6g at iteration %d (ratio %.4g)" % (shist[0], srep["f_best"], srep["best_iteration"], srep["f_best"] / shist[0]))
    print("L-BFGS history:  ", " ".join("%.5g" % v for v in hist))
    print("spectral history:", " ".join("%.5g" % v for v in shist))
    print("accepted trials: ", trial)
    assert rep["iterations"] == 31 and hist.size == 31 and rep["f_last"] == hist[-1] and rep["guarded"] == 0
    assert rep["f_best"] == hist.min() and rep["best_iteration"] == int(np.argmin(hist))
    assert min(hist[:30]) <= 0.5 * hist[0]
    for best in (False, True):
        w = rig.weights(opt, best=best)[0]
        assert np.all(np.isfinite(w)) and np.all(w >= 0)
    for k in range(30):
        if trial[k] == 0:
            assert hist[k + 1] == f_trial[k] and hist[k + 1] <= hist[k], (k, hist[k], hist[k + 1], f_trial[k])
        elif trial[k] > 0:
            slack = LB.rounding_rise_bound(rig.ref, doses[k]) + (max(r.size for r in rig.ref.rois) + 4) * 2.0 ** -52 * hist[k]
            assert f_trial[k] <= hist[k] and hist[k + 1] <= f_trial[k] + slack, (k, hist[k], hist[k + 1], f_trial[k], slack)
        else:
            assert hist[k + 1] == hist[k], (k, trial[k])
    assert np.array_equal(bits(rig.all_weights(opt, best=True)), bits(entered[rep["best_iteration"]]))   # (the iterate that entered it)


def test_resident_means_resident(engine, rig_of, synth):
    """run(30) = run(10) three times, bit for bit; a second engine gives the same history; run(5) captured into a graph on a caller's
    stream and replayed once gives the bits of the direct call."""
    import torch
    scn = hetero_scene(synth, 96, (0.0,))
    rig = rig_of(scn)

    def same(a, b, ra=None):
        ra, ha = a.result()
        rb, hb = b.result()
        assert ra == rb and np.array_equal(bits(ha), bits(hb)), (ra, rb)
        assert a.lbfgs_report() == b.lbfgs_report()
        for best in (False, True):
            assert np.array_equal(bits(rig.weights(a, best)[0]), bits(b.weights(0, best=best)))
        return ra, ha
    a, b = rig.lbfgs(start=0.0), rig.lbfgs(start=0.0)
    a.run(30)
    for _ in range(3):
        b.run(10)
        b.run(0)
    ra, ha = same(a, b)
    assert ha.size == 30
    assert np.array_equal(bits(rig.volume(a.dose())), bits(rig.volume(b.dose())))
    other = rig_of(scn)
    c = other.lbfgs(start=0.0)
    c.run(30)
    rc, hc = c.result()
    assert rc == ra and np.array_equal(bits(hc), bits(ha)) and c.lbfgs_report() == a.lbfgs_report()
    direct, captured = rig.lbfgs(start=0.0), rig.lbfgs(start=0.0)
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
    rd, hd = same(direct, captured)
    rig.eng.set_stream(None)
    assert hd.size == 5 and np.array_equal(bits(hd), bits(ha[:5]))


def test_refusals_and_edges(engine, synth):
    L = engine.lib()
    scn = hetero_scene(synth, 64, (0.0,), spots=3, layers=1)
    rig = LbfgsRig(engine, scn)
    try:
        eng, h = rig.eng, rig.eng._h
        f = rig.fields[0]
        arr = (C.c_void_p * 1)(f._h)
        out = C.c_void_p()
        create = L.rtd_optimizer_create_lbfgs
        # DVH and EUD objectives
        target = rig.ref.rois[0]
        for add in ("dvh", "eud"):
            o = eng.create_objective(rig.dims)
            o.add_roi(target)
            o.add_term(R.SQ_DEVIATION, 0, 1.0, rig.level)
            if add == "dvh":
                o.add_dvh_term(D.MIN_DVH, 0, 5.0, 0.95 * rig.level, 0.98)
            else:
                o.add_eud_term(abi.RTD_OBJ_SQ_MAX_EUD, 0, 1.0, rig.level, 4.0)
            assert create(h, arr, 1, o._h, None, C.byref(out)) == abi.RTD_ERR_INVALID_ARG and not out.value
            assert ("DVH" if add == "dvh" else "EUD") in L.rtd_last_error(h).decode()
            o.destroy()
        # options out of range
        for k, v in (("memory", 0), ("memory", 17), ("max_halvings", 8), ("armijo_c1", 0.0), ("armijo_c1", 0.5), ("armijo_c1", math.nan),
                     ("initial_step", -1.0), ("initial_step", math.inf), ("initial_step", math.nan)):
            bad = lbfgs_options(**{k: v})
            assert create(h, arr, 1, rig.obj._h, C.byref(bad), C.byref(out)) == abi.RTD_ERR_INVALID_ARG and not out.value, (k, v)
        bad = lbfgs_options()
        bad.reserved[2] = 1
        assert create(h, arr, 1, rig.obj._h, C.byref(bad), C.byref(out)) == abi.RTD_ERR_INVALID_ARG
        assert create(h, arr, 0, rig.obj._h, None, C.byref(out)) == abi.RTD_ERR_INVALID_ARG
        assert create(h, None, 1, rig.obj._h, None, C.byref(out)) == abi.RTD_ERR_INVALID_ARG
        fresh = eng.create_field(scn.beams[0], rig.dims)              # no matrix
        assert create(h, (C.c_void_p * 1)(fresh._h), 1, rig.obj._h, None, C.byref(out)) == abi.RTD_ERR_NOT_READY
        fresh.destroy()
        # what an L-BFGS optimiser refuses, and what a spectral one refuses of the new calls
        opt = rig.lbfgs()
        spectral = rig.optimizer()
        rbe = eng.create_rbe(rig.dims, rbe_models.tissue("constant", 0.1, 0.05))
        let_obj = eng.create_objective(rig.dims)
        let_obj.add_roi(target)
        let_obj.add_term(R.MEAN, 0, 1.0, 0.0)
        assert L.rtd_optimizer_set_let_objective(h, opt._h, let_obj._h) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_set_rbe(h, opt._h, rbe._h) == abi.RTD_ERR_INVALID_ARG
        v, p = (C.c_double * 1)(), C.c_void_p()
        assert L.rtd_optimizer_scenario_values(h, opt._h, v, None, None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_scenario_dose(h, opt._h, 0, C.byref(p)) == abi.RTD_ERR_INVALID_ARG
        rep, buf = abi.RtdLbfgsReport(), abi.RtdLbfgsBuffers()
        assert L.rtd_optimizer_lbfgs_report(h, spectral._h, C.byref(rep)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_lbfgs_buffers(h, spectral._h, C.byref(buf)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_lbfgs_report(h, opt._h, None) == abi.RTD_ERR_INVALID_ARG
        let_obj.destroy()
        rbe.destroy()
        r0, h0 = opt.result()
        assert r0["iterations"] == 0 and r0["best_iteration"] == -1 and r0["f_best"] == math.inf and h0.size == 0
        opt.run(4)
        r4, h4 = opt.result()
        assert r4["iterations"] == 4 and np.all(np.diff(h4) <= 0) and h4[-1] < h4[0] and opt.lbfgs_report()["pairs"] >= 1
        # a stall forced by a huge first scale: nothing moves, gamma0 shrinks, a later iteration moves
        probe = rig.lbfgs()
        probe.run(1)
        huge = 1e12 * float(rig.peek(probe)["delta"][-1])             # (10^12 times the first rule's scale)
        big = rig.lbfgs(initial_step=huge, max_halvings=2)
        w0 = rig.all_weights(big)
        big.run(1)
        lb = big.lbfgs_report()
        d_start = rig.volume(big.dose())
        assert lb["stalls"] == 1 and lb["last_trial"] == -1 and lb["last_step"] == 0.0 and lb["stall_factor"] == 2.0 ** -3 and lb["pairs"] == 0
        assert np.array_equal(bits(rig.all_weights(big)), bits(w0)) and np.array_equal(bits(d_start), bits(rig.product(w0)))
        big.run(1)
        lb = big.lbfgs_report()
        assert np.array_equal(bits(rig.volume(big.dose())), bits(d_start)) and lb["stalls"] == 2 and lb["stall_factor"] == 2.0 ** -6
        assert rig.peek(big)["delta"][-1] == huge * 2.0 ** -3
        big.run(30)
        lb, (rb, hb) = big.lbfgs_report(), big.result()
        print("after a first scale of 10^12 times the first rule's: %d stalls, then f %.6g -> %.6g" % (lb["stalls"], hb[0], rb["f_best"]))
        assert lb["unit_steps"] + lb["backtracked_steps"] >= 1 and rb["f_best"] < hb[0] and not np.array_equal(rig.all_weights(big), w0)
        # a stationary start: w = 0 under a pure overdose objective (grad >= 0 everywhere: every entry is active)
        oo = eng.create_objective(rig.dims)
        oo.add_roi(rig.ref.union())
        oo.add_term(R.SQ_OVERDOSE, 0, 1.0, 0.3 * rig.level)
        st = eng.create_lbfgs_optimizer(rig.fields, oo, None)
        rig.set_weights(st, 0.0)
        st.run(3)
        rs, hs = st.result()
        ls = st.lbfgs_report()
        assert rs["step"] == 0.0 and ls["last_step"] == 0.0 and ls["last_trial"] == -1 and ls["stalls"] == 0 and ls["resets"] == 0
        assert np.all(rig.all_weights(st) == 0) and hs[0] == hs[1] == hs[2] and rs["guarded"] == 0 and ls["pairs"] == 0
        st.destroy()
        oo.destroy()
        # start weights of +inf: the objective is not finite, nothing moves, the result says so as it does today
        inf = rig.lbfgs(start=math.inf)
        inf.run(2)
        rep = abi.RtdOptimizerReport()
        assert L.rtd_optimizer_result(h, inf._h, C.byref(rep), None, 0) == abi.RTD_ERR_INVALID_ARG
        assert rep.guarded == 2 and rep.iterations == 2 and not math.isfinite(rep.f_last) and rep.step == 0.0 and rep.f_best == math.inf
        assert "not finite" in L.rtd_last_error(h).decode()
        assert np.all(np.isinf(rig.all_weights(inf)))
        # set_weights brings it back: the dose is recomputed, the ring is empty
        rig.set_weights(inf, 50.0)
        inf.run(4)
        hbuf = (C.c_double * 8)()                                      # (the unusable start stays on the record, as in the spectral optimiser)
        assert L.rtd_optimizer_result(h, inf._h, C.byref(rep), hbuf, 8) == abi.RTD_ERR_INVALID_ARG and rep.history_len == 6
        hi = np.array(hbuf[:6])
        assert rep.guarded == 2 and math.isfinite(hi[2]) and hi[5] < hi[2] and rep.f_best == hi[2:].min()
        assert inf.lbfgs_report()["pairs"] >= 1
        # a field's matrix computed again: run refuses before its first launch
        before = (rig.all_weights(opt), opt.result()[0])
        f.dose_influence()
        assert L.rtd_optimizer_run(h, opt._h, 1) == abi.RTD_ERR_NOT_READY
        assert "computed again" in L.rtd_last_error(h).decode()
        after = (rig.all_weights(opt), opt.result()[0])
        assert np.array_equal(bits(before[0]), bits(after[0])) and before[1] == after[1]
    finally:
        rig.close()
