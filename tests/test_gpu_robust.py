"""GPU tests of the robust optimiser (rtd_optimizer_create_robust, rtd_optimizer_scenario_values, rtd_optimizer_scenario_dose;
include/rtd.h) through the C ABI, against the numpy restatement of its iteration (tests/robust_reference.py).
The 96^3 heterogeneous phantom of the optimiser tests, ray_weight_cutoff = 0, five scenarios: nominal, the patient displaced by
+-5 mm across the beam (gantry x), and the stopping-power table scaled by 0.965 and 1.035."""
import ctypes as C
import math

import numpy as np
import pytest

import optimizer_reference as R
import robust_reference as Q
from gpu_plan_rigs import MODES, RobustRig, same
from gpu_support import bits, hetero_scene, rig_fixture
from raytracedicom_amd import abi, robust, scenarios

pytestmark = pytest.mark.gpu

rrig_of = rig_fixture(RobustRig, "rrig_of")


@pytest.mark.parametrize("dvh", [False, True])
def test_one_scenario_is_the_plain_optimiser(rrig_of, synth, dvh):
    """S = 1, EXPECTED, p = [1.0]: after 10 iterations history, w, w_best and the report are those of rtd_optimizer_create, bit for
    bit; with the objective of section 12 and with the DVH objective of tests/test_gpu_dvh.py."""
    rig = rrig_of(hetero_scene(synth, 96, (0.0, 90.0)))
    obj = rig.dvh_objective()[0] if dvh else rig.obj
    plain = rig.eng.create_optimizer(rig.fields, obj, None)
    rig.opts.append(plain)
    one = rig.robust(abi.RTD_ROBUST_EXPECTED, probabilities=[1.0], scen=[0], obj=obj)
    plain.run(10)
    one.run(10)
    rep, hist = same(rig, plain, one)
    assert rep["iterations"] == 10 and hist.size == 10 and np.all(np.isfinite(hist)) and hist.min() < hist[0]
    assert np.array_equal(bits(rig.volume(plain.dose())), bits(rig.volume(one.dose())))
    v, l, worst = one.scenario_values()
    assert v.size == 1 and v[0] == rep["f_last"] and l[0] == 1.0 and worst == 0
    v, l, worst = plain.scenario_values()                              # a plain optimiser is a set of one scenario
    assert v.size == 1 and v[0] == rep["f_last"] and l[0] == 1.0 and worst == 0 and plain.scenario_dose(0) == plain.dose()


@pytest.mark.parametrize("mode", MODES)
def test_scenario_doses_and_values(rrig_of, synth, mode):
    """After run(1): scenario_dose(s) is a zeroed volume followed by apply(init = 0) per field of scenario s, bit for bit;
    scenario_values()[s] is rtd_objective_eval on that volume, bit for bit; rtd_optimizer_dose is scenario 0. Twice, so that the
    second forward product runs over what the first left."""
    rig = rrig_of(hetero_scene(synth, 96, (0.0, 90.0)))
    opt = rig.robust(mode)
    dDose, dG = rig.alloc(4 * rig.nvox), rig.alloc(4 * rig.nvox)
    for k in range(2):
        ws = rig.weights(opt)
        opt.run(1)
        vals, lam, worst = opt.scenario_values()
        assert opt.dose() == opt.scenario_dose(0) and len({opt.scenario_dose(s) for s in range(rig.S)}) == rig.S
        seen = []
        for s in range(rig.S):
            got = rig.volume(opt.scenario_dose(s))
            rig.scenario_dose_of(s, ws, dDose)
            want = rig.volume(dDose)
            assert want.max() > 0 and np.array_equal(bits(got), bits(want)), (k, s)
            assert rig.obj.eval(dDose, dG)[0] == vals[s], (k, s)
            seen.append(got)
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], seen[3]) and not np.array_equal(seen[3], seen[4])
        print("iteration %d, mode %d: scenario values %s, worst %d" % (k, mode, vals, worst))
        assert worst == int(np.argmax(vals)) and opt.result()[0]["f_last"] == Q.decide(vals, mode)[1]


@pytest.mark.parametrize("mode", MODES)
def test_the_iteration_against_the_restatement(rrig_of, synth, mode):
    """Two crossing fields, iterations 0, 1 and 2, the restatement fed the device's own per-scenario values and per-scenario gradients
    (apply_t on g_s): lambda, F and the combined gradient bit for bit (the gradient through the weights it produces), the step length
    bit for bit against the restatement that sums in the device's order, the updated weights bit for bit."""
    rig = rrig_of(hetero_scene(synth, 96, (0.0, 90.0)))
    p = [0.4, 0.15, 0.15, 0.15, 0.15] if mode == abi.RTD_ROBUST_EXPECTED else None
    opt = rig.robust(mode, probabilities=p)
    dG, dGrad = rig.alloc(4 * rig.nvox), rig.alloc(4 * max(rig.sizes))
    w_prev = grad_prev = None
    for k in range(3):
        w = rig.all_weights(opt)
        opt.run(1)
        rep, hist = opt.result()
        vals, lam, worst = opt.scenario_values()
        values, grads = [], []
        for s in range(rig.S):
            v, g = rig.scenario_grad(rig.obj, s, opt.scenario_dose(s), dG, dGrad)
            values.append(v[0])
            grads.append(g)
        assert np.array_equal(bits(np.array(values)), bits(vals))
        lam_ref, F_ref, worst_ref = Q.decide(values, mode, p)
        assert np.array_equal(bits(lam_ref), bits(lam)) and worst_ref == worst
        assert F_ref == hist[k] and hist[k] == rep["f_last"] and rep["guarded"] == 0
        grad = Q.combine(grads, lam_ref)
        a_ref = Q.step_length_tree(w, w_prev, grad, grad_prev, k > 0)
        print("iteration %d, mode %d: F %.9g, lambda %s, alpha %.17g on the device, %.17g restated" % (k, mode, hist[k], lam, rep["step"], a_ref))
        assert a_ref > 0 and rep["step"] == a_ref
        w_new = rig.all_weights(opt)
        assert np.array_equal(bits(w_new), bits(R.update(w, grad, rep["step"]))) and not np.array_equal(w_new, w)
        w_prev, grad_prev = w, grad


@pytest.mark.parametrize("mode", MODES)
def test_batched_equals_unbatched(rrig_of, synth, mode):
    """The same twelve iterations with RTD_ROBUST_NO_BATCH set before creation (the single-matrix launches, scenario by scenario):
    the same history, weights and scenario doses, bit for bit. With the DVH objective under WORST_CASE, the plain one under EXPECTED."""
    rig = rrig_of(hetero_scene(synth, 96, (0.0, 90.0)))
    obj = rig.dvh_objective()[0] if mode == abi.RTD_ROBUST_WORST_CASE else rig.obj
    a, b = rig.robust(mode, start=0.0, obj=obj), rig.robust(mode, start=0.0, obj=obj, no_batch=True)
    a.run(12)
    b.run(12)
    rep, hist = same(rig, a, b)
    assert rep["iterations"] == 12 and np.all(np.isfinite(hist)) and rep["f_best"] < hist[0]
    va, vb = a.scenario_values(), b.scenario_values()
    assert np.array_equal(bits(va[0]), bits(vb[0])) and np.array_equal(bits(va[1]), bits(vb[1])) and va[2] == vb[2]
    for s in range(rig.S):
        assert np.array_equal(bits(rig.volume(a.scenario_dose(s))), bits(rig.volume(b.scenario_dose(s))))


def test_reproducible_and_capturable(engine, rrig_of, synth):
    """run(30) = run(10) three times; a second engine gives the same history; run(5) captured into a graph on a caller's stream and
    replayed once gives the bits of the direct call."""
    import torch
    scn = hetero_scene(synth, 96, (0.0,))
    rig = rrig_of(scn)
    mode = abi.RTD_ROBUST_WORST_CASE
    a, b = rig.robust(mode, start=0.0), rig.robust(mode, start=0.0)
    a.run(30)
    for _ in range(3):
        b.run(10)
        b.run(0)
    ra, ha = same(rig, a, b)
    assert ha.size == 30
    other = rrig_of(scn)
    c = other.robust(mode, start=0.0)
    c.run(30)
    rc, hc = c.result()
    assert rc == ra and np.array_equal(bits(hc), bits(ha))
    for m in MODES:
        direct, captured = rig.robust(m, start=0.0), rig.robust(m, start=0.0)
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
        assert rd == rg and hd.size == 5 and np.array_equal(bits(hd), bits(hg))
        if m == mode:
            assert np.array_equal(bits(hd), bits(ha[:5]))
        assert np.array_equal(bits(rig.weights(direct)[0]), bits(rig.weights(captured)[0]))


@pytest.mark.parametrize("mode", MODES)
def test_guard(rrig_of, synth, mode):
    """Weights of +inf give an F that is not finite: the guard is taken, the next iterate is w_best and reproduces F_best bit for bit."""
    rig = rrig_of(hetero_scene(synth, 64, (0.0,), spots=3, layers=1))
    opt = rig.robust(mode)
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
    assert np.all(np.isfinite(vals)) and Q.decide(vals, mode)[1] == h7[6]
    opt.run(3)
    r10, h10 = opt.result()
    assert np.all(np.isfinite(h10[6:])) and r10["f_best"] == np.where(np.isfinite(h10), h10, np.inf).min()
    for best in (False, True):
        w = rig.weights(opt, best=best)[0]
        assert np.all(np.isfinite(w)) and np.all(w >= 0)


ITERATIONS = 40
TARGET_HALF_WIDTH_MM = 8.0


def test_the_point_of_it(rrig_of, synth):
    """Three runs of ITERATIONS iterations from w = 0: the plain optimiser on scenario 0 alone, the robust one in WORST_CASE and in
    EXPECTED. For each w_best, max_s f_s and sum_s p_s f_s over the five scenarios (through apply + eval on the device). The
    WORST_CASE plan must have the lower max_s f_s than the nominal plan and the EXPECTED plan the lower expected value; each ratio
    must be below 1 and at most twice the ratio of the same three runs in the numpy restatement with float64 products of the
    matrices copied from the device (the margin of section 13's convergence test, for its reason: Barzilai-Borwein histories are not
    monotone, and float32 products may send one along another path). The restatement's own ratios must be clearly below 0.5, else
    the case shows nothing.

    The objective is the rig's (section 12) with the target cut to the voxels within TARGET_HALF_WIDTH_MM of the beam axis across the
    beam. With the rig's own target, which is as wide as the 5 x 5 spot pattern (spots at -16 .. 16 mm), no plan can be robust
    against a lateral shift: there is no spot outside the target to paint a margin with. The restatement says so by itself: with
    that target its ratios were 0.55 / 0.78 at shifts of 5 mm, and enlarging the shifts does not bring them down (0.53 / 0.72 at
    8 mm, 0.63 / 0.77 at 12 mm, 0.72 / 0.82 at 16 mm, float64 products of the CPU oracle's columns). A target of +-8 mm leaves the
    spots at +-16 mm as a margin wider than the 5 mm shift; the same restatement then gives 0.17 / 0.32."""
    rig = rrig_of(hetero_scene(synth, 96, (0.0,)))
    zeros = np.zeros(rig.n)
    obj, ref = rig.margin_objective(TARGET_HALF_WIDTH_MM)
    plain = rig.eng.create_optimizer(rig.fields, obj, None)
    rig.opts.append(plain)
    rig.set_weights(plain, 0.0)
    worst, expected = rig.robust(abi.RTD_ROBUST_WORST_CASE, start=0.0, obj=obj), rig.robust(abi.RTD_ROBUST_EXPECTED, start=0.0, obj=obj)
    for o in (plain, worst, expected):
        o.run(ITERATIONS)
    dDose, dG = rig.alloc(4 * rig.nvox), rig.alloc(4 * rig.nvox)

    def device_values(o):
        ws = rig.weights(o, best=True)
        out = []
        for s in range(rig.S):
            rig.scenario_dose_of(s, ws, dDose)
            out.append(obj.eval(dDose, dG)[0])
        return np.array(out)
    d_nom, d_worst, d_exp = device_values(plain), device_values(worst), device_values(expected)
    assert d_worst.max() == worst.result()[0]["f_best"] and Q.decide(d_exp, Q.EXPECTED)[1] == expected.result()[0]["f_best"]
    mv, rmv = rig.host_products()
    r_nom = R.ReferenceOptimizer(ref, mv[0], rmv[0], zeros).run(ITERATIONS)
    r_worst = Q.RobustReferenceOptimizer(ref, mv, rmv, zeros, Q.WORST_CASE).run(ITERATIONS)
    r_exp = Q.RobustReferenceOptimizer(ref, mv, rmv, zeros, Q.EXPECTED).run(ITERATIONS)
    h_nom, h_worst, h_exp = r_worst.evaluate(r_nom.w_best), r_worst.evaluate(r_worst.w_best), r_worst.evaluate(r_exp.w_best)
    dev = (d_worst.max() / d_nom.max(), d_exp.mean() / d_nom.mean())
    ref = (h_worst.max() / h_nom.max(), h_exp.mean() / h_nom.mean())
    print("nominal plan: f_s on the device %s, restated %s" % (d_nom, h_nom))
    print("WORST_CASE plan: f_s on the device %s, restated %s" % (d_worst, h_worst))
    print("EXPECTED plan: f_s on the device %s, restated %s" % (d_exp, h_exp))
    print("max_s f_s, WORST_CASE plan / nominal plan: %.4f on the device, %.4f restated" % (dev[0], ref[0]))
    print("mean_s f_s, EXPECTED plan / nominal plan: %.4f on the device, %.4f restated" % (dev[1], ref[1]))
    assert ref[0] < 0.5 and ref[1] < 0.5
    assert dev[0] < 1.0 and dev[0] <= 2.0 * ref[0]
    assert dev[1] < 1.0 and dev[1] <= 2.0 * ref[1]


def test_range_scaled_luts_move_the_distal_edge(engine, synth):
    """Water cube, one layer: with z the depth at which the central-axis dose falls to half its maximum behind the peak, the
    stopping-power table scaled by 1.035 moves it to z / 1.035, within one tracer step (1 mm) plus one dose voxel (2 mm)."""
    scn = scenarios.water_cube(synth, n=128, n_layers=1, spots=9, pitch=5.0)
    voxel, step = scn.spacing[2], 1.0
    start_z, origin_z = 128.0, -256.0 + 150.0                          # scenarios.make_field, scenarios.water_cube

    def distal_half(es):
        dose = np.zeros_like(scn.ct)
        with engine.Engine(0) as eng:
            eng.set_luts(es)
            eng.set_ct(scn.ct)
            eng.compute(scn.beams, dose)
        axis = dose[:, 64, 64].astype(np.float64)
        depth = start_z - (origin_z + voxel * np.arange(axis.size))    # along the beam (it travels towards -z): decreasing with the index
        k = int(np.argmax(axis))
        half = 0.5 * axis[k]
        j = k
        while axis[j] > half:                                          # behind the peak: towards index 0
            j -= 1
        t = (axis[j + 1] - half) / (axis[j + 1] - axis[j])
        return depth[j + 1] + t * (depth[j] - depth[j + 1])
    z0, z1 = distal_half(synth), distal_half(robust.range_scaled_luts(synth, 1.035))
    print("distal half-maximum depth %.3f mm, with the table scaled by 1.035 %.3f mm (z / 1.035 = %.3f)" % (z0, z1, z0 / 1.035))
    assert z0 > 50.0 and abs(z1 - z0 / 1.035) <= step + voxel


def test_refusals(engine, synth):
    L = engine.lib()
    scn = hetero_scene(synth, 64, (0.0, 90.0), spots=3, layers=1)
    rig = RobustRig(engine, scn)
    try:
        eng, h = rig.eng, rig.eng._h
        fresh = eng.create_field(scn.beams[0], rig.dims)              # no matrix
        remote = eng.create_field(scn.beams[0], rig.dims, remote=True)
        coarse = eng.create_field(scn.beams[0], (32, 32, 32))
        coarse.dose_influence()
        other_shape = eng.create_field(hetero_scene(synth, 64, (0.0,), spots=4, layers=1).beams[0], rig.dims)
        other_shape.dose_influence()
        f = rig.sfields
        arr = lambda *fs: (C.c_void_p * 80)(*[x._h for x in fs])   # noqa: E731
        o, out = rig.obj._h, C.c_void_p()
        P = C.POINTER(C.c_double)

        def ro(mode=0, n=2, probs=None):
            r = abi.RtdRobustOptions()
            r.mode, r.n_scenarios = mode, n
            if probs is not None:
                r._keep = np.array(probs, dtype=np.float64)
                r.probabilities = r._keep.ctypes.data_as(P)
            return r
        create = L.rtd_optimizer_create_robust
        good = arr(*f[0], *f[1])
        BAD, NR = abi.RTD_ERR_INVALID_ARG, abi.RTD_ERR_NOT_READY
        assert create(h, None, 2, C.byref(ro()), o, None, C.byref(out)) == BAD
        assert create(h, good, 2, None, o, None, C.byref(out)) == BAD
        assert create(h, good, 2, C.byref(ro()), None, None, C.byref(out)) == BAD
        assert create(h, good, 2, C.byref(ro()), o, None, None) == BAD
        assert create(h, good, 2, C.byref(ro(mode=2)), o, None, C.byref(out)) == BAD
        assert create(h, good, 2, C.byref(ro(mode=-1)), o, None, C.byref(out)) == BAD
        assert create(h, good, 2, C.byref(ro(n=0)), o, None, C.byref(out)) == BAD
        assert create(h, good, 2, C.byref(ro(n=33)), o, None, C.byref(out)) == BAD
        assert create(h, good, 0, C.byref(ro()), o, None, C.byref(out)) == BAD
        assert create(h, good, 17, C.byref(ro()), o, None, C.byref(out)) == BAD
        for probs in ([0.5, 0.0], [0.5, -0.5], [math.inf, 0.5], [0.5, math.nan]):
            assert create(h, good, 2, C.byref(ro(probs=probs)), o, None, C.byref(out)) == BAD, probs
            assert create(h, good, 2, C.byref(ro(mode=1, probs=probs)), o, None, C.byref(out)) == BAD, probs
        assert create(h, arr(f[0][0], f[0][1], remote, f[1][1]), 2, C.byref(ro()), o, None, C.byref(out)) == BAD
        assert create(h, arr(f[0][0], f[0][1], f[1][0], f[0][1]), 2, C.byref(ro()), o, None, C.byref(out)) == BAD      # listed twice, across scenarios
        assert create(h, arr(f[0][0], f[0][0], f[1][0], f[1][1]), 2, C.byref(ro()), o, None, C.byref(out)) == BAD      # and within one
        assert create(h, arr(f[0][0], f[0][1], other_shape, f[1][1]), 2, C.byref(ro()), o, None, C.byref(out)) == BAD  # another spot map
        assert create(h, arr(f[0][0], f[0][1], coarse, f[1][1]), 2, C.byref(ro()), o, None, C.byref(out)) == BAD       # another dose grid
        assert create(h, arr(f[0][0], f[0][1], fresh, f[1][1]), 2, C.byref(ro()), o, None, C.byref(out)) == NR
        small = eng.create_objective((32, 32, 32))
        small.add_term(R.SQ_DEVIATION, small.add_roi(np.arange(10)), 1.0, 1.0)
        assert create(h, good, 2, C.byref(ro()), small._h, None, C.byref(out)) == BAD
        empty = eng.create_objective(rig.dims)
        empty.add_roi(np.arange(10))
        assert create(h, good, 2, C.byref(ro()), empty._h, None, C.byref(out)) == BAD
        bad = abi.default_optimizer_options()
        bad.step_min = 0.0
        assert create(h, good, 2, C.byref(ro()), o, C.byref(bad), C.byref(out)) == BAD
        assert not out.value
        with pytest.raises(ValueError):
            eng.create_robust_optimizer([f[0], f[1][:1]], rig.obj, abi.RTD_ROBUST_EXPECTED)
        with pytest.raises(ValueError):
            eng.create_robust_optimizer([f[0], f[1]], rig.obj, abi.RTD_ROBUST_EXPECTED, probabilities=[1.0])
        for x in (small, empty):
            x.destroy()
        for x in (fresh, remote, coarse, other_shape):
            x.destroy()
        # everything is still usable: 32 scenarios cannot be made of 10 fields without listing one twice, five can
        opt = rig.robust(abi.RTD_ROBUST_WORST_CASE)
        vals, p = (C.c_double * 32)(), C.c_void_p()
        assert L.rtd_optimizer_scenario_values(h, None, vals, None, None) == BAD
        assert L.rtd_optimizer_scenario_values(h, opt._h, None, None, None) == BAD
        assert L.rtd_optimizer_scenario_values(h, opt._h, vals, None, None) == abi.RTD_OK and list(vals)[:5] == [0.0] * 5
        assert L.rtd_optimizer_scenario_dose(h, None, 0, C.byref(p)) == BAD
        assert L.rtd_optimizer_scenario_dose(h, opt._h, 0, None) == BAD
        assert L.rtd_optimizer_scenario_dose(h, opt._h, 5, C.byref(p)) == BAD
        assert L.rtd_optimizer_scenario_dose(h, opt._h, 4, C.byref(p)) == abi.RTD_OK and p.value
        plain = rig.optimizer()
        assert L.rtd_optimizer_scenario_dose(h, plain._h, 1, C.byref(p)) == BAD
        dW = rig.alloc(4 * rig.sizes[0])
        assert L.rtd_optimizer_set_weights(h, opt._h, 2, dW) == BAD and L.rtd_optimizer_weights(h, opt._h, 2, dW, 0) == BAD
        for x in (opt, plain):
            x.run(3)
            rep, hist = x.result()
            assert rep["iterations"] == 3 and np.all(np.isfinite(hist))
        v, lam, worst = opt.scenario_values()
        rep, hist = opt.result()
        assert v[worst] == v.max() == hist[-1] and list(lam) == [1.0 if s == worst else 0.0 for s in range(5)]
    finally:
        rig.close()
