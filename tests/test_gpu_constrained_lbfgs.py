"""GPU tests of the constrained L-BFGS optimiser (include/rtd.h "Constrained L-BFGS: hard dose constraints behind the line search",
DESIGN.md section 32) against its numpy restatement (tests/constrained_lbfgs_reference.py) and against
rtd_objective_eval_constrained, through the C ABI.

Part one needs no field: rtd_objective_constraint_trials on a 40^3 grid at the ROI shapes at which the K-wide kernels can go wrong.
Part two runs the optimiser on the heterogeneous phantom (tests/constrained_lbfgs_rig.py).

The numbers of test_convergence as measured on the device are in its docstring."""
import ctypes as C
import math

import numpy as np
import pytest

import constraint_reference as CR
import lbfgs_terms_reference as LT
import optimizer_reference as R
from constrained_lbfgs_reference import ConstrainedLbfgsReference
from constrained_lbfgs_rig import ConstrainedLbfgsRig, check_trials, con_dict, same_floats, same_state, step_and_compare
from constraint_rig import constrained_options
from gpu_support import bits, hetero_scene, rig_fixture
from lbfgs_rig import chunk_scene, lbfgs_options
from raytracedicom_amd import abi, rbe as rbe_models

pytestmark = pytest.mark.gpu

rig_of = rig_fixture(ConstrainedLbfgsRig)

# ---- part one: the K-wide constraint kernels, no fields ---------------------------------------------------------------------------

DIMS = (40, 40, 40)
NVOX = 64000
RHO = 2.5
NC = abi.RTD_CON_MAX_CONSTRAINTS


def _rois():
    rng = np.random.default_rng(31)
    one = np.array([5])
    r63 = np.sort(rng.choice(NVOX, 63, replace=False))
    r257 = np.arange(30000, 30257)                                    # one block and one thread more
    big = np.flatnonzero(rng.random(NVOX) < 0.31)                     # about 20 000: more than 64 blocks of 256, the reducer's lane loop wraps
    box = np.arange(29900, 31200)                                     # overlaps big and r257
    bare = np.arange(63000, 63100)                                    # constrained, but without any term
    r2049 = np.arange(10000, 12049)                                   # a second chunk of one element
    return [one, r63, r257, big, box, bare, r2049]


TERMS = [(R.SQ_DEVIATION, 3, 1.0, 1.0), (R.SQ_OVERDOSE, 1, 2.0, 0.7), (R.MEAN, 2, 1e-2, 0.0), (R.SQ_UNDERDOSE, 6, 3.0, 0.9),
         (R.SQ_DEVIATION, 0, 1.0, 0.5), (R.SQ_OVERDOSE, 4, 1.5, 1.1)]
# per-voxel and mean constraints interleaved; 0 and 2 overlap voxel by voxel, 5 (a mean) overlaps both, 7 sits on the ROI without a term
CONS = [(CR.MAX_DOSE, 3, 1.0), (CR.MAX_MEAN, 6, 0.9), (CR.MIN_DOSE, 4, 0.8), (CR.MAX_DOSE, 0, 0.4), (CR.MIN_DOSE, 1, 1.3), (CR.MIN_MEAN, 4, 1.1),
        (CR.MAX_DOSE, 2, 1.7), (CR.MAX_DOSE, 5, 0.6)]


def _doses():
    """d1 per case; d0 is one finite random volume."""
    rois = _rois()
    base = (2.0 * np.random.default_rng(8).random(NVOX)).astype(np.float32)
    both = np.intersect1d(rois[3], rois[4])
    only_big = np.setdiff1d(np.setdiff1d(rois[3], rois[4]), rois[6])
    with_nan, with_inf = base.copy(), base.copy()
    with_nan[only_big[7]] = np.nan                                    # in a per-voxel constraint only
    with_inf[both[3]] = np.inf                                        # in two per-voxel constraints and a mean one
    d0 = (2.0 * np.random.default_rng(9).random(NVOX)).astype(np.float32)
    return d0, {"random": base, "nan": with_nan, "inf": with_inf}


@pytest.fixture(scope="module")
def part_one(engine):
    eng = engine.Engine(0)
    obj, ref = eng.create_objective(DIMS), R.ReferenceObjective(NVOX)
    for r in _rois():
        obj.add_roi(r)
        ref.add_roi(r)
    for t in TERMS:
        obj.add_term(*t)
        ref.add_term(*t)
    cs = CR.ConstraintSet(ref, tree=True)
    for k, c in enumerate(CONS):
        assert obj.add_constraint(*c) == k == cs.add(*c), "constraint ids count from 0"
    rng = np.random.default_rng(77)
    lam = rng.random(cs.n_entries).astype(np.float32)
    lam[rng.random(cs.n_entries) < 0.3] = 0.0
    mu = np.zeros(CR.MAX_CONSTRAINTS)
    mu[1], mu[5] = 0.25, 0.0
    bufs = {k: eng.device_alloc(n) for k, n in (("d0", 4 * NVOX), ("d1", 4 * NVOX), ("r", 4 * NVOX), ("g", 4 * NVOX), ("lam", 4 * cs.n_entries), ("mu", 8 * NC))}
    eng.to_device(bufs["lam"], lam)
    eng.to_device(bufs["mu"], mu)
    yield eng, obj, cs, lam, mu, bufs
    for p in bufs.values():
        eng.device_free(p)
    obj.destroy()
    eng.close()


@pytest.mark.parametrize("which", ["random", "nan", "inf"])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_constraint_trials_bit_for_bit(part_one, K, which):
    """psi[k][c] against con_values[1 + c] of rtd_objective_eval_constrained on the uploaded r_k and against the restatement; mean[k][c]
    against the restatement's chunk-tree mean of r_k (the evaluation has no output for the mean itself; the psi of a mean constraint,
    which is compared with the device's, is a function of it). Bit for bit, a NaN matching a NaN."""
    eng, obj, cs, lam, mu, b = part_one
    d0, d1s = _doses()
    d1 = d1s[which]
    eng.to_device(b["d0"], d0)
    eng.to_device(b["d1"], d1)
    psi, mean = obj.constraint_trials(b["d0"], b["d1"], K, b["lam"], b["mu"], RHO)
    psi2, mean2 = obj.constraint_trials(b["d0"], b["d1"], K, b["lam"], b["mu"], RHO)
    assert np.array_equal(bits(psi), bits(psi2)) and np.array_equal(bits(mean), bits(mean2)), "a second call gives other bits"
    assert psi.shape == (K, NC) and not psi[:, len(CONS):].any() and not mean[:, len(CONS):].any(), "entries past the constraints are not +0"
    for k, r in enumerate(LT.rounded_trials(d0, d1, K)):
        eng.to_device(b["r"], r)
        values, con_values = obj.eval_constrained(b["r"], b["lam"], b["mu"], RHO, b["g"])
        _, rc, _ = cs.eval(r, lam, mu, RHO)
        rm = np.array([cs.mean(c, r.astype(np.float64)) if cs.is_mean(kind) else 0.0 for c, (kind, _, _) in enumerate(CONS)])
        print("%s K %d trial %d: psi %s mean %s" % (which, K, k, psi[k, :len(CONS)], mean[k, [1, 5]]))
        assert same_floats(psi[k, :len(CONS)], con_values[1:]), "trial %d: psi %r, eval_constrained %r" % (k, psi[k, :len(CONS)], con_values[1:])
        assert same_floats(psi[k, :len(CONS)], rc[1:]), "trial %d: psi %r, restated %r" % (k, psi[k, :len(CONS)], rc[1:])
        assert same_floats(mean[k, :len(CONS)], rm), "trial %d: mean %r, restated %r" % (k, mean[k, :len(CONS)], rm)
        if which == "random":
            assert np.all(np.isfinite(psi[k])) and np.all(psi[k, :len(CONS)] != 0.0), "trial %d: a constraint acts nowhere" % k
        else:
            assert not np.all(np.isfinite(psi[k])), "trial %d: the %s did not reach a psi" % (k, which)


def test_constraint_trials_refusals(part_one):
    eng, obj, cs, lam, mu, b = part_one
    L, h, INV = eng_lib(eng), eng._h, abi.RTD_ERR_INVALID_ARG
    out = eng.device_alloc(2 * 8 * 8 * NC)
    try:
        call = L.rtd_objective_constraint_trials
        for n in (0, 9):
            assert call(h, obj._h, b["d0"], b["d1"], n, b["lam"], b["mu"], RHO, out, out + 8 * 8 * NC) == INV, "n_trials %d is accepted" % n
        for rho in (0.0, -1.0, math.inf, math.nan):
            assert call(h, obj._h, b["d0"], b["d1"], 3, b["lam"], b["mu"], rho, out, out + 8 * 8 * NC) == INV, "rho %r is accepted" % rho
        args = [b["d0"], b["d1"], 3, b["lam"], b["mu"], RHO, out, out + 8 * 8 * NC]
        for i in (0, 1, 3, 4, 6, 7):
            a = list(args)
            a[i] = None
            assert call(h, obj._h, *a) == INV, "a null pointer at %d is accepted" % i
        free = eng.create_objective(DIMS)
        free.add_roi(np.arange(10))
        free.add_term(R.SQ_DEVIATION, 0, 1.0, 1.0)
        assert call(h, free._h, *args) == INV and "no constraints" in L.rtd_last_error(h).decode(), "an objective without constraints is accepted"
        free.destroy()
        psi, _ = obj.constraint_trials(b["d0"], b["d1"], 2, b["lam"], b["mu"], RHO)
        assert psi.shape == (2, NC), "the objective is no longer usable"
    finally:
        eng.device_free(out)


def eng_lib(eng):
    from raytracedicom_amd import engine
    return engine.lib()


# ---- part two: the optimiser ------------------------------------------------------------------------------------------------------

INNER = 4
SCENES = {"one": (0.0,), "two": (0.0, 90.0)}


def overshoot_scale(make_ref, steps):
    """The first rule's scale times 4, 16, ... until the float64 restatement made by make_ref(initial_step) backtracks as well as takes a
    unit step within `steps` iterations -> the scale."""
    first = make_ref(0.0).step()["delta"][-1]
    for j in range(1, 16):
        ref = make_ref(first * 4.0 ** j)
        marks = [ref.step()["k"] for _ in range(steps)]
        if any(k > 0 for k in marks) and any(k == 0 for k in marks):
            print("first scale %.6g: the float64 restatement accepts %s" % (first * 4.0 ** j, marks))
            return first * 4.0 ** j
    raise AssertionError("no scale at which the restatement backtracks and takes a unit step")


@pytest.mark.parametrize("K", (1, 6))
@pytest.mark.parametrize("scene", list(SCENES))
def test_trial_values_in_the_optimiser(rig_of, synth, scene, K):
    """After every iteration: trial_values[k] = values[0] of rtd_objective_eval_constrained(r_k) with the optimiser's own lambda, mu and
    rho, con_trial its con_values; inside a block the next history entry is the accepted F_k. Six iterations, an outer update at 3."""
    rig = rig_of(hetero_scene(synth, 96, SCENES[scene]))
    con = constrained_options(inner_iterations=3, feasibility_tol=1e-3 * rig.level)
    opt = rig.con_lbfgs(start=60.0, con=con, max_halvings=K - 1)
    d0 = rig.product(rig.start_vector(60.0))
    accepted, chained = None, 0
    for i in range(6):
        opt.run(1)
        ln = rig.line(opt)
        hist = opt.result()[1]
        if accepted is not None and i % 3 != 0:
            assert same_floats(hist[i], accepted), "iteration %d: the history entry %r is not the accepted F_k %r" % (i, hist[i], accepted)
            chained += 1
        lb, _, _ = check_trials(rig, opt, d0, ln["d1"])
        assert lb["last_trial"] >= 0 or K == 1, "iteration %d: no trial accepted" % i
        accepted = lb["trial_values"][lb["last_trial"]] if lb["last_trial"] >= 0 else None
        d0 = rig.volume(opt.dose())
    assert chained >= 2 or K == 1, "the chain from an accepted trial to the next history entry was not seen"
    assert opt.constraint_report()[0]["outer_updates"] == 1, "no outer update ran"


def test_step_by_step_against_the_restatement(rig_of, synth):
    """2 x inner + 3 iterations with inner_iterations 4 and memory 3 on more than one weight chunk: two outer updates, the ring wraps
    and is forgotten twice. Every quantity of every iteration on the bits (constrained_lbfgs_rig.step_and_compare)."""
    rig = rig_of(chunk_scene(synth))
    con = constrained_options(inner_iterations=INNER, feasibility_tol=1e-3 * rig.level)
    n = 2 * INNER + 3
    w0 = rig.start_vector(60.0)
    _, cs64, matvec64, rmatvec64 = rig.compressed()
    kw = dict(memory=3, max_halvings=2)                               # (three trials: the restatement evaluates every one of them in numpy)
    scale = overshoot_scale(lambda step: ConstrainedLbfgsReference(cs64, matvec64, rmatvec64, w0.astype(np.float64), con_dict(con), tree=False, initial_step=step,
                                                                   **kw), INNER + 1)
    opt = rig.con_lbfgs(start=60.0, con=con, initial_step=scale, **kw)
    ref = rig.restatement(w0, con, initial_step=scale, **kw)
    d0 = rig.product(w0)
    pairs = []
    for k in range(n):
        out, d0 = step_and_compare(rig, opt, ref, k, d0, trials=False)
        pairs.append(out["pairs"])
    rep, outer = opt.constraint_report()
    lam, mu, _ = rig.multipliers(opt)
    print("pairs %s, outer %s" % (pairs, outer))
    assert [k for k, _, _ in outer] == [INNER, 2 * INNER] and rep["iterations_since_update"] == 3, (outer, rep)
    assert pairs[INNER] == 0 and pairs[2 * INNER] == 0 and max(pairs) == 3, "the ring did not wrap or was not forgotten: %s" % pairs
    assert lam.max() > 0.0 or mu.max() > 0.0, "no multiplier moved: the scene tests nothing"
    assert ref.backtracked > 0 and ref.unit > 0, "no backtracked step: the scene tests nothing"


def test_resident_means_resident(rig_of, synth):
    """run(3 inner) = run(inner) three times; run(2 inner) captured into a graph and replayed once = the direct call."""
    import torch
    rig = rig_of(hetero_scene(synth, 96, SCENES["one"]))
    con = constrained_options(inner_iterations=INNER, feasibility_tol=1e-3 * rig.level)
    a, b = rig.con_lbfgs(start=60.0, con=con), rig.con_lbfgs(start=60.0, con=con)
    a.run(3 * INNER)
    for _ in range(3):
        b.run(INNER)
        b.run(0)
    ra, ha, ca, oa = same_state(rig, a, b, "split runs")
    assert ha.size == 3 * INNER and ca["outer_updates"] == 2 and ca["iterations_since_update"] == INNER, (ha.size, ca)
    direct, captured = rig.con_lbfgs(start=60.0, con=con), rig.con_lbfgs(start=60.0, con=con)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    rig.eng.sync()
    rig.eng.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        direct.run(2 * INNER)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            captured.run(2 * INNER)
        g.replay()
    torch.cuda.synchronize()
    rd, hd, cd, od = same_state(rig, direct, captured, "graph replay")
    rig.eng.set_stream(None)
    assert hd.size == 2 * INNER and np.array_equal(bits(hd), bits(ha[:2 * INNER])) and cd["outer_updates"] == 1, (hd, cd)


def test_every_term_kind_with_constraints(rig_of, synth):
    """LbfgsTermsRig's mixed objective (plain, DVH and EUD terms) plus the three constraints: the trial values as above, and five
    iterations (an outer update at 3) against the restatement whose terms' values come from rtd_objective_eval (numpy cannot restate
    the EUD's pow to the bit)."""
    rig = rig_of(hetero_scene(synth, 64, (0.0,)))
    rig.set_mixed_constrained()
    con = constrained_options(inner_iterations=3, feasibility_tol=1e-3 * rig.level)
    w0 = rig.start_vector(60.0)
    opt = rig.con_lbfgs(start=60.0, con=con, memory=3, max_halvings=3)
    ref = rig.restatement(w0, con, terms_value_of=rig.value_of, memory=3, max_halvings=3)
    d0 = rig.product(w0)
    for k in range(5):
        out, d0 = step_and_compare(rig, opt, ref, k, d0, trials=True)
    ln = rig.line(opt)
    assert ln["coupled"] and ln["n_terms"] == 6, "the line search ran without the selections: %r" % ln["n_terms"]
    assert opt.constraint_report()[0]["outer_updates"] == 1


def test_compact(engine, synth):
    """RTD_LBFGS_COMPACT: the iteration equals the restatement driven with the compact public products (d1 and grad are
    rtd_field_dose_influence_apply_compact / _apply_t_compact of w_full and of the voxel gradient of rtd_objective_eval_constrained);
    it is created and runs after release_plain, with the bits of the run before; a matrix computed again is refused before the first
    launch."""
    L = engine.lib()
    rig = ConstrainedLbfgsRig(engine, hetero_scene(synth, 64, (0.0,)))
    try:
        h = rig.eng._h
        arr = (C.c_void_p * 1)(rig.fields[0]._h)
        out = C.c_void_p()
        create = L.rtd_optimizer_create_constrained_lbfgs
        assert create(h, arr, 1, rig.obj._h, None, None, abi.RTD_LBFGS_COMPACT, C.byref(out)) == abi.RTD_ERR_NOT_READY and not out.value, "no compact form, yet accepted"
        rig.make_compact()
        con = constrained_options(inner_iterations=3, feasibility_tol=1e-3 * rig.level)
        w0 = rig.start_vector(60.0)
        opt = rig.con_lbfgs(start=60.0, con=con, memory=3)
        ref = rig.restatement(w0, con, memory=3)
        d0 = rig.product(w0)
        for k in range(5):
            d_in = d0
            out_k, d0 = step_and_compare(rig, opt, ref, k, d0, trials=False)
            b = opt.constraint_buffers()
            rig.obj.eval_constrained(rig.upload(d_in), b.lambda_, b.mu, ref.rho, rig.dG)
            grad = rig.gradient_of(rig.volume(rig.dG))
            assert np.array_equal(bits(grad), bits(out_k["grad"])), "iteration %d: grad is not the compact product (%d entries differ)" % (k, int((grad != out_k["grad"]).sum()))
            d1 = rig.product(out_k["w_full"])
            assert np.array_equal(bits(d1), bits(out_k["d1"])), "iteration %d: d1 is not the compact product (%d voxels differ)" % (k, int((d1 != out_k["d1"]).sum()))
        h_before = opt.result()[1]
        plain = rig.con_lbfgs(start=60.0, con=con, memory=3, compact=False)
        plain.run(5)
        assert not np.array_equal(bits(plain.result()[1]), bits(h_before)), "the compact run has the plain run's history"
        rig.fields[0].dose_influence_compact(release_plain=True)
        after = rig.con_lbfgs(start=60.0, con=con, memory=3)
        after.run(5)
        assert np.array_equal(bits(after.result()[1]), bits(h_before)), "the run after release_plain differs"
        opt.run(1)
        assert opt.result()[0]["iterations"] == 6, "a compact optimiser made before the release does not run on"
        assert create(h, arr, 1, rig.obj._h, None, None, 0, C.byref(out)) == abi.RTD_ERR_NOT_READY and not out.value, "the plain form is released, yet accepted"
        assert L.rtd_optimizer_run(h, plain._h, 1) == abi.RTD_ERR_NOT_READY, "the plain optimiser runs on a released matrix"
        rig.fields[0].dose_influence()
        assert L.rtd_optimizer_run(h, after._h, 1) == abi.RTD_ERR_NOT_READY and "computed again" in L.rtd_last_error(h).decode(), "a matrix computed again is accepted"
        assert after.result()[0]["iterations"] == 5, "the refused run launched"
    finally:
        rig.close()


@pytest.mark.parametrize("scene", list(SCENES))
def test_convergence(rig_of, synth, scene):
    """200 iterations, inner_iterations 10, feasibility_tol 1e-3 x level. The float64 restatement of the UNCONSTRAINED run (plain L-BFGS)
    must violate by more than 20 x tol: the scene is a real test. The device's final w must violate by at most
    max(tol, 4 x the float64 restatement's final violation) on the same matrices, the margin of tests/test_gpu_constraints.py for a
    float32 against a float64 trajectory. No accepted step raises F inside a block, guarded == 0, weights finite and non-negative.

    Measured on the device (MI355X), violation of the final w in units of the level; DESIGN.md section 32 quotes these:
      one field   unconstrained restatement 0.4309, constrained restatement 0.0001261, device 0.0005371 (bound 0.001 = tol);
                  rho 262144, 9 increases in 19 updates; 188 unit and 12 backtracked steps, no stall
      two fields  unconstrained restatement 0.5519, constrained restatement 0.00006629, device 0.0008022 (bound 0.001 = tol);
                  rho 1e8 (the cap), 15 increases in 19 updates; 167 unit and 32 backtracked steps, 1 stall"""
    import lbfgs_reference as LB
    rig = rig_of(hetero_scene(synth, 96, SCENES[scene]))
    tol = 1e-3 * rig.level
    inner = 10
    w0 = np.full(sum(rig.sizes), 60.0)
    obj_c, cs, matvec, rmatvec = rig.compressed()                      # (the voxels with rows only: the same plan, a tenth of the volume)
    plain = LB.LbfgsReference(obj_c, matvec, rmatvec, w0, tree=False).run(200)
    v_plain = float(cs.violations(matvec(plain.w))[0].max())
    con = constrained_options(inner_iterations=inner, feasibility_tol=tol)
    ref = ConstrainedLbfgsReference(cs, matvec, rmatvec, w0, con_dict(con), tree=False).run(200)
    v_ref = float(cs.violations(matvec(ref.w))[0].max())
    o = rig.con_lbfgs(start=60.0, con=con)
    o.run(200)
    final = rig.weights(o)
    v_dev, mx, cnt = rig.violation_of(final, tol)
    rep, outer = o.constraint_report()
    r, hist = o.result()
    lb = o.lbfgs_report()
    lam, mu, rho = rig.multipliers(o)
    bound = max(tol, 4.0 * v_ref)
    print("%s: level %.6g; violation / level: unconstrained restatement %.4g, constrained restatement %.4g, device %.4g (bound %.4g); rho %g after %d updates, "
          "%d increases; f_objective %.6g (restatement %.6g); steps %d unit %d backtracked %d stalls %d resets"
          % (scene, rig.level, v_plain / rig.level, v_ref / rig.level, v_dev / rig.level, bound / rig.level, rho, rep["outer_updates"], rep["rho_increases"],
             rep["f_objective"], float(ref.con_values[0]), lb["unit_steps"], lb["backtracked_steps"], lb["stalls"], lb["resets"]))
    assert v_plain > 20.0 * tol, "the unconstrained optimum does not violate enough: choose other levels (%r, tol %r)" % (v_plain, tol)
    assert v_dev <= bound, "the device's final violation %r is above max(tol, 4 x %r) = %r" % (v_dev, v_ref, bound)
    rises = [i for i in range(199) if (i + 1) % inner != 0 and hist[i + 1] > hist[i]]
    assert not rises, "F rose inside a block at %s" % rises
    assert r["guarded"] == 0 and rep["outer_updates"] == 19, (r, rep)
    for w in final + rig.weights(o, best=True):
        assert np.all(np.isfinite(w)) and np.all(w >= 0.0), "weights that are not finite or negative"
    assert np.all(lam >= 0.0) and np.all(mu >= 0.0) and 0.0 < rho <= 1e8, "multipliers or rho out of range"


def test_refusals_leave_the_objects_usable(engine, synth):
    L = engine.lib()
    rig = ConstrainedLbfgsRig(engine, hetero_scene(synth, 64, (0.0,), spots=3, layers=1))
    try:
        eng, h = rig.eng, rig.eng._h
        arr = (C.c_void_p * 1)(rig.fields[0]._h)
        out = C.c_void_p()
        INV = abi.RTD_ERR_INVALID_ARG
        oo = rig.obj._h
        create = L.rtd_optimizer_create_constrained_lbfgs
        free, _ = rig.objective(constraints=False)
        no_terms = eng.create_objective(rig.dims)
        no_terms.add_roi(rig.rois[0])
        no_terms.add_constraint(CR.MAX_DOSE, 0, 1.0)
        rig.extra += [free, no_terms]
        # creation
        assert create(h, arr, 1, free._h, None, None, 0, C.byref(out)) == INV and not out.value and "no constraints" in L.rtd_last_error(h).decode()
        assert create(h, arr, 1, no_terms._h, None, None, 0, C.byref(out)) == INV and not out.value and "no terms" in L.rtd_last_error(h).decode()
        assert create(h, arr, 0, oo, None, None, 0, C.byref(out)) == INV and create(h, None, 1, oo, None, None, 0, C.byref(out)) == INV
        assert create(h, arr, 1, oo, None, None, 0, None) == INV
        for flags in (2, 4, 0x80000000, 3):
            assert create(h, arr, 1, oo, None, None, flags, C.byref(out)) == INV and not out.value, "flags %#x accepted" % flags
        for k, v in (("rho0", 0.0), ("rho0", math.inf), ("rho0", math.nan), ("rho_max", 0.5), ("rho_max", math.inf), ("rho_growth", 0.5), ("rho_growth", math.nan),
                     ("violation_shrink", 0.0), ("violation_shrink", 1.5), ("violation_shrink", math.nan), ("feasibility_tol", -1.0),
                     ("feasibility_tol", math.inf), ("lambda_max", 0.0), ("lambda_max", math.nan), ("inner_iterations", 0)):
            assert create(h, arr, 1, oo, None, C.byref(constrained_options(**{k: v})), 0, C.byref(out)) == INV and not out.value, (k, v)
        for k, v in (("memory", 0), ("memory", 17), ("max_halvings", 8), ("armijo_c1", 0.0), ("armijo_c1", 0.5), ("armijo_c1", math.nan), ("initial_step", -1.0),
                     ("initial_step", math.inf), ("initial_step", math.nan)):
            assert create(h, arr, 1, oo, C.byref(lbfgs_options(**{k: v})), None, 0, C.byref(out)) == INV and not out.value, (k, v)
        bad = constrained_options()
        bad.reserved[3] = 1
        assert create(h, arr, 1, oo, None, C.byref(bad), 0, C.byref(out)) == INV and not out.value
        badl = lbfgs_options()
        badl.reserved[0] = 1
        assert create(h, arr, 1, oo, C.byref(badl), None, 0, C.byref(out)) == INV and not out.value
        fresh = eng.create_field(rig.fields[0]._beam, rig.dims)       # no matrix
        assert create(h, (C.c_void_p * 1)(fresh._h), 1, oo, None, None, 0, C.byref(out)) == abi.RTD_ERR_NOT_READY and not out.value
        fresh.destroy()
        # every other creator still refuses the constrained objective
        assert L.rtd_optimizer_create(h, arr, 1, oo, None, C.byref(out)) == INV and not out.value and "hard constraints" in L.rtd_last_error(h).decode()
        assert L.rtd_optimizer_create_lbfgs(h, arr, 1, oo, None, C.byref(out)) == INV and not out.value
        assert L.rtd_optimizer_create_lbfgs_ex(h, arr, 1, oo, None, 0, C.byref(out)) == INV and not out.value and "hard constraints" in L.rtd_last_error(h).decode()
        assert L.rtd_optimizer_create_compact(h, arr, 1, oo, None, C.byref(out)) == INV and not out.value
        ro = abi.RtdRobustOptions()
        ro.mode, ro.n_scenarios = abi.RTD_ROBUST_EXPECTED, 1
        assert L.rtd_optimizer_create_robust(h, arr, 1, C.byref(ro), oo, None, C.byref(out)) == INV and not out.value
        assert L.rtd_optimizer_create_voxelwise(h, arr, 1, 1, oo, None, C.byref(out)) == INV and not out.value
        tab = (abi.RtdObjectiveTerm * len(rig.terms))(*[abi.RtdObjectiveTerm(*t) for t in rig.terms])
        assert L.rtd_planset_create(h, arr, 1, oo, tab, 1, None, C.byref(out)) == INV and not out.value
        # the new report call on the other kinds
        plain = eng.create_optimizer(rig.fields, free)
        lb = eng.create_lbfgs_optimizer(rig.fields, free)
        spectral = rig.constrained(start=60.0, con=constrained_options(inner_iterations=INNER))
        rig.opts += [plain, lb]
        for other in (plain, lb, spectral):
            assert L.rtd_optimizer_lbfgs_constraint_line(h, other._h, C.byref(abi.RtdLbfgsConstraintLineBuffers())) == INV, "the report call accepts another kind"
        opt = rig.con_lbfgs(start=60.0, con=constrained_options(inner_iterations=INNER))
        assert L.rtd_optimizer_lbfgs_constraint_line(h, opt._h, None) == INV and L.rtd_optimizer_lbfgs_constraint_line(h, None, None) == INV
        # what the new kind refuses
        rbe = eng.create_rbe(rig.dims, rbe_models.tissue("constant", 0.1, 0.05))
        assert L.rtd_optimizer_set_let_objective(h, opt._h, free._h) == INV
        assert L.rtd_optimizer_set_rbe(h, opt._h, rbe._h) == INV
        rbe.destroy()
        v, p = (C.c_double * 1)(), C.c_void_p()
        assert L.rtd_optimizer_scenario_values(h, opt._h, v, None, None) == INV
        assert L.rtd_optimizer_scenario_dose(h, opt._h, 0, C.byref(p)) == INV
        # everything is still usable
        rep0, outer0 = opt.constraint_report()
        assert rep0["rho"] == 1.0 and rep0["outer_updates"] == 0 and rep0["iterations_since_update"] == 0 and outer0 == [], rep0
        opt.run(2 * INNER)
        r, hist = opt.result()
        rep, outer = opt.constraint_report()
        assert r["iterations"] == 2 * INNER and np.all(np.isfinite(hist)) and rep["outer_updates"] == 1 and rep["n_constraints"] == 3 and len(outer) == 1, (r, rep)
        assert opt.lbfgs_report()["unit_steps"] + opt.lbfgs_report()["backtracked_steps"] > 0 and opt.lbfgs_constraint_line().n_constraints == 3
        for other, n in ((plain, 1), (lb, 1), (spectral, 1)):
            other.run(n)
            assert other.result()[0]["iterations"] == n, "another optimiser no longer runs"
        # refused at run, before the first launch: after add_roi, add_term, add_constraint; after a matrix computed again
        for change in ("roi", "term", "constraint"):
            ob, _ = rig.objective(constraints=True)
            rig.extra.append(ob)
            o2 = eng.create_constrained_lbfgs_optimizer(rig.fields, ob, None, constrained_options(inner_iterations=INNER))
            rig.opts.append(o2)
            o2.run(1)
            if change == "roi":
                ob.add_roi(rig.rois[0])
            elif change == "term":
                ob.add_term(R.MEAN, 0, 1e-3, 0.0)
            else:
                ob.add_constraint(CR.MAX_DOSE, 0, 10.0 * rig.level)
            assert L.rtd_optimizer_run(h, o2._h, 1) == abi.RTD_ERR_NOT_READY and "objective has changed" in L.rtd_last_error(h).decode(), change
            assert o2.result()[0]["iterations"] == 1, "the refused run launched (%s)" % change
        rig.fields[0].dose_influence()
        assert L.rtd_optimizer_run(h, opt._h, 1) == abi.RTD_ERR_NOT_READY and "computed again" in L.rtd_last_error(h).decode()
        assert opt.result()[0]["iterations"] == 2 * INNER
        again = rig.con_lbfgs(start=60.0)
        again.run(2)
        assert again.result()[0]["iterations"] == 2, "the fields and the objective no longer serve a new optimiser"
    finally:
        rig.close()
