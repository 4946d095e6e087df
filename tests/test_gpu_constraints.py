"""GPU tests of the hard dose constraints (include/rtd.h "Hard dose constraints: an augmented Lagrangian resident on the device",
DESIGN.md section 31) against their numpy restatement (tests/constraint_reference.py), through the C ABI.

Part one needs no field: an objective on a 40^3 grid, doses uploaded, every kernel of rtd_constrain.hpp reached through the public
calls and compared bit for bit (the restatement follows the device's summation trees). Part two runs the constrained optimiser on
the heterogeneous phantom (tests/constraint_rig.py).

Measured on the device (MI355X), part two's convergence test, violation of w_best in units of the target's level after 200
iterations, inner_iterations 20, feasibility_tol 1e-3 x level; these are the numbers DESIGN.md section 31 quotes:
  one field   unconstrained restatement 0.4264, constrained restatement 0.008477, device 0.002851 (bound 0.03391); rho 16384, 7 increases
  two fields  unconstrained restatement 0.5235, constrained restatement 0.008307, device 0.009192 (bound 0.03323); rho 65536, 8 increases
Most of the nine outer updates go into raising rho; neither run reaches feasibility_tol within 200 iterations."""
import ctypes as C
import math

import numpy as np
import pytest

import constraint_reference as CR
import optimizer_reference as R
from constraint_rig import ConstraintRig, constrained_options, same_state
from gpu_support import bits, hetero_scene, rig_fixture
from raytracedicom_amd import abi, rbe as rbe_models

pytestmark = pytest.mark.gpu

rig_of = rig_fixture(ConstraintRig)

# ---- part one: the kernels, no fields ---------------------------------------------------------------------------------------------

DIMS = (40, 40, 40)
NVOX = 64000
SENTINEL = np.uint32(0x7FC00123)
RHO, LAMBDA_MAX, TOL = 2.5, 1.2, 0.05


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
    rois = _rois()
    base = (2.0 * np.random.default_rng(8).random(NVOX)).astype(np.float32)
    both = np.intersect1d(rois[3], rois[4])
    only_big = np.setdiff1d(np.setdiff1d(rois[3], rois[4]), rois[6])
    with_nan, with_inf = base.copy(), base.copy()
    with_nan[only_big[7]] = np.nan                                    # in a per-voxel constraint only: its psi, F and that voxel's g are NaN
    with_inf[both[3]] = np.inf                                        # in two per-voxel constraints and a mean one
    return {"random": base, "nan": with_nan, "inf": with_inf}


@pytest.fixture(scope="module")
def part_one(engine):
    """One engine, the objective with its constraints, the restatement and the multipliers, shared by the tests of part one."""
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
        assert obj.add_constraint(*c) == k == cs.add(*c)
    rng = np.random.default_rng(77)
    lam = rng.random(cs.n_entries).astype(np.float32)
    lam[rng.random(cs.n_entries) < 0.3] = 0.0
    mu = np.zeros(CR.MAX_CONSTRAINTS)
    mu[1], mu[5] = 0.25, 0.0
    bufs = {k: eng.device_alloc(n) for k, n in (("dose", 4 * NVOX), ("g", 4 * NVOX), ("lam", 4 * cs.n_entries), ("mu", 8 * CR.MAX_CONSTRAINTS))}
    yield eng, obj, cs, lam, mu, bufs
    for p in bufs.values():
        eng.device_free(p)
    obj.destroy()
    eng.close()


def _same_floats(a, b):
    """Bit for bit, a NaN matching any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def test_layout_is_the_restatements(part_one):
    eng, obj, cs, _, _, _ = part_one
    lay, t = obj.constraint_layout(), cs.tables()
    assert (lay.n_union, lay.n_entries, lay.n_constraints, lay.n_mean) == (t["uv"].size, cs.n_entries, len(CONS), 2)
    assert lay.n_union > 64 * 256, "the reducer's lane loop must wrap"
    uv, ptr, idx = np.empty(lay.n_union, dtype=np.int32), np.empty(lay.n_union + 1, dtype=np.int32), np.empty(lay.n_entries, dtype=np.uint8)
    eng.to_host(uv, lay.union_voxels)
    eng.to_host(ptr, lay.entry_ptr)
    eng.to_host(idx, lay.entry_constraint)
    assert np.array_equal(uv, t["uv"]) and np.array_equal(ptr, t["ptr"]) and np.array_equal(idx, t["idx"])
    assert np.diff(ptr).max() >= 3, "a voxel of three per-voxel constraints exercises the order within a voxel"


@pytest.mark.parametrize("which", ["random", "nan", "inf"])
def test_eval_constrained_bit_for_bit(part_one, which):
    eng, obj, cs, lam, mu, b = part_one
    dose = _doses()[which]
    eng.to_device(b["dose"], dose)
    eng.to_device(b["lam"], lam)
    eng.to_device(b["mu"], mu)
    results = []
    for _ in range(2):                                                # a second call gives the same bits
        eng.to_device(b["g"], np.full(NVOX, SENTINEL, dtype=np.uint32))
        values, con_values = obj.eval_constrained(b["dose"], b["lam"], b["mu"], RHO, b["g"])
        g = np.empty(NVOX, dtype=np.float32)
        eng.to_host(g, b["g"])
        results.append((values, con_values, g))
    for x, y in zip(results[0], results[1]):
        assert np.array_equal(bits(x), bits(y))
    values, con_values, g = results[0]
    # the terms alone, through the entry point that ignores constraints
    eng.to_device(b["g"], np.full(NVOX, SENTINEL, dtype=np.uint32))
    plain = obj.eval(b["dose"], b["g"])
    g_terms = np.empty(NVOX, dtype=np.float32)
    eng.to_host(g_terms, b["g"])
    rv, rc, rg = cs.eval(dose, lam, mu, RHO)
    print("%s: F %.17g (restatement %.17g), terms %.17g, psi %s" % (which, values[0], rv[0], con_values[0], con_values[1:]))
    assert _same_floats(plain, np.concatenate([[con_values[0]], values[1:]])), "eval ignores the constraints; values[1 + t] stay the terms'"
    assert _same_floats(con_values, rc), (con_values, rc)
    assert _same_floats(values, rv), (values, rv)
    union = cs.obj.union()
    assert np.all(bits(g)[~union] == SENTINEL) and _same_floats(g[union], rg[union])
    uv = cs.tables()["uv"]
    outside = union.copy()
    outside[uv] = False
    assert np.array_equal(bits(g[outside]), bits(g_terms[outside])), "a voxel without a constraint keeps the terms' gradient"
    bare = cs.obj.rois[5]
    for r in (0, 1, 2, 3, 4, 6):
        bare = np.setdiff1d(bare, cs.obj.rois[r])                     # its voxels that no term reaches
    assert bare.size > 50 and np.all(g_terms[bare] == 0.0) and np.any(g[bare] != 0.0), "the ROI without a term is written by eval (0) and gets the constraint's gradient"
    if which == "random":
        assert np.all(np.isfinite(values)) and np.all(con_values[1:] != 0.0), "every constraint acts somewhere"
    else:
        assert not np.isfinite(values[0])


@pytest.mark.parametrize("which", ["random", "nan", "inf"])
def test_update_multipliers_bit_for_bit(part_one, which):
    eng, obj, cs, lam, mu, b = part_one
    dose = _doses()[which]
    eng.to_device(b["dose"], dose)
    results = []
    for _ in range(2):
        eng.to_device(b["lam"], lam)
        eng.to_device(b["mu"], mu)
        mx, cnt = obj.update_multipliers(b["dose"], RHO, b["lam"], b["mu"], LAMBDA_MAX, TOL)
        l2, m2 = np.empty_like(lam), np.empty_like(mu)
        eng.to_host(l2, b["lam"])
        eng.to_host(m2, b["mu"])
        results.append((mx, cnt, l2, m2))
    for x, y in zip(results[0], results[1]):
        assert np.array_equal(bits(x) if x.dtype != np.uint32 else x, bits(y) if y.dtype != np.uint32 else y)
    mx, cnt, l2, m2 = results[0]
    rl, rm, rmx, rcnt = cs.update(dose, RHO, lam, mu, LAMBDA_MAX, TOL)
    print("%s: max violation %s, violating %s" % (which, mx, cnt))
    assert np.array_equal(bits(l2), bits(rl)) and np.array_equal(bits(m2), bits(rm))
    assert np.array_equal(bits(mx), bits(rmx)) and np.array_equal(cnt.astype(np.int64), rcnt)
    assert np.all(l2 >= 0.0) and l2.max() == np.float32(LAMBDA_MAX) and np.any(l2 == 0.0), "both clamps act"
    assert np.all(m2[[0, 2, 3, 4, 6, 7]] == mu[[0, 2, 3, 4, 6, 7]]), "mu of a per-voxel constraint is not written"
    # the same pass without the update
    eng.to_device(b["lam"], lam)
    vx, vc = obj.constraint_violations(b["dose"], TOL)
    assert np.array_equal(bits(vx), bits(mx)) and np.array_equal(vc, cnt)
    eng.to_host(l2, b["lam"])
    assert np.array_equal(bits(l2), bits(lam))
    if which == "inf":
        assert mx[0] == np.inf and np.isfinite(rl).all(), "an infinite h counts as a violation and leaves its multiplier"
    if which == "nan":
        assert np.all(np.isfinite(mx)), "a NaN h is left out"


# ---- part two: the constrained optimiser ------------------------------------------------------------------------------------------

INNER = 4
SCENES = {"one": (0.0,), "two": (0.0, 90.0)}


@pytest.mark.parametrize("scene", list(SCENES))
def test_iterations_equal_a_loop_of_public_calls(rig_of, synth, scene):
    """2 x inner + 3 iterations, across two outer updates."""
    rig = rig_of(hetero_scene(synth, 96, SCENES[scene]))
    con = constrained_options(inner_iterations=INNER, feasibility_tol=1e-3 * rig.level)
    n = 2 * INNER + 3
    o = rig.constrained(start=60.0, con=con)
    o.run(n)
    st = rig.driven_loop(60.0, n, con)
    r, hist = o.result()
    rep, outer = o.constraint_report()
    lam, mu, rho = rig.multipliers(o)
    print("history", hist, "outer", outer, "report", rep)
    assert r["iterations"] == n and np.array_equal(bits(hist), bits(np.array(st.history)))
    assert np.array_equal(bits(np.concatenate([w.reshape(-1) for w in rig.weights(o)])), bits(st.w))
    assert np.array_equal(bits(np.concatenate([w.reshape(-1) for w in rig.weights(o, best=True)])), bits(st.w_best))
    assert np.array_equal(bits(lam), bits(st.lam)) and np.array_equal(bits(mu), bits(st.mu)) and rho == st.rho == rep["rho"]
    assert outer == [(k, rh, v) for k, rh, v in st.outer] and [k for k, _, _ in outer] == [INNER, 2 * INNER]
    assert rep["outer_updates"] == 2 and rep["rho_increases"] == st.rho_increases and rep["iterations_since_update"] == 3
    assert rep["f_objective"] == st.con_values[0] and np.array_equal(bits(np.array(rep["psi"])), bits(st.con_values[1:]))
    assert np.array_equal(bits(np.array(rep["max_violation"])), bits(st.last_violation[0])) and list(rep["n_violating"]) == list(st.last_violation[1])
    assert r["f_best"] == st.f_best and r["best_iteration"] == st.best_iteration and r["guarded"] == 0
    assert lam.max() > 0.0, "no multiplier moved: the scene tests nothing"


def test_resident_means_resident(rig_of, synth):
    """run(3 inner) = run(inner) three times; run(2 inner) captured into a graph and replayed once = the direct call."""
    import torch
    rig = rig_of(hetero_scene(synth, 96, SCENES["one"]))
    con = constrained_options(inner_iterations=INNER, feasibility_tol=1e-3 * rig.level)
    a, b = rig.constrained(start=60.0, con=con), rig.constrained(start=60.0, con=con)
    a.run(3 * INNER)
    for _ in range(3):
        b.run(INNER)
        b.run(0)
    ra, ha, ca, oa = same_state(rig, a, b, "split runs")
    assert ha.size == 3 * INNER and ca["outer_updates"] == 2 and ca["iterations_since_update"] == INNER
    direct, captured = rig.constrained(start=60.0, con=con), rig.constrained(start=60.0, con=con)
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
    assert hd.size == 2 * INNER and np.array_equal(bits(hd), bits(ha[:2 * INNER])) and cd["outer_updates"] == 1


@pytest.mark.parametrize("scene", list(SCENES))
def test_convergence(rig_of, synth, scene):
    """200 iterations, inner_iterations 20, feasibility_tol 1e-3 x level. The restatement alone (float64 products) shows that the scene
    is a real test: the unconstrained run must violate by more than 20 x feasibility_tol. The device's w_best must then violate by at
    most max(feasibility_tol, 4 x the restatement's final violation): Barzilai-Borwein amplifies last-bit differences between the
    float32 and the float64 trajectory."""
    rig = rig_of(hetero_scene(synth, 96, SCENES[scene]))
    tol = 1e-3 * rig.level
    w0 = np.full(sum(rig.sizes), 60.0)
    cs = rig.cset(tree=False)
    plain = R.ReferenceOptimizer(rig.ref, rig.matvec, rig.rmatvec, w0, float32=False).run(200)
    v_plain = float(cs.violations(rig.matvec(plain.w_best))[0].max())
    ref = CR.ConstrainedReference(cs, rig.matvec, rig.rmatvec, w0, dict(inner_iterations=20, feasibility_tol=tol), float32=False, tree=False).run(200)
    v_ref = float(cs.violations(rig.matvec(ref.w_best))[0].max())
    o = rig.constrained(start=60.0, con=constrained_options(inner_iterations=20, feasibility_tol=tol))
    o.run(200)
    best = rig.weights(o, best=True)
    v_dev, mx, cnt = rig.violation_of(best, tol)
    rep, outer = o.constraint_report()
    lam, mu, rho = rig.multipliers(o)
    print("%s: level %.6g; violation / level: unconstrained restatement %.4g, constrained restatement %.4g, device %.4g (bound %.4g); rho %g after %d updates, "
          "%d increases; f_objective %.6g (unconstrained f_best %.6g)" % (scene, rig.level, v_plain / rig.level, v_ref / rig.level, v_dev / rig.level,
                                                                         max(tol, 4.0 * v_ref) / rig.level, rho, rep["outer_updates"], rep["rho_increases"],
                                                                         rep["f_objective"], plain.f_best))
    assert v_plain > 20.0 * tol, "the unconstrained optimum does not violate enough: choose other levels"
    assert v_dev <= max(tol, 4.0 * v_ref), (v_dev, v_ref, tol)
    for w in best + rig.weights(o):
        assert np.all(np.isfinite(w)) and np.all(w >= 0.0)
    assert np.all(lam >= 0.0) and np.all(mu >= 0.0) and 0.0 < rho <= 1e8 and rep["outer_updates"] == 9
    assert o.result()[0]["guarded"] == 0


def test_refusals_leave_the_objects_usable(engine, synth):
    L = engine.lib()
    rig = ConstraintRig(engine, hetero_scene(synth, 64, (0.0,), spots=3, layers=1))
    try:
        eng, h = rig.eng, rig.eng._h
        arr = (C.c_void_p * 1)(rig.fields[0]._h)
        out = C.c_void_p()
        INV = abi.RTD_ERR_INVALID_ARG
        # section 1: add_constraint
        cid = C.c_int32(-7)
        for c in (abi.RtdDoseConstraint(4, 0, 1.0), abi.RtdDoseConstraint(-1, 0, 1.0), abi.RtdDoseConstraint(0, 99, 1.0), abi.RtdDoseConstraint(0, -1, 1.0),
                  abi.RtdDoseConstraint(0, 0, math.nan), abi.RtdDoseConstraint(0, 0, math.inf)):
            assert L.rtd_objective_add_constraint(h, rig.obj._h, C.byref(c), C.byref(cid)) == INV and cid.value == -7
        bad = abi.RtdDoseConstraint(0, 0, 1.0)
        bad.reserved[1] = 1
        assert L.rtd_objective_add_constraint(h, rig.obj._h, C.byref(bad), None) == INV
        assert L.rtd_objective_add_constraint(h, rig.obj._h, None, None) == INV
        full, _ = rig.objective(constraints=False)
        rig.extra.append(full)
        for k in range(abi.RTD_CON_MAX_CONSTRAINTS):
            assert full.add_constraint(CR.MAX_DOSE, 0, 1.0 + k) == k
        assert L.rtd_objective_add_constraint(h, full._h, C.byref(abi.RtdDoseConstraint(0, 0, 1.0)), None) == INV
        # ... and every other creator refuses an objective that has one, before any launch
        oo = rig.obj._h
        assert L.rtd_optimizer_create(h, arr, 1, oo, None, C.byref(out)) == INV and not out.value
        assert "hard constraints" in L.rtd_last_error(h).decode()
        ro = abi.RtdRobustOptions()
        ro.mode, ro.n_scenarios = abi.RTD_ROBUST_EXPECTED, 1
        for create in (L.rtd_optimizer_create_robust, L.rtd_optimizer_create_robust_compact):
            assert create(h, arr, 1, C.byref(ro), oo, None, C.byref(out)) == INV and not out.value
        for create in (L.rtd_optimizer_create_voxelwise, L.rtd_optimizer_create_voxelwise_compact):
            assert create(h, arr, 1, 1, oo, None, C.byref(out)) == INV and not out.value
        assert L.rtd_optimizer_create_compact(h, arr, 1, oo, None, C.byref(out)) == INV and not out.value
        assert L.rtd_optimizer_create_lbfgs(h, arr, 1, oo, None, C.byref(out)) == INV and not out.value
        assert L.rtd_optimizer_create_lbfgs_ex(h, arr, 1, oo, None, 0, C.byref(out)) == INV and not out.value
        tab = (abi.RtdObjectiveTerm * len(rig.terms))(*[abi.RtdObjectiveTerm(*t) for t in rig.terms])
        assert L.rtd_planset_create(h, arr, 1, oo, tab, 1, None, C.byref(out)) == INV and not out.value
        assert "hard constraints" in L.rtd_last_error(h).decode()
        # a plain optimiser on an objective WITHOUT constraints: an added, never used ROI changes no bit of run(10)
        # (the ROI lies behind every other voxel of the union: rtd_objective_eval sums one thread per union voxel in blocks of 256, so
        # an ROI in front would move every voxel to another thread and change the last bits of the sums, with or without this block)
        free_a, _ = rig.objective(constraints=False)
        last = int(max(np.flatnonzero(m)[-1] for m in rig.rois))
        never = np.zeros(rig.nvox, dtype=bool)
        never[last + 1:last + 51] = True
        assert never.sum() == 50, "no room behind the union"
        free_b, _ = rig.objective(constraints=False, extra_roi=never)
        rig.extra += [free_a, free_b]
        hists = []
        for ob in (free_a, free_b):
            p = eng.create_optimizer(rig.fields, ob)
            rig.opts.append(p)
            rig.set_weights(p, 60.0)
            p.run(10)
            hists.append(p.result()[1])
        assert hists[0].size == 10 and np.array_equal(bits(hists[0]), bits(hists[1]))
        plain = rig.opts[-1]
        assert L.rtd_optimizer_set_let_objective(h, plain._h, oo) == INV and "hard constraints" in L.rtd_last_error(h).decode()
        # section 3: the calls on an objective
        d = rig.alloc(4 * rig.nvox)
        lam, mu, vals, viol = rig.alloc(4 * rig.nvox), rig.alloc(8 * 16), rig.alloc(8 * 65), rig.alloc(16 * 16)
        lay = abi.RtdConstraintLayout()
        assert L.rtd_objective_constraint_layout(h, free_a._h, C.byref(lay)) == INV
        assert L.rtd_objective_eval_constrained(h, free_a._h, d, lam, mu, 1.0, vals, vals, d) == INV and "no constraints" in L.rtd_last_error(h).decode()
        assert L.rtd_objective_update_multipliers(h, free_a._h, d, 1.0, 1.0, 0.0, lam, mu, viol) == INV
        assert L.rtd_objective_constraint_violations(h, free_a._h, d, 0.0, viol) == INV
        no_terms = eng.create_objective(rig.dims)
        rig.extra.append(no_terms)
        no_terms.add_roi(rig.rois[0])
        no_terms.add_constraint(CR.MAX_DOSE, 0, 1.0)
        assert L.rtd_objective_eval_constrained(h, no_terms._h, d, lam, mu, 1.0, vals, vals, d) == INV
        for rho in (0.0, -1.0, math.inf, math.nan):
            assert L.rtd_objective_eval_constrained(h, oo, d, lam, mu, rho, vals, vals, d) == INV
            assert L.rtd_objective_update_multipliers(h, oo, d, rho, 1.0, 0.0, lam, mu, viol) == INV
        assert L.rtd_objective_update_multipliers(h, oo, d, 1.0, 0.0, 0.0, lam, mu, viol) == INV
        assert L.rtd_objective_update_multipliers(h, oo, d, 1.0, math.nan, 0.0, lam, mu, viol) == INV
        assert L.rtd_objective_update_multipliers(h, oo, d, 1.0, 1.0, -1.0, lam, mu, viol) == INV
        assert L.rtd_objective_constraint_violations(h, oo, d, math.nan, viol) == INV
        assert L.rtd_objective_eval_constrained(h, oo, d, None, mu, 1.0, vals, vals, d) == INV
        assert L.rtd_objective_update_multipliers(h, oo, d, 1.0, 1.0, 0.0, lam, mu, None) == INV
        assert L.rtd_objective_constraint_violations(h, oo, None, 0.0, viol) == INV
        # section 5: the creator and what the optimiser refuses
        create = L.rtd_optimizer_create_constrained
        assert create(h, arr, 1, free_a._h, None, None, C.byref(out)) == INV and not out.value
        assert create(h, arr, 1, no_terms._h, None, None, C.byref(out)) == INV
        assert create(h, arr, 0, oo, None, None, C.byref(out)) == INV and create(h, None, 1, oo, None, None, C.byref(out)) == INV
        for k, v in (("rho0", 0.0), ("rho0", math.inf), ("rho0", math.nan), ("rho_max", 0.5), ("rho_max", math.inf), ("rho_growth", 0.5), ("rho_growth", math.nan),
                     ("violation_shrink", 0.0), ("violation_shrink", 1.5), ("violation_shrink", math.nan), ("feasibility_tol", -1.0),
                     ("feasibility_tol", math.inf), ("lambda_max", 0.0), ("lambda_max", math.nan), ("inner_iterations", 0)):
            assert create(h, arr, 1, oo, None, C.byref(constrained_options(**{k: v})), C.byref(out)) == INV and not out.value, (k, v)
        bad = constrained_options()
        bad.reserved[3] = 1
        assert create(h, arr, 1, oo, None, C.byref(bad), C.byref(out)) == INV
        fresh = eng.create_field(rig.fields[0]._beam, rig.dims)       # no matrix
        assert create(h, (C.c_void_p * 1)(fresh._h), 1, oo, None, None, C.byref(out)) == abi.RTD_ERR_NOT_READY
        fresh.destroy()
        opt = rig.constrained(start=60.0, con=constrained_options(inner_iterations=INNER))
        rbe = eng.create_rbe(rig.dims, rbe_models.tissue("constant", 0.1, 0.05))
        assert L.rtd_optimizer_set_let_objective(h, opt._h, free_a._h) == INV
        assert L.rtd_optimizer_set_rbe(h, opt._h, rbe._h) == INV
        rbe.destroy()
        v, p = (C.c_double * 1)(), C.c_void_p()
        assert L.rtd_optimizer_scenario_values(h, opt._h, v, None, None) == INV
        assert L.rtd_optimizer_scenario_dose(h, opt._h, 0, C.byref(p)) == INV
        assert L.rtd_optimizer_lbfgs_report(h, opt._h, C.byref(abi.RtdLbfgsReport())) == INV
        assert L.rtd_optimizer_lbfgs_buffers(h, opt._h, C.byref(abi.RtdLbfgsBuffers())) == INV
        assert L.rtd_optimizer_lbfgs_line_buffers(h, opt._h, C.byref(abi.RtdLbfgsLineBuffers())) == INV
        assert L.rtd_optimizer_constraint_report(h, plain._h, C.byref(abi.RtdConstraintReport()), None, 0) == INV
        assert L.rtd_optimizer_constraint_buffers(h, plain._h, C.byref(abi.RtdConstraintBuffers())) == INV
        assert L.rtd_optimizer_constraint_report(h, opt._h, None, None, 0) == INV
        assert L.rtd_optimizer_constraint_report(h, opt._h, C.byref(abi.RtdConstraintReport()), None, 4) == INV
        # everything is still usable
        rep0, outer0 = opt.constraint_report()
        assert rep0["rho"] == 1.0 and rep0["outer_updates"] == 0 and rep0["iterations_since_update"] == 0 and outer0 == []
        opt.run(2 * INNER)
        r, hist = opt.result()
        rep, outer = opt.constraint_report()
        assert r["iterations"] == 2 * INNER and np.all(np.isfinite(hist)) and rep["outer_updates"] == 1 and rep["n_constraints"] == 3 and len(outer) == 1
        plain.run(1)
        assert plain.result()[0]["iterations"] == 11
        # the stale-matrix habit: a matrix computed again, or an objective that changed, and run refuses before its first launch
        other = rig.constrained(start=60.0)
        rig.obj.add_roi(never)
        assert L.rtd_optimizer_run(h, other._h, 1) == abi.RTD_ERR_NOT_READY and "objective has changed" in L.rtd_last_error(h).decode()
        rig.fields[0].dose_influence()
        assert L.rtd_optimizer_run(h, opt._h, 1) == abi.RTD_ERR_NOT_READY and "computed again" in L.rtd_last_error(h).decode()
        assert opt.result()[0]["iterations"] == 2 * INNER
    finally:
        rig.close()
