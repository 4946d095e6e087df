"""CPU tests of the restatement of the constrained L-BFGS iteration (tests/constrained_lbfgs_reference.py; include/rtd.h "Constrained
L-BFGS: hard dose constraints behind the line search") on the toy plan of tests/constraint_toy.py: what the
method promises (a monotone inner solver, multipliers that stay non-negative, a penalty that grows only under section 31's rule, an
outer update at the current iterate that converges) is shown in float64 before any of it is compared with the device."""
import numpy as np
import pytest

import constraint_reference as CR
import lbfgs_terms_reference as LT
import optimizer_reference as R
from constrained_lbfgs_reference import ConstrainedLbfgsReference
from constraint_toy import Toy

START = 60.0


def _run(toy, inner, n, tree=False, **kw):
    tol = 1e-3 * toy.level
    ref = ConstrainedLbfgsReference(toy.cs, toy.matvec, toy.rmatvec, np.full(toy.n_spots, START), dict(inner_iterations=inner, feasibility_tol=tol), tree=tree, **kw)
    records = [ref.step() for _ in range(n)]
    return ref, records, tol


@pytest.fixture(scope="module")
def runs():
    toy = Toy()
    return toy, {inner: _run(toy, inner, 200) for inner in (10, 20)}


@pytest.mark.parametrize("inner", [10, 20])
def test_inner_solver_is_monotone_and_the_rules_hold(runs, inner):
    toy, by_inner = runs
    ref, records, tol = by_inner[inner]
    hist = ref.history
    assert len(hist) == 200 and [k for k, _, _ in ref.outer] == list(range(inner, 200, inner))
    accepted = 0
    for i, out in enumerate(records[:-1]):
        nxt = records[i + 1]
        if out["k"] >= 0:
            accepted += 1
            assert out["f_trial"] <= out["f"], (i, out["f_trial"], out["f"])
            if not nxt["outer"]:
                assert hist[i + 1] == out["f_trial"], "inside a block the next value is the accepted trial's (%d: %r, %r)" % (i, hist[i + 1], out["f_trial"])
        elif not nxt["outer"]:
            assert hist[i + 1] == hist[i], "nothing moved, the value stays (%d)" % i
    assert accepted > 100, accepted
    assert np.all(ref.lam >= 0.0) and np.all(ref.mu >= 0.0) and np.any(ref.lam > 0.0)
    o = ref.opt
    rho, v_prev, increases = o["rho0"], 0.0, 0
    for j, (_, r, v) in enumerate(ref.outer):
        grow = j > 0 and v > o["feasibility_tol"] and v > o["violation_shrink"] * v_prev
        rho = min(rho * o["rho_growth"], o["rho_max"]) if grow else rho
        increases += int(grow)
        assert r == rho, "rho moved outside section 31's rule at update %d: %r, expected %r" % (j, r, rho)
        v_prev = v
    assert increases == ref.rho_increases
    assert ref.guarded == 0 and np.all(np.isfinite(ref.w)) and np.all(ref.w >= 0.0)


@pytest.mark.parametrize("inner", [10, 20])
def test_convergence_on_the_toy(runs, inner):
    """The conditions the issue verified with the float64 references: the unconstrained optimum violates by more than 20 x tol, the
    final w of the constrained L-BFGS by at most tol, and its objective is not above the spectral constrained reference's f(w_best)."""
    toy, by_inner = runs
    ref, _, tol = by_inner[inner]
    w0 = np.full(toy.n_spots, START)
    plain = R.ReferenceOptimizer(toy.obj, toy.matvec, toy.rmatvec, w0, float32=False).run(200)
    v_plain = toy.violation(plain.w_best)
    spectral = CR.ConstrainedReference(toy.cs, toy.matvec, toy.rmatvec, w0, dict(inner_iterations=inner, feasibility_tol=tol), float32=False, tree=False).run(200)
    f_spectral = float(toy.obj.eval(toy.matvec(spectral.w_best))[0][0])
    v = toy.violation(ref.w)
    f = float(toy.obj.eval(toy.matvec(ref.w))[0][0])
    print("inner %d: violation / level: unconstrained %.4g, L-BFGS %.4g (tol 1e-3), spectral %.4g; f: L-BFGS %.6g, spectral %.6g; rho %g, stalls %d"
          % (inner, v_plain / toy.level, v / toy.level, toy.violation(spectral.w_best) / toy.level, f, f_spectral, ref.rho, ref.stalls))
    assert v_plain > 20.0 * tol, (v_plain, tol)
    assert v <= tol, (v, tol)
    assert f <= f_spectral, (f, f_spectral)


def test_trial_values_are_the_evaluation_of_the_rounded_trials():
    """tree=True: F_k and psi_{c,k} of every trial are ConstraintSet.eval on r_k = float32(t_k), with the multipliers of the moment;
    memory 3 and inner 4 so that the ring wraps and is forgotten at an update."""
    toy = Toy(tree=True)
    tol = 1e-3 * toy.level
    ref = ConstrainedLbfgsReference(toy.cs, toy.matvec, toy.rmatvec, np.full(toy.n_spots, START), dict(inner_iterations=4, feasibility_tol=tol), tree=True, memory=3,
                                    max_halvings=3)
    moved = False
    for i in range(11):
        pairs_before = ref.count
        d0 = None if ref.d0 is None else ref.d0.copy()
        out = ref.step()
        if d0 is None:
            d0 = ref.forward(np.full(toy.n_spots, START, dtype=np.float32))
        if out["outer"]:
            assert out["pairs"] == 0 and not out["admitted"], "the memory is dropped at an update (%d pairs before)" % pairs_before
        assert len(out["con_trial"]) == ref.K == len(out["mean_trial"])
        for k, r in enumerate(LT.rounded_trials(d0, out["d1"], ref.K)):
            values, con_values, _ = toy.cs.eval(r, ref.lam, ref.mu, out["rho"])
            assert values[0] == out["F"][k] and np.array_equal(con_values, out["con_trial"][k]), (i, k)
            assert out["mean_trial"][k][2] == toy.cs.mean(2, r.astype(np.float64)) and out["mean_trial"][k][0] == 0.0
        moved = moved or bool(np.any(ref.lam > 0.0))
    assert moved and [k for k, _, _ in ref.outer] == [4, 8]
    assert ref.f_best == min(ref.history[8:]) and ref.best_iteration >= 8, "f_best is the current subproblem's"
