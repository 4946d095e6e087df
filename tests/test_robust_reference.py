"""The numpy restatement of the robust iteration (tests/robust_reference.py) on its own: what the decision and the combine must give
in their corner cases, the combined gradient against finite differences, and on the 1-D plan of tests/test_dvh_reference.py under
shifts and stretches that a plan optimised over the scenarios beats the nominal plan where it matters: in the worst scenario."""
import numpy as np
import pytest

import dvh_reference as D
import optimizer_reference as R
import robust_reference as Q


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_decide_expected_and_worst_case():
    f = [3.0, 7.0, 5.0]
    lam, F, worst = Q.decide(f, Q.EXPECTED, [0.5, 0.25, 0.25])
    assert list(lam) == [0.5, 0.25, 0.25] and F == ((0.0 + 0.5 * 3.0) + 0.25 * 7.0) + 0.25 * 5.0 and worst == 1
    lam, F, worst = Q.decide(f, Q.EXPECTED)
    third = 1.0 / 3.0
    assert list(lam) == [third] * 3 and F == ((0.0 + third * 3.0) + third * 7.0) + third * 5.0
    lam, F, worst = Q.decide(f, Q.WORST_CASE, [0.5, 0.25, 0.25])     # probabilities are ignored
    assert list(lam) == [0.0, 1.0, 0.0] and F == 7.0 and worst == 1
    # probabilities are used as given, not normalised
    assert Q.decide([2.0, 4.0], Q.EXPECTED, [1.0, 1.0])[1] == 6.0
    # one scenario with p = 1: F is f to the bit
    v = 0.1 + 0.2
    assert Q.decide([v], Q.EXPECTED, [1.0])[1] == v and Q.decide([v], Q.WORST_CASE)[1] == v


def test_tie_goes_to_the_lower_index():
    lam, F, worst = Q.decide([1.0, 4.0, 4.0, 2.0], Q.WORST_CASE)
    assert worst == 1 and list(lam) == [0.0, 1.0, 0.0, 0.0] and F == 4.0
    assert Q.decide([4.0, 4.0], Q.WORST_CASE)[2] == 0


@pytest.mark.parametrize("mode", [Q.EXPECTED, Q.WORST_CASE])
@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_a_value_that_is_not_finite_becomes_F(mode, bad):
    lam, F, worst = Q.decide([1.0, bad, 9.0, np.nan], mode)
    assert worst == 1 and not np.isfinite(F) and (np.isnan(F) if np.isnan(bad) else F == bad)
    assert list(lam) == ([0.25] * 4 if mode == Q.EXPECTED else [0.0, 1.0, 0.0, 0.0])


def test_combine_starts_from_the_first_product():
    g0 = np.float32([1.5, -0.0, 0.0, -3.25e-20, np.float32(1) / np.float32(3)])
    out = Q.combine([g0], [1.0])
    assert out.dtype == np.float32 and np.array_equal(_bits(out), _bits(g0)) and np.signbit(out[1]) and not np.signbit(out[2])
    # a scenario with lambda 0 is skipped, not multiplied: its row may hold anything
    junk = np.float32([np.nan, np.inf, -np.inf, 1.0, 2.0])
    out = Q.combine([junk, g0, junk], [0.0, 1.0, 0.0])
    assert np.array_equal(_bits(out), _bits(g0))
    # float64 sum of separately rounded products, ascending, rounded once
    rng = np.random.default_rng(1)
    G = rng.standard_normal((4, 50)).astype(np.float32)
    lam = np.array([0.4, 0.3, 0.2, 0.1])
    want = ((lam[0] * G[0].astype(np.float64) + lam[1] * G[1].astype(np.float64)) + lam[2] * G[2].astype(np.float64)) + lam[3] * G[3].astype(np.float64)
    assert np.array_equal(_bits(Q.combine(G, lam)), _bits(want.astype(np.float32)))


def test_one_scenario_is_the_plain_restatement():
    rng = np.random.default_rng(5)
    A = rng.random((60, 12))
    obj = R.ReferenceObjective(60)
    obj.add_term(R.SQ_DEVIATION, obj.add_roi(np.arange(10, 40)), 1.0, 2.0)
    obj.add_term(R.SQ_OVERDOSE, obj.add_roi(np.arange(40, 60)), 2.0, 0.5)
    mv, rmv = (lambda w: A @ w.astype(np.float64)), (lambda g: A.T @ g.astype(np.float64))
    plain = R.ReferenceOptimizer(obj, mv, rmv, np.ones(12)).run(15)
    for mode, p in ((Q.EXPECTED, [1.0]), (Q.WORST_CASE, None)):
        rob = Q.RobustReferenceOptimizer(obj, [mv], [rmv], np.ones(12), mode, p).run(15)
        assert np.array_equal(_bits(np.array(rob.history)), _bits(np.array(plain.history)))
        assert np.array_equal(_bits(rob.w), _bits(plain.w)) and np.array_equal(_bits(rob.w_best), _bits(plain.w_best))


def test_expected_gradient_is_the_derivative():
    """A small dense problem, three scenarios, float64 throughout: central differences of F(w) = sum_s p_s f_s(A_s w) against the
    combined gradient, within 1e-6 of its largest entry (the objective is piecewise quadratic; h = 1e-5 stays inside a piece for
    almost every entry, and the bound holds for all of them here)."""
    rng = np.random.default_rng(9)
    n, m = 80, 10
    As = [rng.random((n, m)) for _ in range(3)]
    p = np.array([0.5, 0.3, 0.2])
    obj = R.ReferenceObjective(n)
    obj.add_term(R.SQ_DEVIATION, obj.add_roi(np.arange(0, 50)), 1.0, 3.0)
    obj.add_term(R.SQ_OVERDOSE, obj.add_roi(np.arange(40, 80)), 2.0, 2.0)
    obj.add_term(R.MEAN, 1, 0.1)
    w = rng.random(m)
    F = lambda x: Q.decide([obj.eval(A @ x)[0][0] for A in As], Q.EXPECTED, p)[1]   # noqa: E731
    grads = [A.T @ obj.eval(A @ w)[1] for A in As]
    grad = Q.combine(grads, p, np.float64)
    h = 1e-5
    for j in range(m):
        e = np.zeros(m)
        e[j] = h
        fd = (F(w + e) - F(w - e)) / (2 * h)
        assert abs(fd - grad[j]) <= 1e-6 * np.abs(grad).max(), (j, fd, grad[j])


SHIFT, STRETCH, ITERATIONS = 80.0, 1.035, 100


def _line_objective():
    P = 2e-5
    obj = D.DvhReferenceObjective(4000)
    target, oar, body = obj.add_roi(np.arange(1500, 2500)), obj.add_roi(np.arange(2500, 3300)), obj.add_roi(np.arange(0, 1500))
    obj.add_term(R.SQ_DEVIATION, target, 1.0, P)
    obj.add_dvh_term(D.MIN_DVH, target, 5.0, 0.95 * P, 0.98)
    obj.add_dvh_term(D.MAX_DVH, oar, 3.0, 0.3 * P, 0.25)
    obj.add_term(R.SQ_OVERDOSE, body, 1.0, 0.5 * P)
    return obj


@pytest.mark.parametrize("seed", range(5))
def test_the_robust_plan_is_ahead_in_the_worst_scenario(seed):
    """The 1-D plan and objective of tests/test_dvh_reference.py; five scenarios: nominal, the columns displaced by +-80 voxels
    (of the order of the narrowest column's sigma, 60), the depth axis stretched by 1 / 1.035 and 1.035. A hundred iterations from
    w = 1 of the plain restatement on the nominal matrix and of the robust one in both modes: the WORST_CASE plan's worst-scenario
    objective lies below the nominal plan's, and so does the EXPECTED plan's expected value. The ratios are printed (DESIGN.md
    section 14 records them: 0.27 to 0.37 and 0.46 to 0.57)."""
    As = [Q.line_plan(seed)] + [Q.line_plan(seed, shift=s) for s in (SHIFT, -SHIFT)] + [Q.line_plan(seed, stretch=t) for t in (1.0 / STRETCH, STRETCH)]
    obj = _line_objective()
    mv = [(lambda w, A=A: A @ w.astype(np.float64)) for A in As]
    rmv = [(lambda g, A=A: A.T @ g.astype(np.float64)) for A in As]
    n = As[0].shape[1]
    nominal = R.ReferenceOptimizer(obj, mv[0], rmv[0], np.ones(n)).run(ITERATIONS)
    worst = Q.RobustReferenceOptimizer(obj, mv, rmv, np.ones(n), Q.WORST_CASE).run(ITERATIONS)
    expected = Q.RobustReferenceOptimizer(obj, mv, rmv, np.ones(n), Q.EXPECTED).run(ITERATIONS)
    f_nom, f_worst, f_exp = worst.evaluate(nominal.w_best), worst.evaluate(worst.w_best), worst.evaluate(expected.w_best)
    r_worst, r_exp = f_worst.max() / f_nom.max(), f_exp.mean() / f_nom.mean()
    print("seed %d: max_s f_s %.6g (nominal plan) -> %.6g (WORST_CASE plan), ratio %.3f; mean_s f_s %.6g -> %.6g (EXPECTED plan), ratio %.3f"
          % (seed, f_nom.max(), f_worst.max(), r_worst, f_nom.mean(), f_exp.mean(), r_exp))
    assert worst.guarded == 0 and expected.guarded == 0 and np.all(np.isfinite(worst.history))
    assert f_worst.max() == worst.f_best                            # w_best is the iterate with the best worst case
    assert r_worst < 1.0 and r_exp < 1.0
