"""CPU checks of the numpy restatement of the hard dose constraints (tests/constraint_reference.py) on a synthetic sparse matrix
(tests/constraint_toy.py): what the augmented Lagrangian promises, before any device is asked (no GPU needed)."""
import numpy as np
import pytest

import constraint_reference as CR
import constraint_toy as T
import optimizer_reference as R

ITER = 200
W0 = 100.0


@pytest.fixture(scope="module")
def toy():
    return T.Toy()


@pytest.fixture(scope="module")
def runs(toy):
    """The unconstrained spectral run and the constrained one at the defaults, both float64, computed once."""
    w0 = np.full(toy.n_spots, W0)
    plain = R.ReferenceOptimizer(toy.obj, toy.matvec, toy.rmatvec, w0, float32=False).run(ITER)
    con = CR.ConstrainedReference(toy.cs, toy.matvec, toy.rmatvec, w0, float32=False, tree=False)
    snapshots = []
    for _ in range(ITER):
        con.step()
        snapshots.append((con.lam.copy(), con.mu.copy()))
    return plain, con, snapshots


def test_the_plan_it_was_made_from_is_strictly_feasible(toy):
    mx, cnt = toy.cs.violations(toy.dose_true)
    assert np.all(mx == 0.0) and np.all(cnt == 0)


def test_multipliers_are_never_negative(runs):
    _, con, snapshots = runs
    assert len(con.outer) == ITER // 20 - 1
    for lam, mu in snapshots:
        assert np.all(lam >= 0.0) and np.all(mu >= 0.0)
    assert snapshots[-1][0].max() > 0.0, "no constraint ever became active: the toy tests nothing"


def test_a_satisfied_constraint_with_a_zero_multiplier_adds_exactly_nothing(toy):
    for tree in (False, True):
        cs = CR.ConstraintSet(toy.obj, tree=tree)
        for c in toy.cs.cons:
            cs.add(*c)
        dose = toy.dose_true.astype(np.float32)
        vt, gt = cs.term_values(dose)
        values, con_values, g = cs.eval(dose, np.zeros(cs.n_entries, dtype=np.float32), np.zeros(CR.MAX_CONSTRAINTS), 7.0)
        assert np.all(con_values[1:] == 0.0)
        assert values[0] == vt[0] == con_values[0]
        assert np.array_equal(g.view(np.uint32), gt.view(np.uint32))


def test_gradient_matches_a_finite_difference_of_F(toy):
    """g is float32(dF / d dose): central differences in float64 at every constrained voxel and a sample of the others, with
    multipliers that make all three constraints act. Bound: the float32 rounding of g (2^-24 relative) plus the difference's own error;
    F is piecewise quadratic, so away from a kink the central difference is exact up to rounding, 1e-9 of F / step."""
    rng = np.random.default_rng(3)
    cs = toy.cs
    dose = toy.dose_true * (1.0 + 0.08 * rng.standard_normal(toy.n_vox))
    lam = (0.5 * rng.random(cs.n_entries)).astype(np.float32)
    mu = np.zeros(CR.MAX_CONSTRAINTS)
    mu[2] = 0.3
    rho = 3.0
    values, _, g = cs.eval(dose, lam, mu, rho)
    step = 1e-5
    probe = np.unique(np.concatenate([cs.tables()["uv"], rng.choice(toy.n_vox, 60, replace=False)]))
    checked = 0
    for v in probe:
        lo, hi = dose.copy(), dose.copy()
        lo[v] -= step
        hi[v] += step
        fd = (cs.eval(hi, lam, mu, rho)[0][0] - cs.eval(lo, lam, mu, rho)[0][0]) / (2.0 * step)
        bound = 2.0 ** -23 * abs(fd) + 1e-9 * abs(values[0]) / step + 1e-12
        kink = abs(cs.eval(hi, lam, mu, rho)[2][v] - cs.eval(lo, lam, mu, rho)[2][v]) > 1e-3 * (abs(g[v]) + 1e-6)   # a clamp changes side inside the step
        if kink:
            continue
        assert abs(float(g[v]) - fd) <= bound, (v, float(g[v]), fd, bound)
        checked += 1
    assert checked > probe.size // 2
    assert np.any(g[cs.tables()["uv"]] != cs.term_values(dose)[1][cs.tables()["uv"]]), "the constraints add nothing here"


def test_the_penalty_grows_only_under_the_stated_rule(runs):
    _, con, _ = runs
    o = con.opt
    assert con.outer[0][1] == o["rho0"], "the first update never grows the penalty"
    increases = 0
    for (k0, rho0, v0), (k1, rho1, v1) in zip(con.outer, con.outer[1:]):
        assert k1 - k0 == o["inner_iterations"]
        grow = v1 > o["feasibility_tol"] and v1 > o["violation_shrink"] * v0
        assert rho1 == (min(rho0 * o["rho_growth"], o["rho_max"]) if grow else rho0), (k1, rho0, rho1, v0, v1)
        increases += grow
    assert increases == con.rho_increases and con.rho <= o["rho_max"]


def test_the_final_violation_is_below_the_unconstrained_run(toy, runs):
    plain, con, _ = runs
    v_plain, v_con = toy.violation(plain.w_best), toy.violation(con.w_best)
    print("violation / level: unconstrained %.4g, constrained %.4g" % (v_plain / toy.level, v_con / toy.level))
    assert v_plain > 0.02 * toy.level, "the unconstrained optimum does not violate: the toy tests nothing"
    assert v_con <= 0.002 * toy.level
    assert v_con < v_plain
    assert np.all(con.w >= 0.0) and np.all(np.isfinite(con.w))
