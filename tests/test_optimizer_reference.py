"""The numpy restatement of the objective and of the optimiser's iteration (tests/optimizer_reference.py) on its own, on a synthetic
matrix: its gradient is the derivative of its value, and thirty iterations from w = 0 meet the project's bar for this loop (the
objective at no more than half its start) before any GPU is involved."""
import numpy as np
import pytest

import optimizer_reference as R

N = 32


def _matrix():
    """216 Gaussian columns (sigma 2.5 voxels, 1e-9 per particle at the centre) on a 6 x 6 x 6 lattice of a 32^3 grid, dense float64."""
    ax = np.arange(N, dtype=np.float64)
    centres = 6.0 + 4.0 * np.arange(6)
    g1 = np.exp(-0.5 * ((ax[None, :] - centres[:, None]) / 2.5) ** 2)          # [6][32]
    cols = np.einsum("az,by,cx->abczyx", g1, g1, g1).reshape(216, N ** 3)
    cols[cols < 1e-4] = 0.0
    return (1e-9 * cols).T.copy()                                             # [voxels][spots]


def _problem():
    A = _matrix()
    rng = np.random.default_rng(4)
    w_true = 50.0 + 100.0 * rng.random(A.shape[1])
    z, y, x = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    r2 = (z - 15.5) ** 2 + (y - 15.5) ** 2 + (x - 15.5) ** 2
    target, around = (r2 <= 7.0 ** 2).reshape(-1), ((r2 > 7.0 ** 2) & (r2 <= 13.0 ** 2)).reshape(-1)
    level = float((A @ w_true)[target].mean())
    obj = R.ReferenceObjective(N ** 3)
    t, a = obj.add_roi(target), obj.add_roi(around)
    obj.add_term(R.SQ_DEVIATION, t, 1.0, level)
    obj.add_term(R.SQ_UNDERDOSE, t, 5.0, 0.95 * level)
    obj.add_term(R.SQ_OVERDOSE, a, 1.0, 0.3 * level)
    obj.add_term(R.MEAN, a, 1e-3 * level)
    return A, obj, w_true, level


def test_gradient_is_the_derivative_of_the_value():
    """Central differences of the value in float64 at voxels away from the kinks (every penalty is piecewise quadratic, so the
    difference quotient is exact up to rounding): within 1e-6 of the largest gradient entry."""
    A, obj, w_true, level = _problem()
    rng = np.random.default_rng(9)
    dose = A @ (w_true * (0.6 + 0.8 * rng.random(w_true.size)))
    values, g, gabs = obj.eval(dose)
    assert values[0] > 0 and np.all(values[1:] > 0) and abs(values[0] - values[1:].sum()) <= 1e-12 * values[0]
    union = obj.union()
    assert np.all(g[~union] == 0) and np.all(gabs >= np.abs(g) * (1 - 1e-12))
    h = 1e-3 * level
    kinks = np.array([lv for _, _, _, lv in obj.terms[:3]])
    away = union & np.all(np.abs(dose[:, None] - kinks[None, :]) > 10 * h, axis=1)
    picks = rng.choice(np.flatnonzero(away), size=60, replace=False)
    assert (g[picks] < 0).any() and (g[picks] > 0).any()
    for v in picks:
        up, dn = dose.copy(), dose.copy()
        up[v] += h
        dn[v] -= h
        fd = (obj.eval(up)[0][0] - obj.eval(dn)[0][0]) / (2 * h)
        assert abs(fd - g[v]) <= 1e-6 * np.abs(g).max(), (v, fd, g[v])
    outside = np.flatnonzero(~union)[:3]
    for v in outside:
        up = dose.copy()
        up[v] += h
        assert obj.eval(up)[0][0] == values[0]


@pytest.mark.parametrize("float32", [False, True])
def test_thirty_iterations_from_zero_halve_the_objective(float32):
    A, obj, w_true, level = _problem()
    opt = R.ReferenceOptimizer(obj, lambda w: A @ w.astype(np.float64), lambda g: A.T @ g.astype(np.float64), np.zeros(A.shape[1]), float32=float32)
    for _ in range(30):
        opt.step()
        assert np.all(opt.w >= 0) and np.all(np.isfinite(opt.w))
    h = np.array(opt.history)
    print("f_0 %.6g, f_best %.6g at iteration %d, ratio %.4g (float32 vectors: %s)" % (h[0], opt.f_best, opt.best_iteration, opt.f_best / h[0], float32))
    assert opt.f_best <= 0.5 * h[0]
    fin = h[np.isfinite(h)]
    assert opt.f_best == fin.min() and h[opt.best_iteration] == opt.f_best and opt.best_iteration == int(np.argmin(np.where(np.isfinite(h), h, np.inf)))
    assert np.array_equal(obj.eval(A @ opt.w_best.astype(np.float64))[0][0], opt.f_best)


def test_step_rules_and_guard():
    """The first rule, the Barzilai-Borwein rule with its fall-back and clamp, a stationary start, and the guard."""
    w, g = np.array([1.0, 0.0, 2.0]), np.array([0.5, 3.0, -4.0])
    assert R.step_length(w, None, g, None, False) == 1.0 / 4.0                  # |P(w - g) - w| = (0.5, 0, 4)
    assert R.step_length(np.zeros(3), None, np.array([1.0, 0.0, 2.0]), None, False) == 0.0
    wp, gp = np.array([0.0, 0.0, 1.0]), np.array([0.0, 3.0, -6.0])
    assert R.step_length(w, wp, g, gp, True) == 2.0 / 2.5                       # s = (1, 0, 1), y = (0.5, 0, 2)
    assert R.step_length(w, wp, g, g + np.array([1.0, 0.0, 0.0]), True) == 1e30  # <s, y> < 0
    assert R.step_length(w, wp, g, gp, True, step_max=0.5) == 0.5
    assert np.array_equal(R.update(np.float32([1.0, 0.25]), np.float32([2.0, -1.0]), 0.5), np.float32([0.0, 0.75]))
    obj = R.ReferenceObjective(4)
    obj.add_term(R.SQ_OVERDOSE, obj.add_roi([0, 1, 2, 3]), 1.0, 1.0)
    A = np.eye(4)
    opt = R.ReferenceOptimizer(obj, lambda w: A @ w.astype(np.float64), lambda g: A.T @ g.astype(np.float64), np.zeros(4))
    opt.run(3)
    assert opt.history == [0.0, 0.0, 0.0] and np.all(opt.w == 0) and opt.best_iteration == 0
    opt = R.ReferenceOptimizer(obj, lambda w: A @ w.astype(np.float64), lambda g: A.T @ g.astype(np.float64), np.full(4, 3.0))
    opt.run(2)
    opt.w = np.full(4, np.inf, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        opt.run(2)
    assert not np.isfinite(opt.history[2]) and np.isfinite(opt.history[3]) and opt.guarded == 1 and np.all(np.isfinite(opt.w))
