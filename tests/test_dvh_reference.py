"""The numpy restatement of the dose-volume terms (tests/dvh_reference.py) on its own: the properties that make it a dose-volume
penalty, and the convergence of the existing restated optimiser with DVH terms on a synthetic plan, before any GPU is involved."""
import numpy as np
import pytest

import dvh_reference as D
import optimizer_reference as R


def _one_roi(n=200, seed=3):
    rng = np.random.default_rng(seed)
    obj = D.DvhReferenceObjective(n + 20)
    roi = obj.add_roi(np.arange(5, 5 + n))
    dose = np.zeros(n + 20, dtype=np.float32)
    dose[5:5 + n] = rng.random(n).astype(np.float32)          # distinct values in [0, 1)
    return obj, roi, dose


def test_rank_and_dose_at_volume():
    """v = 1 is the minimum of the ROI, the smallest fraction (and anything below 1 / N) the maximum, and in between the k-th largest
    with k = ceil(v N); ties are values of the ROI like any other."""
    obj, roi, dose = _one_roi()
    dv = dose[obj.rois[roi]]
    n = dv.size
    assert [D.rank(v, n) for v in (1.0 / n, 1e-9, 0.02, 0.5, 0.95, 0.98, 1.0)] == [1, 1, 4, 100, 190, 196, 200]
    assert D.rank(1.0, 1) == D.rank(0.3, 1) == 1 and D.rank(0.5, 3) == 2
    got = obj.dose_at_volume(dose, [(roi, 1.0), (roi, 1.0 / n), (roi, 1e-9), (roi, 0.5)])
    desc = np.sort(dv)[::-1]
    assert got.dtype == np.float32 and got[0] == dv.min() and got[1] == got[2] == dv.max() and got[3] == desc[99]
    tied = np.float32([3, 1, 3, 2, 3, 1, 2, 3])
    o2 = D.DvhReferenceObjective(8)
    r2 = o2.add_roi(np.arange(8))
    assert list(o2.dose_at_volume(tied, [(r2, v) for v in (0.125, 0.5, 0.625, 0.75, 0.76, 1.0)])) == [3, 3, 2, 2, 1, 1]


def test_cumulative_histogram():
    obj, roi, dose = _one_roi()
    dose[7] = 0.25                                             # exactly on an edge of 8 bins over [0, 1)
    dose[8] = 5.0                                              # above dose_max: in every bin
    h = obj.dvh(dose, 8, 1.0)
    dv = dose[obj.rois[roi]].astype(np.float64)
    assert h.shape == (1, 8) and h.dtype == np.uint32 and h[0, 0] == dv.size
    assert np.all(np.diff(h[0].astype(np.int64)) <= 0)
    assert h[0, 2] == (dv >= 0.25).sum() and h[0, 7] == (dv >= 0.875).sum() >= 1


@pytest.mark.parametrize("kind", [D.MAX_DVH, D.MIN_DVH])
def test_a_satisfied_constraint_costs_nothing(kind):
    """MAX_DVH: D_v <= level (at most a fraction v above the level); MIN_DVH: D_v >= level. Value 0 and gradient 0, although single
    voxels lie on the wrong side of the level."""
    obj, roi, dose = _one_roi()
    v = 0.25 if kind == D.MAX_DVH else 0.9
    d_v = float(obj.dose_at_volume(dose, [(roi, v)])[0])
    level = d_v + 0.01 if kind == D.MAX_DVH else d_v - 0.01
    dv = dose[obj.rois[roi]]
    assert ((dv > level) if kind == D.MAX_DVH else (dv < level)).sum() > 5
    obj.add_dvh_term(kind, roi, 2.0, level, v)
    values, g, gabs = obj.eval(dose)
    assert values[0] == 0.0 and values[1] == 0.0 and not g.any() and not gabs.any()
    # violated: exactly the voxels between the level and D_v pay
    level = d_v - 0.1 if kind == D.MAX_DVH else d_v + 0.05
    o2 = D.DvhReferenceObjective(obj.n_voxels)
    o2.add_roi(obj.rois[roi])
    o2.add_dvh_term(kind, 0, 2.0, level, v)
    values, g, _ = o2.eval(dose)
    d64 = dose.astype(np.float64)
    pays = np.zeros(dose.size, dtype=bool)
    pays[obj.rois[roi]] = True
    pays &= ((d64 > level) & (d64 <= d_v)) if kind == D.MAX_DVH else ((d64 < level) & (d64 >= d_v))
    assert pays.sum() > 3 and np.array_equal(g != 0, pays)
    want = 2.0 / 200.0 * float(np.sum(((d64 - level) ** 2)[pays]))
    assert abs(values[0] - want) <= 200 * 2.0 ** -52 * want            # (another order of the same 200 or fewer additions)
    assert np.all(g[pays] > 0) if kind == D.MAX_DVH else np.all(g[pays] < 0)
    nan = dose.copy()
    nan[obj.rois[roi][3]] = np.nan
    assert np.isnan(o2.eval(nan)[0][0])


def test_gradient_is_the_derivative_of_the_value():
    """Central differences at voxels away from the level and from D_v (there the term is a quadratic in the voxel's dose and D_v
    does not move): within 1e-6 of the largest gradient entry. Mixed with a plain term on an overlapping ROI."""
    rng = np.random.default_rng(11)
    n = 400
    obj = D.DvhReferenceObjective(n)
    a, b = obj.add_roi(np.arange(0, 300)), obj.add_roi(np.arange(200, 400))
    obj.add_dvh_term(D.MAX_DVH, a, 3.0, 0.3, 0.25)
    obj.add_term(R.SQ_DEVIATION, b, 1.0, 0.6)
    obj.add_dvh_term(D.MIN_DVH, b, 5.0, 0.7, 0.9)
    dose = rng.random(n)
    values, g, _ = obj.eval(dose)
    assert np.all(values[1:] > 0)
    da = float(np.sort(dose[:300])[::-1][D.rank(0.25, 300) - 1])
    db = float(np.sort(dose[200:])[::-1][D.rank(0.9, 200) - 1])
    h = 1e-4
    away = np.all(np.abs(dose[:, None] - np.array([0.3, 0.7, da, db])[None, :]) > 10 * h, axis=1)
    picks = rng.choice(np.flatnonzero(away), size=80, replace=False)
    assert (g[picks] != 0).sum() > 20
    for v in picks:
        up, dn = dose.copy(), dose.copy()
        up[v] += h
        dn[v] -= h
        fd = (obj.eval(up)[0][0] - obj.eval(dn)[0][0]) / (2 * h)
        assert abs(fd - g[v]) <= 1e-6 * np.abs(g).max(), (v, fd, g[v])


def _plan(seed):
    """4000 voxels on a line, 120 Gaussian columns (sigma 60 to 150 voxels, 1e-6 at the centre, float32, entries below 1e-9 zeroed)."""
    rng = np.random.default_rng(seed)
    x = np.arange(4000, dtype=np.float64)
    centre, sigma = rng.uniform(0.0, 4000.0, 120), rng.uniform(60.0, 150.0, 120)
    A = (1e-6 * np.exp(-0.5 * ((x[:, None] - centre[None, :]) / sigma[None, :]) ** 2)).astype(np.float32)
    A[A < 1e-9] = 0.0
    P = 2e-5
    obj = D.DvhReferenceObjective(4000)
    target, oar, body = obj.add_roi(np.arange(1500, 2500)), obj.add_roi(np.arange(2500, 3300)), obj.add_roi(np.arange(0, 1500))
    obj.add_term(R.SQ_DEVIATION, target, 1.0, P)
    obj.add_dvh_term(D.MIN_DVH, target, 5.0, 0.95 * P, 0.98)
    obj.add_dvh_term(D.MAX_DVH, oar, 3.0, 0.3 * P, 0.25)
    obj.add_term(R.SQ_OVERDOSE, body, 1.0, 0.5 * P)
    return A.astype(np.float64), obj, P


@pytest.mark.parametrize("seed", range(5))
def test_sixty_iterations_with_dvh_terms(seed):
    """The existing restated optimiser from w = 1: f_best at no more than 1 % of f_0, and the OAR's volume above 30 % of the
    prescription brought from at least three quarters to at most 30 % (the constraint asks for 25 %; a penalty gets close, not there).
    The history is not monotone (Barzilai-Borwein), so only f_best is bounded."""
    A, obj, P = _plan(seed)
    opt = R.ReferenceOptimizer(obj, lambda w: A @ w.astype(np.float64), lambda g: A.T @ g.astype(np.float64), np.ones(A.shape[1]))
    opt.run(60)
    h = np.array(opt.history)
    oar = obj.rois[1]
    above = lambda w: float(((A @ w.astype(np.float64))[oar] > 0.3 * P).mean())   # noqa: E731
    start, best = above(np.ones(A.shape[1])), above(opt.w_best)
    print("seed %d: f_0 %.6g, f_best %.6g at iteration %d (ratio %.4g), %d upward steps; OAR above 0.3 P: %.3f at the start, %.3f at w_best"
          % (seed, h[0], opt.f_best, opt.best_iteration, opt.f_best / h[0], int((np.diff(h) > 0).sum()), start, best))
    assert np.all(np.isfinite(h)) and opt.guarded == 0
    assert opt.f_best / h[0] <= 0.01
    assert start >= 0.75
    assert best <= 0.30
