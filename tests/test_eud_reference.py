"""The numpy restatement of the EUD terms (tests/eud_reference.py) on its own: the properties that make it a generalised equivalent
uniform dose, its gradient against central differences, and the convergence of the existing restated optimiser with an EUD term on
the synthetic line plan of the DVH restatement's tests, before any GPU is involved."""
import numpy as np
import pytest

import eud_reference as E
import optimizer_reference as R

U = 2.0 ** -52


def _one_roi(n=300, seed=4, level=2.0):
    """One ROI of n voxels inside a longer volume, doses in [0.2 L, 3 L] (nothing clamped)."""
    rng = np.random.default_rng(seed)
    obj = E.EudReferenceObjective(n + 20)
    roi = obj.add_roi(np.arange(7, 7 + n))
    dose = np.zeros(n + 20, dtype=np.float64)
    dose[7:7 + n] = level * rng.uniform(0.2, 3.0, n)
    return obj, roi, dose, level


def test_mean_and_root_mean_square():
    """a = 1 is the mean and a = 2 the root mean square of an unclamped ROI, to N 2^-52 (the division by L and the product with it
    cost a rounding each, far inside that)."""
    obj, roi, dose, L = _one_roi()
    dv = dose[obj.rois[roi]]
    n = dv.size
    e1, e2 = obj.eud(dose, [(roi, L, 1.0), (roi, L, 2.0)])
    mean, rms = float(np.mean(dv)), float(np.sqrt(np.mean(dv * dv)))
    print("a = 1: %.17g against the mean %.17g; a = 2: %.17g against the rms %.17g; bound %.3g relative" % (e1, mean, e2, rms, n * U))
    assert abs(e1 - mean) <= n * U * mean and abs(e2 - rms) <= n * U * rms


def test_ordering_and_monotony_in_the_exponent():
    """min <= E(a < 0) <= mean <= E(a > 1) <= max, and E does not decrease with a (the power mean inequality)."""
    obj, roi, dose, L = _one_roi()
    dv = dose[obj.rois[roi]]
    exps = [-64.0, -20.0, -10.0, -1.0, -0.0625, 0.0625, 0.5, 1.0, 2.0, 8.0, 16.0, 64.0]
    e = obj.eud(dose, [(roi, L, a) for a in exps])
    slack = 1 + 8 * dv.size * U
    assert np.all(np.diff(e) >= -8 * dv.size * U * e[:-1])
    mean = float(np.mean(dv))
    for a, v in zip(exps, e):
        assert dv.min() / slack <= v <= dv.max() * slack, a
        if a < 0:
            assert v <= mean * slack, a
        if a > 1:
            assert v >= mean / slack, a
    # one voxel alone carries at least 1 / N of the mean of p: E(-64) <= min N^(1/64), E(64) >= max N^(-1/64)
    assert e[0] <= dv.min() * dv.size ** (1 / 64.0) * slack and e[-1] >= dv.max() * dv.size ** (-1 / 64.0) / slack and e[0] < e[3] < e[7] < e[-1]


@pytest.mark.parametrize("kind,a,scale", [(E.SQ_EUD, 1.0, 1.0), (E.SQ_EUD, -10.0, 1.0), (E.SQ_MAX_EUD, 8.0, 0.5), (E.SQ_MIN_EUD, -20.0, 3.0),
                                          (E.SQ_EUD, 0.0625, 1.0), (E.SQ_MAX_EUD, 64.0, 1.0)])
def test_gradient_is_the_directional_derivative(kind, a, scale):
    """A central difference of the value along a random direction, h = 1e-6 L, against <g, delta>: within 1e-6 relative (the
    truncation is of order h^2 with room to spare; not a device number). Doses in [0.2 L, 3 L] and |E - L| >= 0.1 L. The level of the
    one-sided kinds is scaled so that they are violated."""
    obj, roi, dose, L0 = _one_roi(seed=17)
    L = L0 * scale
    if kind == E.SQ_EUD and abs(obj.eud(dose, [(roi, L, a)])[0] - L) < 0.1 * L:
        L = 1.5 * L
    obj.add_eud_term(kind, roi, 3.0, L, a)
    values, g, gabs = obj.eval(dose)
    e = obj.eud(dose, [(roi, L, a)])[0]
    assert abs(e - L) >= 0.1 * L and values[1] > 0 and values[0] == values[1]
    idx = obj.rois[roi]
    assert np.all(dose[idx] >= 0.2 * L0) and np.all(dose[idx] <= 3.0 * L0)
    delta = np.zeros_like(dose)
    delta[idx] = np.random.default_rng(18).uniform(-1.0, 1.0, idx.size)
    h = 1e-6 * L
    fd = (obj.eval(dose + h * delta)[0][0] - obj.eval(dose - h * delta)[0][0]) / (2 * h)
    an = float(np.dot(g, delta))
    print("kind %d, a %g: finite difference %.12g, <g, delta> %.12g, relative difference %.3g" % (kind, a, fd, an, abs(fd - an) / abs(an)))
    assert abs(fd - an) <= 1e-6 * abs(an)
    assert not g[np.setdiff1d(np.arange(dose.size), idx)].any() and np.array_equal(gabs, np.abs(g))


@pytest.mark.parametrize("kind", [E.SQ_MAX_EUD, E.SQ_MIN_EUD])
def test_a_satisfied_one_sided_term_costs_nothing(kind):
    obj, roi, dose, L = _one_roi()
    a = 8.0 if kind == E.SQ_MAX_EUD else -10.0
    e = obj.eud(dose, [(roi, L, a)])[0]
    level = 1.2 * e if kind == E.SQ_MAX_EUD else 0.8 * e
    obj.add_term(R.SQ_DEVIATION, roi, 1.0, L)
    obj.add_eud_term(kind, roi, 2.0, level, a)
    values, g, gabs = obj.eval(dose)
    alone = E.EudReferenceObjective(obj.n_voxels)
    alone.add_roi(obj.rois[roi])
    alone.add_term(R.SQ_DEVIATION, 0, 1.0, L)
    va, ga, _ = alone.eval(dose)
    assert values[2] == 0.0 and values[0] == values[1] == va[0] and np.array_equal(g, ga)
    assert not np.signbit(values[2])
    # the other side of the same level pays
    other = E.EudReferenceObjective(obj.n_voxels)
    other.add_roi(obj.rois[roi])
    other.add_eud_term(E.SQ_MIN_EUD if kind == E.SQ_MAX_EUD else E.SQ_MAX_EUD, 0, 2.0, level, a)
    vo, go, _ = other.eval(dose)
    assert vo[0] > 0 and (np.all(go[obj.rois[roi]] < 0) if kind == E.SQ_MAX_EUD else np.all(go[obj.rois[roi]] > 0))


def test_clamped_voxels_receive_nothing():
    """Zero, negative and tiny doses are clamped to 2^-15 L, huge ones to 2^15 L: they count in E with the clamped value and receive
    a gradient of exactly +0.0, under either sign of the exponent; E stays finite."""
    obj, roi, dose, L = _one_roi()
    idx = obj.rois[roi]
    low, high = idx[[3, 50, 51, 200]], idx[[9, 120]]
    dose[low] = (0.0, -1.0, 2.0 ** -16 * L, -np.inf)
    dose[high] = (2.0 ** 15 * L * (1 + 2.0 ** -40), np.inf)
    on_the_edge = idx[[60, 61]]
    dose[on_the_edge] = (2.0 ** -15 * L, 2.0 ** 15 * L)               # equal to the bounds: not clamped
    for a in (-64.0, -1.0, 0.0625, 2.0, 64.0):
        o = E.EudReferenceObjective(obj.n_voxels)
        o.add_roi(idx)
        o.add_eud_term(E.SQ_EUD, 0, 1.0, L, a)
        values, g, _ = o.eval(dose)
        e = o.eud(dose, [(0, L, a)])[0]
        assert np.isfinite(values[0]) and values[0] > 0 and 2.0 ** -15 * L <= e <= 2.0 ** 15 * L, a
        assert np.all(g[low] == 0.0) and np.all(g[high] == 0.0) and not np.signbit(g[low]).any() and not np.signbit(g[high]).any(), a
        assert np.all(np.isfinite(g)) and not E.clamp(dose[on_the_edge], L)[1].any() and E.clamp(dose[np.concatenate([low, high])], L)[1].all(), a
        want = dose.copy()
        want[low], want[high] = 2.0 ** -15 * L, 2.0 ** 15 * L
        assert e == o.eud(want, [(0, L, a)])[0], a


def test_a_nan_dose_gives_a_nan_value():
    obj, roi, dose, L = _one_roi()
    other = obj.add_roi(np.arange(0, 5))
    dose[obj.rois[roi][11]] = np.nan
    obj.add_eud_term(E.SQ_MAX_EUD, roi, 1.0, 0.5 * L, 8.0)
    obj.add_eud_term(E.SQ_EUD, other, 1.0, L, 2.0)
    values, g, _ = obj.eval(dose)
    assert np.isnan(values[0]) and np.isnan(values[1]) and np.isfinite(values[2])
    e = obj.eud(dose, [(roi, L, 8.0), (other, L, 8.0)])
    assert np.isnan(e[0]) and np.isfinite(e[1])


def _plan(seed):
    """The line problem of the DVH restatement's tests: 4000 voxels, 120 Gaussian columns (sigma 60 to 150 voxels, 1e-6 at the centre,
    float32, entries below 1e-9 zeroed), the target terms of that plan and the overdose term on the body."""
    rng = np.random.default_rng(seed)
    x = np.arange(4000, dtype=np.float64)
    centre, sigma = rng.uniform(0.0, 4000.0, 120), rng.uniform(60.0, 150.0, 120)
    A = (1e-6 * np.exp(-0.5 * ((x[:, None] - centre[None, :]) / sigma[None, :]) ** 2)).astype(np.float32)
    A[A < 1e-9] = 0.0
    P = 2e-5
    obj = E.EudReferenceObjective(4000)
    target, oar, body = obj.add_roi(np.arange(1500, 2500)), obj.add_roi(np.arange(2500, 3300)), obj.add_roi(np.arange(0, 1500))
    obj.add_term(R.SQ_DEVIATION, target, 1.0, P)
    obj.add_dvh_term(E.MIN_DVH, target, 5.0, 0.95 * P, 0.98)
    obj.add_term(R.SQ_OVERDOSE, body, 1.0, 0.5 * P)
    return A.astype(np.float64), obj, P, oar


@pytest.mark.parametrize("seed", range(5))
def test_sixty_iterations_with_a_max_eud_term(seed):
    """Two runs of the restated optimiser from w = 1: the target terms alone, then with SQ_MAX_EUD (a = 8) on the OAR at 0.8 of the
    gEUD the first plan reaches there. The OAR's gEUD at w_best must come out lower with the term than without."""
    A, plain, P, oar = _plan(seed)
    mv, rmv = (lambda w: A @ w.astype(np.float64)), (lambda g: A.T @ g.astype(np.float64))
    first = R.ReferenceOptimizer(plain, mv, rmv, np.ones(A.shape[1])).run(60)
    e_without = float(plain.eud(mv(first.w_best), [(oar, P, 8.0)])[0])
    _, with_term, _, _ = _plan(seed)
    with_term.add_eud_term(E.SQ_MAX_EUD, oar, 3.0, 0.8 * e_without, 8.0)
    second = R.ReferenceOptimizer(with_term, mv, rmv, np.ones(A.shape[1])).run(60)
    e_with = float(with_term.eud(mv(second.w_best), [(oar, P, 8.0)])[0])
    h = np.array(second.history)
    print("seed %d: gEUD(a = 8) of the OAR %.6g without the term, %.6g with it (asked: <= %.6g); f_0 %.6g, f_best %.6g at iteration %d"
          % (seed, e_without, e_with, 0.8 * e_without, h[0], second.f_best, second.best_iteration))
    assert np.all(np.isfinite(h)) and second.guarded == 0 and first.guarded == 0
    assert e_with < e_without
