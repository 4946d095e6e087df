"""The numpy restatement of the voxel-wise worst case (tests/voxelwise_reference.py) on its own: the corner cases of the extremes,
one scenario against the plain restatement, the composite against every scenario's own objective, the combined gradient against finite
differences, and on the 1-D plan of tests/robust_reference.py under shifts and stretches that the voxel-wise plan beats both the
nominal plan and the scenario-wise WORST_CASE plan on the composite objective."""
import numpy as np
import pytest

import optimizer_reference as R
import robust_reference as Q
import voxelwise_reference as V


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_extremes_corner_cases():
    nan_a, nan_b = np.uint32(0x7FC00123).view(np.float32), np.uint32(0xFFC00456).view(np.float32)
    d = np.float32([[1.0, 4.0, -0.0, 0.0, 2.0, 5.0, nan_b],
                    [3.0, 4.0, 0.0, -0.0, nan_a, 5.0, nan_a],
                    [3.0, 1.0, -0.0, 0.0, nan_b, 5.0, 9.0],
                    [2.0, 4.0, 0.0, 0.0, 7.0, 5.0, -9.0]])
    lo, s_lo, hi, s_hi = V.extremes(d)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    # a tie goes to the lower index
    assert (hi[0], s_hi[0], lo[0], s_lo[0]) == (3.0, 1, 1.0, 0)
    assert (hi[1], s_hi[1], lo[1], s_lo[1]) == (4.0, 0, 1.0, 2)
    assert (s_hi[5], s_lo[5]) == (0, 0)
    # -0 against +0: equal, so the lower index, with its own sign
    assert s_hi[2] == 0 and s_lo[2] == 0 and np.signbit(hi[2]) and np.signbit(lo[2])
    assert s_hi[3] == 0 and s_lo[3] == 0 and not np.signbit(hi[3]) and not np.signbit(lo[3])
    # one NaN: both extremes are that NaN, both indices that scenario; several: the lowest scenario's
    assert s_hi[4] == 1 and s_lo[4] == 1 and _bits(hi[4:5])[0] == 0x7FC00123 and _bits(lo[4:5])[0] == 0x7FC00123
    assert s_hi[6] == 0 and s_lo[6] == 0 and _bits(hi[6:7])[0] == 0xFFC00456 and _bits(lo[6:7])[0] == 0xFFC00456
    # S = 1: the volume itself
    lo, s_lo, hi, s_hi = V.extremes(d[1:2])
    assert np.array_equal(_bits(lo), _bits(d[1])) and np.array_equal(_bits(hi), _bits(d[1])) and not s_lo.any() and not s_hi.any()


def _small_objective(n=60):
    obj = R.ReferenceObjective(n)
    a, b = obj.add_roi(np.arange(10, 40)), obj.add_roi(np.arange(30, 60))
    obj.add_term(R.SQ_DEVIATION, a, 1.0, 2.0)
    obj.add_term(R.SQ_UNDERDOSE, a, 5.0, 1.9)
    obj.add_term(R.SQ_OVERDOSE, b, 2.0, 0.5)
    obj.add_term(R.MEAN, b, 0.1)
    return obj


def test_one_scenario_is_the_plain_restatement():
    rng = np.random.default_rng(5)
    obj = _small_objective()
    dose = (3.0 * rng.random(60)).astype(np.float32)
    dose[12] = np.nan
    values, G, active, _ = V.eval_voxelwise(obj, dose[None, :])
    rv, rg, _ = obj.eval(dose)
    assert np.array_equal(_bits(values), _bits(rv)) and np.array_equal(_bits(G[0]), _bits(rg)) and active == 1
    A = rng.random((60, 12))
    mv, rmv = (lambda w: A @ w.astype(np.float64)), (lambda g: A.T @ g.astype(np.float64))
    plain = R.ReferenceOptimizer(obj, mv, rmv, np.ones(12)).run(15)
    one = V.VoxelwiseReferenceOptimizer(obj, [mv], [rmv], np.ones(12)).run(15)
    assert np.array_equal(_bits(np.array(one.history)), _bits(np.array(plain.history)))
    assert np.array_equal(_bits(one.w), _bits(plain.w)) and np.array_equal(_bits(one.w_best), _bits(plain.w_best))
    assert one.worst == 0 and list(one.lambdas) == [1.0] and one.scenario_values[0] == one.history[-1]


def test_gradient_goes_to_the_scenario_that_holds_the_extreme():
    """Two voxels, three scenarios, by hand: OVERDOSE follows the maximum, UNDERDOSE the minimum, DEVIATION the one further from its
    level; one sum when one scenario holds both extremes; a scenario that holds neither gets +0 and no bit."""
    obj = R.ReferenceObjective(3)
    r = obj.add_roi(np.arange(2))
    obj.add_term(R.SQ_OVERDOSE, r, 1.0, 1.0)
    obj.add_term(R.SQ_UNDERDOSE, r, 1.0, 3.0)
    obj.add_term(R.SQ_DEVIATION, r, 1.0, 2.5)
    d = np.float32([[2.0, 4.0, 7.0], [5.0, 4.0, 7.0], [3.0, 4.0, 7.0]])
    values, G, active, _ = V.eval_voxelwise(obj, d)
    # voxel 0: hi 5 (s 1), lo 2 (s 0); DEVIATION: |5 - 2.5| >= |2 - 2.5| -> hi. voxel 1: all 4 -> one sum at s 0.
    assert G[1][0] == (0.0 + 1.0 * (5.0 - 1.0)) + 1.0 * (5.0 - 2.5) and G[0][0] == 0.0 + 1.0 * (2.0 - 3.0) and G[2][0] == 0.0
    assert G[0][1] == ((0.0 + 1.0 * (4.0 - 1.0)) + 1.0 * 0.0) + 1.0 * (4.0 - 2.5) and G[1][1] == 0.0 and G[2][1] == 0.0
    assert not G[:, 2].any() and active == 0b011
    assert values[1] == 0.5 * (16.0 + 9.0) and values[2] == 0.5 * 1.0 and values[3] == 0.5 * (6.25 + 2.25)


def test_composite_dominates_every_scenario():
    """phi of every term is largest at the extreme the term sees, voxel by voxel, so F >= f_s up to the summation bound N 2^-52."""
    rng = np.random.default_rng(3)
    obj = _small_objective()
    for S in (2, 5, 32):
        d = (3.0 * rng.random((S, 60))).astype(np.float32)
        F = V.eval_voxelwise(obj, d)[0][0]
        fs = np.array([obj.eval(d[s])[0][0] for s in range(S)])
        print("S %d: F %.9g, max_s f_s %.9g" % (S, F, fs.max()))
        assert np.all(F >= fs * (1.0 - 60 * 2.0 ** -52)) and F > fs.max()


def test_composite_gradient_is_the_derivative():
    """A small dense problem, three scenarios, float64 throughout: central differences of F(w) against the combined gradient, within
    1e-6 of its largest entry, h = 1e-5 (the bound of test_expected_gradient_is_the_derivative). The composite is only piecewise
    smooth: the weights are drawn until no two scenarios lie within 1e-3 of each other at a voxel and no dose within 10 h of a level
    or of the point where a DEVIATION term changes sides (the moves of a dose under h are below 10 h: the rows sum to less than 10)."""
    n, m, h = 80, 10, 1e-5
    obj = R.ReferenceObjective(n)
    a, b = obj.add_roi(np.arange(0, 50)), obj.add_roi(np.arange(40, 80))
    obj.add_term(R.SQ_DEVIATION, a, 1.0, 3.0)
    obj.add_term(R.SQ_UNDERDOSE, a, 5.0, 2.8)
    obj.add_term(R.SQ_OVERDOSE, b, 2.0, 2.0)
    obj.add_term(R.MEAN, b, 0.1)
    levels = (3.0, 2.8, 2.0)
    for seed in range(9, 200):
        rng = np.random.default_rng(seed)
        As = [rng.random((n, m)) for _ in range(3)]
        w = rng.random(m)
        d = np.stack([A @ w for A in As])
        gaps = min(np.abs(d[i] - d[j]).min() for i in range(3) for j in range(i))
        near = min(np.abs(d - lv).min() for lv in levels)
        sides = np.abs(np.abs(d.max(axis=0) - 3.0) - np.abs(d.min(axis=0) - 3.0)).min()
        if gaps > 1e-3 and near > 10 * h and sides > 40 * h:
            break
    else:
        raise AssertionError("no draw keeps clear of the kinks")
    F = lambda x: V.eval_voxelwise(obj, np.stack([A @ x for A in As]))[0][0]   # noqa: E731
    _, G, active, _ = V.eval_voxelwise(obj, d)
    assert active == 0b111
    grad = V.combine([A.T @ G[s] for s, A in enumerate(As)], [1.0, 1.0, 1.0], m, np.float64)
    for j in range(m):
        e = np.zeros(m)
        e[j] = h
        fd = (F(w + e) - F(w - e)) / (2 * h)
        assert abs(fd - grad[j]) <= 1e-6 * np.abs(grad).max(), (j, fd, grad[j])


SHIFT, STRETCH, ITERATIONS = 80.0, 1.035, 100


def _line_objective():
    """The objective of tests/test_robust_reference.py with its DVH terms replaced by SQ_UNDERDOSE at 0.95 P on the target and
    SQ_OVERDOSE at 0.3 P on the OAR."""
    P = 2e-5
    obj = R.ReferenceObjective(4000)
    target, oar, body = obj.add_roi(np.arange(1500, 2500)), obj.add_roi(np.arange(2500, 3300)), obj.add_roi(np.arange(0, 1500))
    obj.add_term(R.SQ_DEVIATION, target, 1.0, P)
    obj.add_term(R.SQ_UNDERDOSE, target, 5.0, 0.95 * P)
    obj.add_term(R.SQ_OVERDOSE, oar, 3.0, 0.3 * P)
    obj.add_term(R.SQ_OVERDOSE, body, 1.0, 0.5 * P)
    return obj


@pytest.mark.parametrize("seed", range(5))
def test_the_voxelwise_plan_is_ahead_on_the_composite(seed):
    """The 1-D plan of robust_reference.line_plan; five scenarios: nominal, the columns displaced by +-80 voxels, the depth axis
    stretched by 1 / 1.035 and 1.035. A hundred iterations from w = 1 of the plain restatement on the nominal matrix, of the
    scenario-wise WORST_CASE one and of the voxel-wise one: the voxel-wise plan's composite objective at w_best lies below the nominal
    plan's and below the WORST_CASE plan's, no guard is taken, and the composite is at least every scenario's own value. The ratios
    are printed (DESIGN.md section 15 records them)."""
    As = [Q.line_plan(seed)] + [Q.line_plan(seed, shift=s) for s in (SHIFT, -SHIFT)] + [Q.line_plan(seed, stretch=t) for t in (1.0 / STRETCH, STRETCH)]
    obj = _line_objective()
    mv = [(lambda w, A=A: A @ w.astype(np.float64)) for A in As]
    rmv = [(lambda g, A=A: A.T @ g.astype(np.float64)) for A in As]
    n = As[0].shape[1]
    nominal = R.ReferenceOptimizer(obj, mv[0], rmv[0], np.ones(n)).run(ITERATIONS)
    worst = Q.RobustReferenceOptimizer(obj, mv, rmv, np.ones(n), Q.WORST_CASE).run(ITERATIONS)
    vox = V.VoxelwiseReferenceOptimizer(obj, mv, rmv, np.ones(n)).run(ITERATIONS)
    c_nom, c_worst, c_vox = vox.composite(nominal.w_best), vox.composite(worst.w_best), vox.composite(vox.w_best)
    print("seed %d: composite objective %.6g (nominal plan), %.6g (WORST_CASE plan), %.6g (voxel-wise plan): ratios to the nominal plan %.3f and %.3f"
          % (seed, c_nom, c_worst, c_vox, c_worst / c_nom, c_vox / c_nom))
    assert vox.guarded == 0 and np.all(np.isfinite(vox.history)) and c_vox == vox.f_best
    assert c_vox / c_nom < 1.0 and c_vox < c_worst
    for w in (nominal.w_best, worst.w_best, vox.w_best):
        assert np.all(vox.composite(w) >= worst.evaluate(w) * (1.0 - 4000 * 2.0 ** -52))
