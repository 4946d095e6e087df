"""The numpy restatement of the robust iteration (include/rtd.h "Robust spot-weight optimisation"): what one
launch decides between the per-scenario objective values (decide), how the per-scenario spot gradients become one (combine), and the
whole iteration on S pairs of callables (RobustReferenceOptimizer). A test helper, not product code.

Steps 4-7 of the plain iteration are those of optimizer_reference.ReferenceOptimizer.advance, fed F_k and the combined gradient."""
import numpy as np

import optimizer_reference as R

EXPECTED, WORST_CASE = 0, 1


def decide(values, mode, probabilities=None):
    """Step 3 -> (lambdas float64[S], F, worst). EXPECTED: lambda = p (1 / S each without), F = sum_s p_s f_s from 0.0 in ascending s,
    every product rounded before it is added. WORST_CASE: the lowest index holding the maximum, lambda one-hot, F = that value.
    A value that is not finite: the lowest such index is `worst` and its value F, in either mode."""
    f = np.asarray(values, dtype=np.float64).reshape(-1)
    S = f.size
    p = np.full(S, 1.0 / S) if probabilities is None else np.asarray(probabilities, dtype=np.float64).reshape(-1)
    assert p.size == S and S >= 1
    worst, F = 0, 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(S):
            if s == 0 or f[s] > f[worst]:
                worst = s
            F = F + p[s] * f[s]
    bad = np.flatnonzero(~np.isfinite(f))
    if bad.size:
        worst = int(bad[0])
    if mode == WORST_CASE or bad.size:
        F = float(f[worst])
    lam = p.copy() if mode == EXPECTED else np.where(np.arange(S) == worst, 1.0, 0.0)
    return lam, float(F), int(worst)


def combine(grads, lambdas, ft=np.float32):
    """Step 5: ft(sum over the scenarios with lambda != 0, ascending, of lambda_s * float64(grad_s)), the sum STARTING from the first
    product (so that one scenario with lambda 1.0 hands its bits through, a -0 included). grads: [S][n] (rows of scenarios with
    lambda == 0 are not read)."""
    acc = None
    with np.errstate(over="ignore", invalid="ignore"):
        for s, l in enumerate(np.asarray(lambdas, dtype=np.float64)):
            if l == 0.0:
                continue
            prod = l * np.asarray(grads[s]).reshape(-1).astype(np.float64)
            acc = prod if acc is None else acc + prod
    assert acc is not None
    return acc.astype(ft)


class RobustReferenceOptimizer(R.ReferenceOptimizer):
    """matvecs / rmatvecs: one pair of callables per scenario. scenario_values / lambdas / worst belong to the iterate that entered
    the last step, as on the device."""

    def __init__(self, objective, matvecs, rmatvecs, w0, mode, probabilities=None, **kw):
        super().__init__(objective, None, None, w0, **kw)
        self.matvecs, self.rmatvecs = list(matvecs), list(rmatvecs)
        self.mode, self.prob = mode, probabilities
        self.scenario_values = self.lambdas = None
        self.worst = 0

    def evaluate(self, w):
        """f_s of every scenario at w (float64 array)."""
        return np.array([float(self.obj.eval(mv(w))[0][0]) for mv in self.matvecs])

    def step(self, values=None, grads=None):
        """One iteration; values [S] and grads [S][n] replace the per-scenario evaluations and transposed products when given."""
        if values is None:
            values, grads = [], []
            for mv, rmv in zip(self.matvecs, self.rmatvecs):
                v, g, _ = self.obj.eval(mv(self.w))
                values.append(float(v[0]))
                with np.errstate(over="ignore", invalid="ignore"):
                    grads.append(np.asarray(rmv(g.astype(self.ft))).astype(self.ft))
        self.scenario_values = np.asarray(values, dtype=np.float64)
        self.lambdas, F, self.worst = decide(values, self.mode, self.prob)
        return self.advance(F, combine(grads, self.lambdas, self.ft))


def line_plan(seed, shift=0.0, stretch=1.0):
    """The 1-D problem of tests/test_dvh_reference.py (4000 voxels on a line, 120 Gaussian columns, sigma 60 to 150 voxels, 1e-6 at the
    centre, float32, entries below 1e-9 zeroed) under an error: the columns displaced by `shift` voxels and their depth axis stretched
    by `stretch` (a column centred at c lands at c / stretch + shift, its width scales alike). -> float64 matrix [4000][120]."""
    rng = np.random.default_rng(seed)
    x = np.arange(4000, dtype=np.float64)
    centre, sigma = rng.uniform(0.0, 4000.0, 120), rng.uniform(60.0, 150.0, 120)
    xs = (x - shift) * stretch
    A = (1e-6 * np.exp(-0.5 * ((xs[:, None] - centre[None, :]) / sigma[None, :]) ** 2)).astype(np.float32)
    A[A < 1e-9] = 0.0
    return A.astype(np.float64)


def _wave_sum(v):
    """The butterfly of a wave of 64 (lane distances 32, ..., 1) in float64; every lane ends with the same sum, lane 0's is returned."""
    v = np.asarray(v, dtype=np.float64).copy()
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[idx ^ m]
    return float(v[0])


def tree_sum(x, chunk=2048):
    """The fixed tree of step 5 of the plain iteration: chunks of 2048 entries, lane t adds the entries t, t + 64, ... in order,
    butterfly; the chunk sums are added the same way (chunk c to lane c mod 64)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)

    def lanes(a):
        acc = np.zeros(64)
        for i in range(0, a.size, 64):
            part = a[i:i + 64]
            acc[:part.size] = acc[:part.size] + part
        return _wave_sum(acc)
    return lanes(np.array([lanes(x[a:a + chunk]) for a in range(0, x.size, chunk)]))


def step_length_tree(w, w_prev, grad, grad_prev, have_bb, step_min=1e-30, step_max=1e30):
    """optimizer_reference.step_length with the two dot products summed in the device's order: the same bits, not only the same
    value within a summation bound."""
    if not have_bb:
        return R.step_length(w, w_prev, grad, grad_prev, False, step_min, step_max)
    w, grad = np.asarray(w, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    s = w - np.asarray(w_prev, dtype=np.float64)
    y = grad - np.asarray(grad_prev, dtype=np.float64)
    ss, sy = tree_sum(s * s), tree_sum(s * y)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        a = ss / sy if sy > 0.0 else step_max
    if not a >= step_min:
        a = step_min
    return step_max if a > step_max else a
