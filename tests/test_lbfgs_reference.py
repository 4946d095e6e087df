"""CPU checks of the restatement of the L-BFGS iteration (tests/lbfgs_reference.py, written from include/rtd.h) on synthetic
non-negative sparse matrices: no GPU needed. What the GPU tests take for granted of the restatement is checked here: the
coefficient-space recursion is the textbook two-loop, accepted steps never raise the objective, the iteration finds the optimum of a
bound-constrained least-squares problem, the ring wraps, and the reset, stall and backtrack paths are all taken."""
import numpy as np
import pytest

import lbfgs_reference as LB
import optimizer_reference as R

U64 = 2.0 ** -53
ROWS, COLS = 4000, 300


def banded(seed=2, rows=ROWS, cols=COLS, width=40):
    """Column j is a noisy bell of `width` rows around row rows (j + 0.5) / cols: neighbouring columns overlap heavily, as the dose
    columns of neighbouring spots do. Non-negative float32, sparse (6 widths of rows per column), held dense."""
    rng = np.random.default_rng(seed)
    A = np.zeros((rows, cols), dtype=np.float32)
    for j in range(cols):
        c = int(rows * (j + 0.5) / cols)
        r = np.arange(max(0, c - 3 * width), min(rows, c + 3 * width))
        v = np.exp(-0.5 * ((r - c) / width) ** 2) * (0.5 + rng.random(r.size))
        A[r, j] = np.where(v > 1e-3, v, 0.0)
    return A


class Problem:
    def __init__(self, A, terms, rois):
        self.A = A
        self.obj = R.ReferenceObjective(A.shape[0])
        for m in rois:
            self.obj.add_roi(m)
        for t in terms:
            self.obj.add_term(*t)
        A64 = A.astype(np.float64)
        self.matvec = lambda w: A64 @ np.asarray(w, dtype=np.float64)
        self.rmatvec = lambda g: A64.T @ np.asarray(g, dtype=np.float64)

    def lbfgs(self, w0, **kw):
        return LB.LbfgsReference(self.obj, self.matvec, self.rmatvec, w0, **kw)


@pytest.fixture(scope="module")
def plan():
    """The four term kinds on the banded matrix: a target in the middle (SQ_DEVIATION + SQ_UNDERDOSE), the rest SQ_OVERDOSE + MEAN."""
    A = banded()
    w_true = (40.0 + 120.0 * np.random.default_rng(7).random(COLS)).astype(np.float32)
    w_true[:COLS // 4] *= 0.1
    w_true[COLS * 13 // 20:] *= 0.1
    x = np.arange(ROWS)
    target = (x > 0.3 * ROWS) & (x < 0.6 * ROWS)
    level = float((A @ w_true)[target].mean())
    terms = [(R.SQ_DEVIATION, 0, 1.0, level), (R.SQ_UNDERDOSE, 0, 5.0, 0.95 * level), (R.SQ_OVERDOSE, 1, 1.0, 0.3 * level),
             (R.MEAN, 1, 1e-3 * level, 0.0)]
    return Problem(A, terms, [target, ~target])


def events(o, n):
    out = []
    for _ in range(n):
        r = o.step()
        out.append((r, "R" if r.get("reset") else "S" if r.get("stall") else "." if r["k"] < 0 else str(r["k"])))
    return out


def two_loop_bound(pairs, ghat, m):
    """A float64 bound on the max-norm distance of two evaluations of r = H ghat (any two orders of the sums, on vectors or on
    coefficients over the Gram matrix).

    H is a product of 2 c operators I - rho_i s_i y_i^T (and transposes) and one scaling gamma, c the pairs held. Each operator has
    2-norm at most a_i = 1 + |s_i| |y_i| / <s_i, y_i>. One step evaluates one inner product of n terms, whose computed value is off by
    at most (n + 2) u |a| |b| in any order of summation (and its denominator <s_i, y_i> by the same relative to |s_i| |y_i|), so the
    vector it adds is off by at most (n + 2) u a_i^2 times the norm of what entered the step; the coefficient form sums at most 2m + 1
    such products per inner product instead (factor 2m + 1, n + 2m + 3 terms). What entered a step is at most amp |ghat| gamma, amp =
    prod a_i^2, and what a step leaves is amplified by at most amp by the steps behind it. Two evaluations, 2 c steps each:
        |r - r'| <= 2 * 2c * (2m + 1) * (n + 2m + 3) u * amp * max a_i^2 * gamma |ghat|   (first order; the factor 2 in front of 2c
    leaves room for the second-order terms at these sizes: n u is 1e-13)."""
    a = [1.0 + np.linalg.norm(s) * np.linalg.norm(y) / float(np.dot(s, y)) for s, y in pairs]
    amp = float(np.prod(np.square(a)))
    s, y = pairs[0]
    gamma = float(np.dot(s, y)) / float(np.dot(y, y))
    n = ghat.size
    return 4.0 * len(pairs) * (2 * m + 1) * (n + 2 * m + 3) * U64 * amp * max(a) ** 2 * gamma * float(np.linalg.norm(ghat))


@pytest.mark.parametrize("tree", [False, True])
def test_coefficient_direction_is_the_vector_two_loop(plan, tree):
    m = 3
    o = plan.lbfgs(np.zeros(COLS), memory=m, tree=tree)
    checked, worst = 0, 0.0
    for _ in range(12):
        r = o.step()
        if not r.get("pairs"):
            continue
        ring = o.ring.astype(np.float64)
        pairs = [(ring[i], ring[m + i]) for i in r["order"]]
        ghat = r["ghat"].astype(np.float64)
        r_coef = r["delta"][2 * m] * ghat
        for i in range(2 * m):
            r_coef = r_coef + r["delta"][i] * ring[i]
        r_vec = LB.two_loop_vectors(pairs, ghat)
        err, bound = float(np.max(np.abs(r_coef - r_vec))), two_loop_bound(pairs, ghat, m)
        worst = max(worst, err / bound)
        assert err <= bound, (err, bound)
        assert float(np.linalg.norm(r_vec)) > 1e3 * bound, "the bound says nothing at this size"
        checked += 1
    print("two-loop: %d directions, worst error / bound %.3g" % (checked, worst))
    assert checked >= 10


def test_history_is_non_increasing(plan):
    """Plain float64: f_{k+1} is the accepted F_k itself, so no accepted step raises it at all. Tree order with float32 storage: after a
    unit step the same holds bit for bit (d0 = d1); after a backtracked step d0 is the mixed dose rounded once to float32."""
    for start, kw in ((0.0, dict(memory=8)), (100.0, dict(memory=8, initial_step=1e3)), (100.0, dict(memory=16, max_halvings=2))):
        o = plan.lbfgs(np.full(COLS, start), tree=False, **kw)
        o.run(40)
        h = np.array(o.history)
        assert np.all(np.diff(h) <= 0.0), (kw, h)
        assert o.f_best == h.min() and o.best_iteration == int(np.argmin(h))
        t = plan.lbfgs(np.full(COLS, start), tree=True, **kw)
        n_back = 0
        for k in range(40):
            r = t.step()
            f_now, f_next = t.history[k], t.value(t.d0.astype(np.float64))      # (f_next: what the next iteration will record)
            if r["k"] == 0:
                assert f_next == r["F"][0] and f_next <= f_now, (k, f_now, f_next)
            elif r["k"] > 0:
                n_back += 1
                assert r["f_trial"] <= f_now and f_next <= r["f_trial"] + LB.rounding_rise_bound(plan.obj, t.d0), (k, f_now, f_next, r["f_trial"])
            else:
                assert f_next == f_now, (k, r)
        assert n_back >= 1 or start == 0.0


def test_bound_constrained_least_squares_reaches_the_projected_gradient_optimum():
    """f(w) = sum_t w_t / N_t |A_t w - L_t|^2 over w >= 0 (two SQ_DEVIATION terms: a level in the middle, zero outside, so that bounds
    are active at the optimum). A long projected-gradient run with step 1 / L ends at w_pg with natural residual r = w_pg - P(w_pg -
    grad). The tolerance is that run's own: f is mu-strongly convex and L-smooth (mu, L the extreme eigenvalues of the Hessian), so
    |w_pg - w*| <= d = (1 + L) / mu |r| (the error bound of the natural residual for a strongly monotone, Lipschitz map), and
    f(w_pg) - f* <= |grad(w_pg)| d + L / 2 d^2 = eps. Since f* <= f_lbfgs, L-BFGS has reached the optimum as far as that run can
    tell iff f_lbfgs <= f(w_pg) + eps."""
    A = banded(seed=5, cols=120, rows=1600, width=16)
    rows, cols = A.shape
    x = np.arange(rows)
    target = (x > 0.3 * rows) & (x < 0.6 * rows)
    level = 60.0
    p = Problem(A, [(R.SQ_DEVIATION, 0, 1.0, level), (R.SQ_DEVIATION, 1, 2.0, 0.0)], [target, ~target])
    A64 = A.astype(np.float64)
    scale = np.where(target, 2.0 * 1.0 / target.sum(), 2.0 * 2.0 / (~target).sum())
    H = A64.T @ (scale[:, None] * A64)
    ev = np.linalg.eigvalsh(H)
    mu, L = float(ev[0]), float(ev[-1])
    assert mu > 0.0

    def fg(w):
        values, g, _ = p.obj.eval(p.matvec(w))
        return float(values[0]), p.rmatvec(g)
    w = np.zeros(cols)
    for _ in range(10000):
        w = R.project(w - fg(w)[1] / L)
    f_pg, g_pg = fg(w)
    res = float(np.linalg.norm(w - R.project(w - g_pg)))
    d = (1.0 + L) / mu * res
    eps = float(np.linalg.norm(g_pg)) * d + 0.5 * L * d * d
    o = p.lbfgs(np.zeros(cols), memory=8, tree=False)
    o.run(300)
    print("least squares: f_pg %.12g residual %.3g eps %.3g; f_lbfgs %.12g after 300, active bounds %d of %d, mu %.3g L %.3g"
          % (f_pg, res, eps, o.f_best, int((o.w == 0).sum()), cols, mu, L))
    assert int((w == 0).sum()) > 0, "no bound is active at the optimum: the problem does not test the projection"
    assert eps < 1e-3 * f_pg, "the projected-gradient run has not converged far enough to say anything"
    assert o.f_best <= f_pg + eps, (o.f_best, f_pg, eps)
    assert np.all(o.w >= 0.0) and np.all(np.isfinite(o.w))


def test_the_ring_wraps(plan):
    m = 3
    o = plan.lbfgs(np.zeros(COLS), memory=m, tree=True)
    slots = []
    for _ in range(12):
        r = o.step()
        if r["admitted"]:
            slots.append(r["slot"])
            assert np.array_equal(o.ring[r["slot"]], r["s"]) and np.array_equal(o.ring[m + r["slot"]], r["y"])
            assert o.G[r["slot"], m + r["slot"]] == r["dots"]["sy"] and o.G[m + r["slot"], m + r["slot"]] == r["dots"]["yy"]
            assert r["order"][0] == r["slot"]
    assert len(slots) > 2 * m and slots[:7] == [0, 1, 2, 0, 1, 2, 0], slots
    assert o.count == m
    assert np.array_equal(o.G, o.G.T)


def test_backtrack_and_stall_paths(plan):
    """A start of 100 per spot and a first scale of 1e3 overshoots: the first iteration (no pairs) accepts none of its K trial steps
    (a stall: nothing moves, gamma0 shrinks by 2^-K), the second backtracks."""
    K = 6
    o = plan.lbfgs(np.full(COLS, 100.0), memory=8, initial_step=1e3, tree=True)
    w0, d_before = o.w.copy(), None
    r0 = o.step()
    assert r0.get("stall") and r0["k"] == -1 and o.stalls == 1 and np.array_equal(o.w, w0) and o.stall == 2.0 ** -K
    d_before = o.d0.copy()
    assert r0["delta"][16] == 1e3
    r1 = o.step()
    assert r1["delta"][16] == 1e3 * 2.0 ** -K and not r1["admitted"]
    assert r1["k"] >= 1 and o.backtracked == 1 and o.halvings == r1["k"] and o.stall == 1.0
    assert not np.array_equal(o.w, w0) and not np.array_equal(o.d0, d_before)
    assert o.history[1] == o.history[0]
    r2 = o.step()
    assert r2["admitted"] and o.history[2] < o.history[1]


def test_reset_path():
    """A tiny dense problem (6 voxels, 4 spots, found by search) on which the projected quasi-Newton direction stops being a descent
    direction with pairs held: the memory is dropped, nothing moves, and the next iteration is a projected steepest-descent step."""
    rng = np.random.default_rng(12)
    cols, rows = int(rng.integers(2, 6)), 0
    rows = int(rng.integers(cols, 12))
    A = (rng.random((rows, cols)) ** 3).astype(np.float32)
    b = A @ (rng.random(cols) * (rng.random(cols) > 0.5)) * 10
    p = Problem(A, [(R.SQ_DEVIATION, 0, 1.0, float(b.mean()) + 1e-3), (R.MEAN, 0, 0.5, 0.0)], [np.ones(rows, dtype=bool)])
    w0 = rng.random(cols) * 10 ** rng.uniform(-3, 2, cols)
    o = p.lbfgs(w0, memory=3, tree=True)
    ev = events(o, 12)
    marks = "".join(e for _, e in ev)
    assert "R" in marks, marks
    k = marks.index("R")
    r = ev[k][0]
    assert r["pairs"] > 0 and not r["gp"] < 0.0 and o.resets >= 1
    nxt = ev[k + 1][0]
    assert nxt["pairs"] == 0 and not nxt["admitted"] and np.all(nxt["delta"][:6] == 0.0) and nxt["delta"][6] > 0.0
    assert o.history[k + 1] == o.history[k]
    assert nxt["k"] >= 0 and o.history[k + 2] < o.history[k + 1], marks
