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
        out.append((r, LB.event_letter(r)))
    return out


def letters(o, n):
    return "".join(e for _, e in events(o, n))


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


def test_event_letters(plan):
    assert LB.event_letter({"k": -1, "reset": True}) == "R" and LB.event_letter({"k": -1, "stall": True}) == "S"
    assert LB.event_letter({"k": -1}) == "." and LB.event_letter({"k": -1, "guard": True}) == "."
    assert [LB.event_letter({"k": k}) for k in range(8)] == list("01234567")
    # ... and on records of step(): a stall, then a backtracked step (test_backtrack_and_stall_paths' run); a guarded start
    o = plan.lbfgs(np.full(COLS, 100.0), memory=8, initial_step=1e3, tree=True)
    r0, r1 = o.step(), o.step()
    assert LB.event_letter(r0) == "S" and LB.event_letter(r1) == str(r1["k"]) and r1["k"] >= 1
    g = plan.lbfgs(np.full(COLS, np.inf), tree=True)
    assert LB.event_letter(g.step()) == "." and g.guarded == 1


def test_set_weights(plan):
    """set_weights is k_lb_forget plus a stale dose: the pairs are dropped and w - w_prev is no pair; the ring head, the stall factor,
    the history, f_best with its iterate and the counters stay. The next iteration is a first-rule step from the new weights'
    product, and the one after it admits a pair at the slot the head pointed to."""
    m = 3
    o = plan.lbfgs(np.zeros(COLS), memory=m, tree=True)
    fresh = np.full(COLS, 3.0)
    o.set_weights(fresh)                                               # before the first iteration: also the best iterate
    assert np.array_equal(o.w, fresh.astype(np.float32)) and np.array_equal(o.w_best, o.w) and o.d0 is None
    o.set_weights(np.zeros(COLS))
    o.run(4)
    assert o.count == 3 and o.moved and o.head == 0
    o.run(1)
    assert o.count == 3 and o.head == 1
    kept = (o.head, o.stall, list(o.history), o.f_best, o.best_iteration, o.w_best.copy(), o.ring.copy(), o.G.copy(),
            (o.guarded, o.unit, o.backtracked, o.halvings, o.resets, o.stalls))
    w_new = (5.0 + 20.0 * np.random.default_rng(3).random(COLS)).astype(np.float32)
    o.set_weights(w_new)
    assert not o.moved and o.count == 0 and o.d0 is None and np.array_equal(o.w, w_new)
    now = (o.head, o.stall, list(o.history), o.f_best, o.best_iteration, o.w_best, o.ring, o.G,
           (o.guarded, o.unit, o.backtracked, o.halvings, o.resets, o.stalls))
    for a, b in zip(kept, now):
        assert np.array_equal(a, b), (a, b)
    r = o.step()
    assert r["f"] == o.value(o.forward(w_new).astype(np.float64)) == o.history[5]
    assert r["pairs"] == 0 and not r["admitted"] and np.all(r["delta"][:2 * m] == 0.0) and r["delta"][2 * m] > 0.0 and o.head == 1
    assert r["k"] >= 0
    r = o.step()
    assert r["admitted"] and r["slot"] == 1 and r["pairs"] == 1 and o.head == 2
    # the stall factor survives it
    s = plan.lbfgs(np.full(COLS, 100.0), memory=8, initial_step=1e3, tree=True)
    assert s.step().get("stall") and s.stall == 2.0 ** -6
    s.set_weights(np.full(COLS, 90.0))
    assert s.stall == 2.0 ** -6 and s.stalls == 1
    assert s.step()["delta"][16] == 1e3 * 2.0 ** -6


def mean_only(plan):
    """A MEAN term over the rows of the matrix, weight 1: the gradient g = A^T (1 / N) does not depend on w. The start is r_j g_j with
    r_j in (0.5, 3.5) and the first scale 1: every accepted step takes g off, so entry j reaches 0 after ceil(r_j) steps."""
    rows = np.flatnonzero(plan.A.any(axis=1))
    p = Problem(plan.A, [(R.MEAN, 0, 1.0, 0.0)], [rows])
    g = p.rmatvec(p.obj.eval(np.zeros(ROWS))[1])
    assert np.all(g > 0.0)
    w0 = ((0.5 + 3.0 * np.random.default_rng(11).random(COLS)) * g).astype(np.float32)
    return p, w0


def test_a_pair_with_y_zero_is_never_admitted(plan):
    p, w0 = mean_only(plan)
    for m in (1, 3):
        o = p.lbfgs(w0, memory=m, initial_step=1.0, tree=True)
        ev = events(o, 8)
        marks = "".join(e for _, e in ev)
        print("MEAN only, m = %d: %s" % (m, marks))
        assert marks == "0000....", marks
        for k, (r, e) in enumerate(ev):
            assert not r["admitted"] and r["pairs"] == 0 and np.all(r["delta"][:2 * m] == 0.0), k
            if k > 0:
                assert not np.any(r["y"]) and r["dots"]["yy"] == 0.0 and (k > 4 or r["dots"]["ss"] > 0.0), k
        assert np.all(o.w == 0.0) and o.resets == 0 and o.stalls == 0 and o.unit == 4
        assert all(r["gp"] == 0.0 and np.array_equal(r["w_full"], np.zeros(COLS, np.float32)) for r, e in ev[4:])


def test_a_zero_gradient_moves_nothing(plan):
    """SQ_OVERDOSE at a level above any dose the start gives: g is +0 everywhere, so grad is +0, the first rule's mx is 0 and its
    scale 1 / mx is taken as 0: w_full is w bit for bit, gp is 0, no counter moves."""
    w0 = (1.0 + np.random.default_rng(13).random(COLS)).astype(np.float32)
    top = float((plan.A.astype(np.float64) @ w0).max())
    p = Problem(plan.A, [(R.SQ_OVERDOSE, 0, 1.0, 2.0 * top)], [np.ones(ROWS, dtype=bool)])
    m = 4
    o = p.lbfgs(w0, memory=m, tree=True)
    for k in range(3):
        r = o.step()
        assert LB.event_letter(r) == "." and r["f"] == 0.0 and r["mx"] == 0.0 and not np.any(r["grad"]) and not np.signbit(r["grad"]).any()
        assert np.all(r["delta"] == 0.0) and r["gp"] == 0.0 and not r["admitted"] and r["pairs"] == 0
        assert np.array_equal(r["w_full"].view(np.uint32), w0.view(np.uint32)) and np.array_equal(o.w.view(np.uint32), w0.view(np.uint32))
    assert (o.guarded, o.unit, o.backtracked, o.halvings, o.resets, o.stalls) == (0,) * 6 and o.stall == 1.0 and not o.moved
    assert o.best_iteration == 0 and o.history == [0.0, 0.0, 0.0]


def test_one_trial_stalls_with_and_without_pairs(plan):
    """max_halvings = 0 (K = 1: the full step or nothing). A stall with pairs held drops them and leaves the stall factor alone; a
    stall without pairs halves it (2^-K). m = 3 from w = 0 stalls at iterations 25 (3 pairs) and 26 (none); m = 16 from w = 100 at
    iteration 2 (one pair)."""
    o = plan.lbfgs(np.zeros(COLS), memory=3, max_halvings=0, tree=True)
    ev, ws = [], []
    for _ in range(28):
        ws.append(o.w.copy())
        ev += events(o, 1)
    marks = "".join(e for _, e in ev)
    assert marks == "0" * 25 + "SS0", marks
    a, b = ev[25][0], ev[26][0]
    assert a["pairs"] == 3 and a["stall_factor"] == 1.0 and len(a["F"]) == 1
    assert b["pairs"] == 0 and not b["admitted"] and b["stall_factor"] == 1.0 and np.all(b["delta"][:6] == 0.0)
    assert ev[27][0]["stall_factor"] == 0.5 and ev[27][0]["pairs"] == 0 and o.stalls == 2 and o.stall == 1.0
    assert o.history[25] == o.history[26] == o.history[27] and np.array_equal(ws[25], ws[26]) and np.array_equal(ws[26], ws[27])
    assert not np.array_equal(ws[24], ws[25]) and not np.array_equal(ws[27], o.w)
    assert o.halvings == 0 and o.backtracked == 0 and o.unit == 26
    o = plan.lbfgs(np.full(COLS, 100.0), memory=16, max_halvings=0, tree=True)
    ev = events(o, 4)
    marks = "".join(e for _, e in ev)
    assert marks == "00S0", marks
    assert ev[2][0]["pairs"] == 2 and ev[2][0]["admitted"] and o.stalls == 1 and ev[3][0]["pairs"] == 0 and ev[3][0]["stall_factor"] == 1.0


def test_the_last_trial_is_reached_for_every_trial_count(plan):
    """From w = 0 the first scale is the first rule's times 2^j, j = 0, 1, ... until the first iteration accepts its last trial K - 1:
    one more doubling per halving, j = 9 + (K - 2) on this problem for K = 2 .. 8."""
    first = plan.lbfgs(np.zeros(COLS), tree=True).step()["delta"][-1]
    for K in range(2, 9):
        found = None
        for j in range(40):
            o = plan.lbfgs(np.zeros(COLS), memory=3, max_halvings=K - 1, initial_step=first * 2.0 ** j, tree=True)
            r = o.step()
            if r["k"] == K - 1:
                found = j
                break
        assert found == 9 + (K - 2), (K, found)
        assert len(r["F"]) == K and r["a"] == 2.0 ** -(K - 1) and o.halvings == K - 1 and o.backtracked == 1
        assert all(not f <= r["f"] + (o.c1 * 2.0 ** -k) * r["gp"] for k, f in enumerate(r["F"][:K - 1]))
        marks = LB.event_letter(r) + letters(o, 4)
        assert marks[0] == str(K - 1) and "S" not in marks and "R" not in marks, marks
