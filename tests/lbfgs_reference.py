"""The numpy restatement of the L-BFGS iteration of rtd_optimizer_create_lbfgs, written from the text of include/rtd.h ("L-BFGS with a
line search on the device", steps 1 to 7). A test helper, not product code.

Two variants of one skeleton:
  tree=True   float32 storage where the device stores float32, and every sum in the device's order: the chunk tree of step 4 (chunks
              of 2048 entries, lane t adds the entries t, t + 64, ... from +0.0, butterfly 32 ... 1, the chunk sums the same way), the
              evaluation's tree for F_k (one thread per union voxel, blocks of 256, wave butterfly, (w0 + w1) + (w2 + w3), block b to
              lane b mod 64, butterfly, times wn_t, the terms in term order), index order over the Gram matrix. Its bits can be
              compared with the device's.
  tree=False  the same iteration in plain float64 (numpy sums), vectors kept in float64.
The two products come from callables (matvec: weights -> flat dose, rmatvec: flat voxel gradient -> spot gradient); step() also takes
the device's own d0, d1 and grad, so that everything between the products is compared."""
import numpy as np

import optimizer_reference as R

CHUNK = 2048


def _butterfly(v):
    """v [rows, 64] float64: every lane adds the lane at distance 32, ..., 1 (xor); lane 0's sum per row."""
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[:, idx ^ m]
    return v[:, 0]


def _lane_sums(x):
    """x [rows, length] float64, length a multiple of 64: lane t's sequential sum of the entries t, t + 64, ... from +0.0."""
    rows, length = x.shape
    acc = np.zeros((rows, 64))
    for i in range(length // 64):
        acc = acc + x[:, 64 * i:64 * i + 64]
    return acc


def _pad(x, mult):
    n = x.shape[-1]
    to = -(-max(n, 1) // mult) * mult
    if to == n:
        return x
    out = np.zeros(x.shape[:-1] + (to,))
    out[..., :n] = x
    return out


def tree_sum(prod):
    """The optimiser's fixed tree over float64 addends (step 4)."""
    x = _pad(np.asarray(prod, dtype=np.float64).reshape(-1), CHUNK)
    chunks = _butterfly(_lane_sums(x.reshape(-1, CHUNK)))
    return float(_butterfly(_lane_sums(_pad(chunks, 64).reshape(1, -1)))[0])


def tree_dot(a, b):
    with np.errstate(over="ignore", invalid="ignore"):
        return tree_sum(np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64))


def plain_dot(a, b):
    return float(np.dot(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)))


def n_chunks(n):
    return -(-n // CHUNK)


def trial_doses(d0, d1, K):
    """Step 7: t_0 = double(d1), t_k = double(d0) + 2^-k * (double(d1) - double(d0))."""
    x0, x1 = np.asarray(d0).reshape(-1).astype(np.float64), np.asarray(d1).reshape(-1).astype(np.float64)
    out = [x1]
    with np.errstate(over="ignore", invalid="ignore"):
        dd = x1 - x0
        a = 1.0
        for _ in range(1, K):
            a *= 0.5
            out.append(x0 + a * dd)
    return out


def objective_tree_value(obj, t):
    """The objective of the float64 trial dose t by the evaluation's tree -> float (the bits of values[0])."""
    f = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for v in objective_tree_terms(obj, t):
            f = f + v
    return float(f)


def objective_tree_terms(obj, t):
    """The terms of the objective of the float64 trial dose t by the evaluation's tree -> [wn_t * sum phi_t, ...] (the bits of
    values[1:]); the objective is their sum in term order from +0.0."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    u = np.flatnonzero(obj.union())
    n_blocks = -(-u.size // 256)
    pos = np.full(obj.n_voxels, -1, dtype=np.int64)
    pos[u] = np.arange(u.size)
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for kind, roi, weight, level in obj.terms:
            idx = obj.rois[roi]
            wn = weight / float(idx.size)
            dv = t[idx]
            if kind == R.MEAN:
                phi_t = dv
            else:
                x = dv - level
                if kind == R.SQ_OVERDOSE:
                    x = np.where(x < 0.0, 0.0, x)
                elif kind == R.SQ_UNDERDOSE:
                    x = np.where(x > 0.0, 0.0, x)
                phi_t = x * x
            phi = np.zeros(n_blocks * 256)
            phi[pos[idx]] = phi_t
            w = _butterfly(phi.reshape(-1, 64)).reshape(n_blocks, 4)
            blocks = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
            acc = float(_butterfly(_lane_sums(_pad(blocks, 64).reshape(1, -1)))[0])
            out.append(float(wn * acc))
    return out


def rounding_rise_bound(obj, d):
    """How much one float32 rounding of every voxel of a float64 dose can raise the objective: |delta_v| <= 2^-24 |d_v|, first order
    sum_v (sum_t |c_t x_t|) delta_v, second order sum_t wn_t sum_v delta_v^2 (phi is at most quadratic, with curvature 2)."""
    d = np.asarray(d, dtype=np.float64)
    delta = 2.0 ** -24 * np.abs(d)
    _, _, gabs = obj.eval(d)
    second = sum(w / obj.rois[roi].size * float(np.sum(delta[obj.rois[roi]] ** 2)) for kind, roi, w, _ in obj.terms if kind != R.MEAN)
    return float(np.sum(gabs * delta)) + second


def two_loop_vectors(pairs, ghat, dot=plain_dot):
    """The textbook two-loop recursion on vectors: pairs newest first, [(s, y), ...] -> r = H ghat (float64)."""
    q = np.asarray(ghat, dtype=np.float64).copy()
    alphas = []
    for s, y in pairs:
        a = dot(s, q) / dot(s, y)
        alphas.append(a)
        q = q - a * np.asarray(y, dtype=np.float64)
    s, y = pairs[0]
    r = (dot(s, y) / dot(y, y)) * q
    for (s, y), a in zip(reversed(pairs), reversed(alphas)):
        b = dot(y, r) / dot(s, y)
        r = r + (a - b) * np.asarray(s, dtype=np.float64)
    return r


def event_letter(r):
    """The one-letter record of a step() result: R the memory was dropped (no descent with pairs held), S no trial was accepted, . nothing
    moved without a stall (no descent without pairs, or the guard), else the accepted trial index."""
    return "R" if r.get("reset") else "S" if r.get("stall") else "." if r["k"] < 0 else str(r["k"])


class LbfgsReference:
    def __init__(self, objective, matvec, rmatvec, w0, memory=8, max_halvings=5, armijo_c1=1e-4, initial_step=0.0, tree=True):
        self.obj, self.matvec, self.rmatvec = objective, matvec, rmatvec
        self.tree = bool(tree)
        self.ft = np.float32 if tree else np.float64
        self.dot = tree_dot if tree else plain_dot
        self.m, self.K, self.c1, self.initial_step = int(memory), 1 + int(max_halvings), float(armijo_c1), float(initial_step)
        self.w = np.asarray(w0).reshape(-1).astype(self.ft)
        n = self.w.size
        self.n = n
        self.w_prev, self.grad_prev = np.zeros(n, self.ft), np.zeros(n, self.ft)
        self.w_best = self.w.copy()
        self.ring = np.zeros((2 * self.m, n), self.ft)                 # the s slots, then the y slots
        D = 2 * self.m + 1
        self.G = np.zeros((D, D))
        self.head = self.count = 0
        self.moved = False
        self.stall = 1.0
        self.d0 = None                                                 # the tracked dose (stale)
        self.f_best, self.best_iteration = np.inf, -1
        self.history = []
        self.guarded = self.unit = self.backtracked = self.halvings = self.resets = self.stalls = 0
        self.a = 0.0
        self.last = {}

    # -- pieces -----------------------------------------------------------------------------------------------------------------
    def live(self, slot):
        return (self.head - 1 - slot + 2 * self.m) % self.m < self.count

    def live_indices(self):
        return [i for i in range(2 * self.m) if self.live(i % self.m)] + [2 * self.m]

    def newest_first(self):
        return [(self.head - 1 - age + 2 * self.m) % self.m for age in range(self.count)]

    def value(self, t):
        return objective_tree_value(self.obj, t) if self.tree else float(self.obj.eval(t)[0][0])

    def forward(self, w):
        with np.errstate(over="ignore", invalid="ignore"):
            return np.asarray(self.matvec(w)).reshape(-1).astype(self.ft)

    def coefficients(self, mx):
        """Step 5 on the Gram matrix -> delta (2m + 1)."""
        m, D = self.m, 2 * self.m + 1
        delta = np.zeros(D)
        if self.count == 0:
            if self.initial_step > 0.0:
                g0 = self.initial_step
            else:
                g0 = 1.0 / mx if mx > 0.0 else 0.0
            delta[2 * m] = g0 * self.stall
            return delta
        live = self.live_indices()
        G = self.G

        def inner(i, c):
            acc = 0.0
            for j in live:
                acc = acc + c[j] * G[i, j]
            return acc
        cq = np.zeros(D)
        cq[2 * m] = 1.0
        alpha = {}
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            for i in self.newest_first():
                alpha[i] = inner(i, cq) / G[i, m + i]
                cq[m + i] = cq[m + i] - alpha[i]
            newest = (self.head - 1 + m) % m
            gamma = G[newest, m + newest] / G[m + newest, m + newest]
            cq = gamma * cq
            for i in reversed(self.newest_first()):
                beta = inner(m + i, cq) / G[i, m + i]
                cq[i] = cq[i] + (alpha[i] - beta)
        for j in live:
            delta[j] = cq[j]
        return delta

    def set_weights(self, w):
        """rtd_optimizer_set_weights on an L-BFGS optimiser (k_lb_forget and lbDoseStale): w - w_prev is no pair and the pairs held
        are dropped, the tracked dose is stale (the next step takes d0 from outside or forms the product itself). The ring head, the
        stall factor, the history, f_best with its iterate and the counters stay."""
        w = np.asarray(w).reshape(-1).astype(self.ft)
        assert w.size == self.n
        self.w = w
        if not self.history:                                           # (before the first iteration the start is also the best iterate)
            self.w_best = w.copy()
        self.moved = False
        self.count = 0
        self.d0 = None

    # -- one iteration ----------------------------------------------------------------------------------------------------------
    def step(self, d0=None, d1=None, grad=None, f=None):
        """One iteration. d0 (the tracked dose entering it), d1 (the dose of w_full), grad and f replace what the restatement would
        compute itself. Returns the dict of what it decided (also self.last)."""
        m, D, K = self.m, 2 * self.m + 1, self.K
        if d0 is not None:
            self.d0 = np.asarray(d0).reshape(-1).astype(self.ft)
        elif self.d0 is None:
            self.d0 = self.forward(self.w)
        values, g, _ = self.obj.eval(self.d0)
        if f is None:
            f = self.value(self.d0.astype(np.float64))
        if grad is None:
            with np.errstate(over="ignore", invalid="ignore"):
                grad = self.rmatvec(g.astype(self.ft))
        grad = np.asarray(grad).reshape(-1).astype(self.ft)
        k_iter = len(self.history)
        self.history.append(f)
        out = {"f": f, "k": -1, "a": 0.0, "admitted": False, "guard": False}
        self.last = out
        self.a = 0.0
        if not np.isfinite(f):
            self.guarded += 1
            self.moved = False
            out["guard"] = True
            return out
        improved = f < self.f_best
        if improved:
            self.f_best, self.best_iteration, self.w_best = f, k_iter, self.w.copy()
        w64, g64 = self.w.astype(np.float64), grad.astype(np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            s = (w64 - self.w_prev.astype(np.float64)).astype(self.ft)                 # 2.
            y = (g64 - self.grad_prev.astype(np.float64)).astype(self.ft)
            active = (self.w == 0) & (grad > 0)
            ghat = np.where(active, self.ft(0.0), grad).astype(self.ft)               # 3.
            mx = float(np.max(np.where(w64 - g64 < 0.0, np.abs(w64), np.abs(g64)))) if self.n else 0.0
            # 4. the products of s, y, ghat with the live ring vectors (before the admission), with ghat, s and y
            live_old = [i for i in range(2 * m) if self.live(i % m)]
            ps = {i: self.dot(s, self.ring[i]) for i in live_old}
            py = {i: self.dot(y, self.ring[i]) for i in live_old}
            pg = {i: self.dot(ghat, self.ring[i]) for i in live_old}
            ss, sy, yy = self.dot(s, s), self.dot(s, y), self.dot(y, y)
            gs, gy, gg = self.dot(ghat, s), self.dot(ghat, y), self.dot(ghat, ghat)
        if self.moved and sy > 0.0 and yy > 0.0 and np.isfinite(sy) and np.isfinite(yy):
            h = self.head
            for i in range(2 * m):
                self.G[h, i] = self.G[i, h] = ps.get(i, 0.0)
                self.G[m + h, i] = self.G[i, m + h] = py.get(i, 0.0)
            self.G[h, h], self.G[m + h, m + h] = ss, yy
            self.G[h, m + h] = self.G[m + h, h] = sy
            self.ring[h], self.ring[m + h] = s, y
            self.head, self.count = (h + 1) % m, min(self.count + 1, m)
            out["admitted"], out["slot"] = True, h
            pg[h], pg[m + h] = gs, gy
        for i in range(2 * m):
            self.G[2 * m, i] = self.G[i, 2 * m] = pg.get(i, 0.0)
        self.G[2 * m, 2 * m] = gg
        delta = self.coefficients(mx)                                                 # 5.
        out.update(order=self.newest_first(), pairs=self.count, stall_factor=self.stall)
        with np.errstate(over="ignore", invalid="ignore"):
            acc = np.zeros(self.n)                                                    # 6.
            for i in self.live_indices():
                b = ghat if i == 2 * m else self.ring[i]
                acc = acc + delta[i] * b.astype(np.float64)
            direction = np.where(active, 0.0, -acc)
            x = w64 + direction
            w_full = np.where(x > 0.0, x, 0.0).astype(self.ft)
            gp = self.dot(grad, w_full.astype(np.float64) - w64) if self.tree else float(np.dot(g64, w_full.astype(np.float64) - w64))
        if d1 is None:
            d1 = self.forward(w_full)
        d1 = np.asarray(d1).reshape(-1).astype(self.ft)
        trials = trial_doses(self.d0, d1, K)                                          # 7.
        F = [self.value(t) for t in trials]
        out.update(G=self.G.copy(), delta=delta, w_full=w_full, gp=gp, F=F, d1=d1, mx=mx, ghat=ghat, s=s, y=y, grad=grad,
                   dots={"ss": ss, "sy": sy, "yy": yy, "gs": gs, "gy": gy, "gg": gg})
        if not gp < 0.0:
            self.moved = False
            if self.count > 0:
                self.count = 0
                self.resets += 1
                out["reset"] = True
            return out
        a, k_acc = 1.0, -1
        for k in range(K):
            if F[k] <= f + (self.c1 * a) * gp:
                k_acc = k
                break
            a *= 0.5
        if k_acc < 0:
            self.moved = False
            self.stalls += 1
            out["stall"] = True
            if self.count > 0:
                self.count = 0
            else:
                self.stall *= a
            return out
        self.moved, self.stall, self.a = True, 1.0, a
        if k_acc == 0:
            self.unit += 1
        else:
            self.backtracked += 1
            self.halvings += k_acc
        self.w_prev, self.grad_prev = self.w.copy(), grad.copy()
        if k_acc == 0:
            self.w, self.d0 = w_full.copy(), d1.copy()
        else:
            self.w = (w64 + a * (w_full.astype(np.float64) - w64)).astype(self.ft)
            self.d0 = trials[k_acc].astype(self.ft)
        out.update(k=k_acc, a=a, f_trial=F[k_acc])
        return out

    def run(self, n):
        for _ in range(n):
            self.step()
        return self
