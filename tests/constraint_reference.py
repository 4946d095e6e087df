"""The numpy restatement of the hard dose constraints (include/rtd.h "Hard dose constraints: an augmented Lagrangian resident on the
device"), written from the header's text. A test helper, not product code.

ConstraintSet restates the arithmetic on an optimizer_reference.ReferenceObjective: the tables (union of the constrained ROIs, CSR of
the per-voxel constraints, mask of the mean ones), eval (F, con_values, the combined float32 gradient), update (the multipliers and
the violations). With tree=True every sum follows the device's order (the evaluation's tree over the union of the constrained ROIs for
psi, the chunk tree of rtd_objective_eud for a mean, the evaluation's tree for the terms), so its bits can be compared with the
device's; tree=False sums with numpy.
ConstrainedReference restates the iteration of rtd_optimizer_create_constrained on any pair of callables (matvec, rmatvec). Its pieces
(outer_due, outer_update, evaluate, advance) can be fed with the device's own doses and gradients, so that a loop driven from outside
with the public calls is compared step by step."""
import numpy as np

import lbfgs_reference as LB
import optimizer_reference as R

MAX_DOSE, MIN_DOSE, MAX_MEAN, MIN_MEAN = 0, 1, 2, 3
MAX_CONSTRAINTS = 16
EUD_CHUNK = 2048


def _block_sums(x):
    """x [rows, 256] float64: per row the wave butterflies, then (w0 + w1) + (w2 + w3)."""
    w = LB._butterfly(x.reshape(-1, 64)).reshape(-1, 4)
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def eval_tree_sum(addends):
    """The evaluation's tree over one addend per union voxel (in union order): blocks of 256, then block b to lane b mod 64."""
    blocks = _block_sums(LB._pad(np.asarray(addends, dtype=np.float64).reshape(-1), 256).reshape(-1, 256))
    return float(LB._butterfly(LB._lane_sums(LB._pad(blocks, 64).reshape(1, -1)))[0])


def _thread_sums(x):
    """x [rows, 256 k] float64: thread t's sequential sum of the entries t, t + 256, ... of its row from +0.0 -> [rows, 256]."""
    rows, length = x.shape
    acc = np.zeros((rows, 256))
    for i in range(length // 256):
        acc = acc + x[:, 256 * i:256 * i + 256]
    return acc


def chunk_tree_sum(vals):
    """The chunk tree of rtd_objective_eud over a ROI's values in list order: chunks of 2048, thread t adds t, t + 256, ..., block sum;
    the chunk sums: chunk c to thread c mod 256, block sum."""
    x = LB._pad(np.asarray(vals, dtype=np.float64).reshape(-1), EUD_CHUNK).reshape(-1, EUD_CHUNK)
    chunks = _block_sums(_thread_sums(x))
    return float(_block_sums(_thread_sums(LB._pad(chunks, 256).reshape(1, -1)))[0])


def _a_of(lam, rho, h):
    u = lam + rho * h
    a = np.where(u > 0.0, u, 0.0)
    return np.where(np.isnan(h), h, a)


class ConstraintSet:
    def __init__(self, objective, tree=True):
        self.obj = objective
        self.tree = tree
        self.cons = []      # (kind, roi, level)
        self._tab = None

    def add(self, kind, roi, level):
        assert kind in (MAX_DOSE, MIN_DOSE, MAX_MEAN, MIN_MEAN) and 0 <= roi < len(self.obj.rois) and len(self.cons) < MAX_CONSTRAINTS
        self.cons.append((int(kind), int(roi), float(level)))
        self._tab = None
        return len(self.cons) - 1

    @staticmethod
    def sign(kind):
        return 1.0 if kind in (MAX_DOSE, MAX_MEAN) else -1.0

    @staticmethod
    def is_mean(kind):
        return kind >= MAX_MEAN

    def tables(self):
        """-> dict: uv (union of the constrained ROIs, ascending), ptr / idx (CSR of the per-voxel constraints in constraint order),
        entries[c] (the CSR entries of constraint c, in ROI order), pos[c] (the union positions of the ROI of constraint c)."""
        if self._tab is None:
            m = np.zeros(self.obj.n_voxels, dtype=bool)
            for _, roi, _ in self.cons:
                m[self.obj.rois[roi]] = True
            uv = np.flatnonzero(m)
            where = np.full(self.obj.n_voxels, -1, dtype=np.int64)
            where[uv] = np.arange(uv.size)
            count = np.zeros(uv.size, dtype=np.int64)
            for kind, roi, _ in self.cons:
                if not self.is_mean(kind):
                    count[where[self.obj.rois[roi]]] += 1
            ptr = np.concatenate([[0], np.cumsum(count)])
            idx = np.zeros(int(ptr[-1]), dtype=np.uint8)
            fill = ptr[:-1].copy()
            entries, pos = [], []
            for c, (kind, roi, _) in enumerate(self.cons):
                p = where[self.obj.rois[roi]]
                pos.append(p)
                if self.is_mean(kind):
                    entries.append(np.zeros(0, dtype=np.int64))
                    continue
                e = fill[p].copy()
                idx[e] = c
                fill[p] += 1
                entries.append(e)
            self._tab = dict(uv=uv, ptr=ptr, idx=idx, entries=entries, pos=pos)
        return self._tab

    @property
    def n_entries(self):
        return int(self.tables()["ptr"][-1])

    def _sum_eval(self, c, addends):
        if not self.tree:
            return float(np.sum(addends))
        t = self.tables()
        x = np.zeros(t["uv"].size)
        x[t["pos"][c]] = addends
        return eval_tree_sum(x)

    def mean(self, c, d):
        _, roi, _ = self.cons[c]
        idx = self.obj.rois[roi]
        s = chunk_tree_sum(d[idx]) if self.tree else float(np.sum(d[idx]))
        return s * (1.0 / float(idx.size))

    def term_values(self, dose):
        """values of the terms alone: [f, term 0, ...] (by the evaluation's tree with tree=True) and the float32 gradient of the terms."""
        vals, g, _ = self.obj.eval(dose)
        if self.tree:
            terms = LB.objective_tree_terms(self.obj, np.asarray(dose, dtype=np.float64).reshape(-1))
            f = 0.0
            with np.errstate(over="ignore", invalid="ignore"):
                for v in terms:
                    f = f + v
            vals = np.array([f] + list(terms), dtype=np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            return vals, g.astype(np.float32)

    def eval(self, dose, lam, mu, rho, g_terms=None, values_terms=None):
        """-> (values float64[1 + terms] with values[0] = F, con_values float64[1 + constraints], g float32[n_voxels]). g_terms /
        values_terms: the terms' own gradient (float32) and values when they come from elsewhere (the device's)."""
        d = np.asarray(dose).reshape(-1).astype(np.float64)
        lam = np.asarray(lam, dtype=np.float32).astype(np.float64)
        mu = np.asarray(mu, dtype=np.float64)
        rho = float(rho)
        if g_terms is None or values_terms is None:
            vt, gt = self.term_values(dose)
            values_terms = vt if values_terms is None else values_terms
            g_terms = gt if g_terms is None else g_terms
        t = self.tables()
        G = np.zeros(self.obj.n_voxels, dtype=np.float64)
        con_values = np.zeros(1 + len(self.cons), dtype=np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            for c, (kind, roi, level) in enumerate(self.cons):
                idx = self.obj.rois[roi]
                s, inv_n = self.sign(kind), 1.0 / float(idx.size)
                if self.is_mean(kind):
                    h = np.float64(s * (self.mean(c, d) - level))
                    a = float(_a_of(mu[c], rho, h))
                    psi = (a * a - mu[c] * mu[c]) / (2.0 * rho)
                    gc = np.full(idx.size, s * (a * inv_n))
                else:
                    l = lam[t["entries"][c]]
                    h = s * (d[idx] - level)
                    a = _a_of(l, rho, h)
                    psi = self._sum_eval(c, a * a - l * l) * (inv_n / (2.0 * rho))
                    gc = s * (a * inv_n)
                G[idx] = G[idx] + gc
                con_values[1 + c] = psi
            values = np.array(values_terms, dtype=np.float64).copy()
            con_values[0] = values[0]
            f = values[0]
            for c in range(len(self.cons)):
                f = f + con_values[1 + c]
            values[0] = f
            g = np.asarray(g_terms, dtype=np.float32).copy()
            uv = t["uv"]
            g[uv] = (g[uv].astype(np.float64) + G[uv]).astype(np.float32)
        return values, con_values, g

    def update(self, dose, rho, lam, mu, lambda_max=1e20, tol=0.0, apply=True):
        """-> (lambda float32[n_entries], mu float64[16], max_violation float64[constraints], n_violating int64[constraints]); with
        apply=False the multipliers come back unchanged (rtd_objective_constraint_violations)."""
        d = np.asarray(dose).reshape(-1).astype(np.float64)
        lam = np.asarray(lam, dtype=np.float32).copy()
        mu = np.asarray(mu, dtype=np.float64).copy()
        t = self.tables()
        mx, cnt = np.zeros(len(self.cons)), np.zeros(len(self.cons), dtype=np.int64)
        with np.errstate(over="ignore", invalid="ignore"):
            for c, (kind, roi, level) in enumerate(self.cons):
                idx = self.obj.rois[roi]
                s = self.sign(kind)
                if self.is_mean(kind):
                    h = np.array([s * (self.mean(c, d) - level)])
                    old = mu[c:c + 1]
                else:
                    h = s * (d[idx] - level)
                    old = lam[t["entries"][c]].astype(np.float64)
                if apply:
                    u = old + float(rho) * h
                    new = np.minimum(np.where(u > 0.0, u, 0.0), lambda_max)
                    new = np.where(np.isfinite(h), new, old)
                    if self.is_mean(kind):
                        mu[c] = new[0]
                    else:
                        lam[t["entries"][c]] = new.astype(np.float32)
                pos = np.where(h > 0.0, h, 0.0)
                mx[c] = float(pos.max()) if pos.size else 0.0
                cnt[c] = int(np.count_nonzero(h > tol))
        return lam, mu, mx, cnt

    def violations(self, dose, tol=0.0):
        _, _, mx, cnt = self.update(dose, 1.0, np.zeros(self.n_entries, dtype=np.float32), np.zeros(MAX_CONSTRAINTS), tol=tol, apply=False)
        return mx, cnt


def default_options():
    return dict(rho0=1.0, rho_growth=4.0, rho_max=1e8, violation_shrink=0.5, feasibility_tol=0.0, lambda_max=1e20, inner_iterations=20)


class ConstrainedReference:
    """The iteration of rtd_optimizer_create_constrained. float32=True keeps w, grad and g in float32 as the device does; tree=True
    takes the step length's two sums by the optimiser's chunk tree (lbfgs_reference.tree_dot), so that the bits can be compared."""

    def __init__(self, cset, matvec, rmatvec, w0, options=None, step_min=1e-30, step_max=1e30, float32=True, tree=True):
        self.cs, self.matvec, self.rmatvec = cset, matvec, rmatvec
        self.opt = default_options()
        self.opt.update(options or {})
        self.ft = np.float32 if float32 else np.float64
        self.dot = LB.tree_dot if tree else LB.plain_dot
        self.w = np.asarray(w0).reshape(-1).astype(self.ft)
        self.w_best = self.w.copy()
        self.w_prev = np.zeros_like(self.w)
        self.grad_prev = np.zeros_like(self.w)
        self.step_min, self.step_max = step_min, step_max
        self.have_bb = False
        self.f_best, self.best_iteration = np.inf, -1
        self.alpha = 0.0
        self.history = []
        self.guarded = 0
        self.start_bad = False
        self.lam = np.zeros(cset.n_entries, dtype=np.float32)
        self.mu = np.zeros(MAX_CONSTRAINTS, dtype=np.float64)
        self.rho = float(self.opt["rho0"])
        self.v_prev = 0.0
        self.outer = []          # (iteration, rho, v)
        self.rho_increases = 0
        self.last_violation = None

    @property
    def k(self):
        return len(self.history)

    def outer_due(self):
        return self.k > 0 and self.k % int(self.opt["inner_iterations"]) == 0

    def restore(self):
        """Step 0a."""
        if self.f_best < np.inf:
            self.w = self.w_best.copy()

    def decide(self, mx, cnt=None):
        """Step 0e on the violations of the update."""
        v = float(np.max(mx)) if len(mx) else 0.0
        v = max(v, 0.0)
        if self.outer and v > self.opt["feasibility_tol"] and v > self.opt["violation_shrink"] * self.v_prev:
            self.rho = min(self.rho * self.opt["rho_growth"], self.opt["rho_max"])
            self.rho_increases += 1
        self.v_prev = v
        self.outer.append((self.k, self.rho, v))
        self.f_best = np.inf
        self.have_bb = False
        self.last_violation = (np.asarray(mx).copy(), None if cnt is None else np.asarray(cnt).copy())

    def outer_update(self, dose):
        """Steps 0d and 0e on the dose of the restored iterate."""
        self.lam, self.mu, mx, cnt = self.cs.update(dose, self.rho, self.lam, self.mu, self.opt["lambda_max"], self.opt["feasibility_tol"])
        self.decide(mx, cnt)

    def step_length(self, grad):
        w, g = self.w.astype(np.float64), np.asarray(grad, dtype=np.float64)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            if not self.have_bb:
                m = float(np.max(np.where(w - g < 0.0, np.abs(w), np.abs(g)))) if w.size else 0.0
                return 1.0 / m if m > 0.0 else 0.0
            s, y = w - self.w_prev.astype(np.float64), g - self.grad_prev.astype(np.float64)
            ss, sy = self.dot(s, s), self.dot(s, y)
            a = ss / sy if sy > 0.0 else self.step_max
            if not a >= self.step_min:
                a = self.step_min
            return self.step_max if a > self.step_max else a

    def advance(self, f, grad):
        """Steps 4 to 7 of the spectral iteration on F and the spot gradient of the combined g."""
        k = self.k
        self.history.append(float(f))
        grad = np.asarray(grad).reshape(-1).astype(self.ft)
        if not np.isfinite(f):
            if not self.f_best < np.inf:
                self.start_bad = True
            self.w = self.w_best.copy()
            self.have_bb = False
            self.guarded += 1
            return f
        if f < self.f_best:
            self.f_best, self.best_iteration, self.w_best = float(f), k, self.w.copy()
        self.alpha = self.step_length(grad)
        self.have_bb = True
        self.w_prev, self.grad_prev = self.w.copy(), grad.copy()
        with np.errstate(over="ignore", invalid="ignore"):
            self.w = R.update(self.w, grad, self.alpha, self.ft)
        return f

    def step(self):
        if self.outer_due():
            self.restore()
            dose = self.matvec(self.w)
            self.outer_update(dose)
        else:
            dose = self.matvec(self.w)
        values, con_values, g = self.cs.eval(dose, self.lam, self.mu, self.rho)
        self.con_values = con_values
        with np.errstate(over="ignore", invalid="ignore"):
            grad = self.rmatvec(g.astype(self.ft))
        return self.advance(float(values[0]), grad)

    def run(self, n):
        for _ in range(n):
            self.step()
        return self
