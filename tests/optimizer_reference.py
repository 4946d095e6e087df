"""The float64 numpy restatement of rtd_objective_eval and of one iteration of rtd_optimizer_run (include/rtd.h).
A test helper, not product code: the device loop is checked against it step by step.

ReferenceObjective.eval follows the header's arithmetic: d widened to float64, per voxel the terms in term order starting from 0.0,
c_t = 2 w_t / N_t and wn_t = w_t / N_t computed once, products and sums separately rounded (numpy does not contract).
ReferenceOptimizer.step is steps 1-7 of the iteration on any pair of callables (matvec: weights -> flat dose, rmatvec: flat voxel
gradient -> spot gradient), e.g. the methods of engine.DoseInfluence; `dose` / `grad` may be fed from outside (the device's own), so
that only the objective, the step length and the update are compared."""
import numpy as np

SQ_DEVIATION, SQ_OVERDOSE, SQ_UNDERDOSE, MEAN = 0, 1, 2, 3


class ReferenceObjective:
    def __init__(self, n_voxels):
        self.n_voxels = int(n_voxels)
        self.rois = []
        self.terms = []     # (kind, roi, weight, level)

    def add_roi(self, mask_or_indices):
        a = np.asarray(mask_or_indices)
        idx = np.flatnonzero(a) if a.dtype == np.bool_ else a.reshape(-1)
        idx = idx.astype(np.int64)
        assert idx.size > 0 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < self.n_voxels
        self.rois.append(idx)
        return len(self.rois) - 1

    def add_term(self, kind, roi, weight, level=0.0):
        assert kind in (SQ_DEVIATION, SQ_OVERDOSE, SQ_UNDERDOSE, MEAN) and 0 <= roi < len(self.rois) and weight > 0
        self.terms.append((int(kind), int(roi), float(weight), float(level)))

    def union(self):
        m = np.zeros(self.n_voxels, dtype=bool)
        for r in self.rois:
            m[r] = True
        return m

    def eval(self, dose):
        """-> (values float64[1 + terms], g float64[n_voxels] (0 outside the union, NOT yet rounded to float32),
        gabs float64[n_voxels] = sum_t |c_t x_t| per voxel, the scale of g's rounding bound)."""
        d = np.asarray(dose).reshape(-1).astype(np.float64)
        assert d.size == self.n_voxels
        g = np.zeros(self.n_voxels, dtype=np.float64)
        gabs = np.zeros(self.n_voxels, dtype=np.float64)
        values = np.zeros(1 + len(self.terms), dtype=np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            for t, (kind, roi, weight, level) in enumerate(self.terms):
                idx = self.rois[roi]
                n = float(idx.size)
                c, wn = 2.0 * weight / n, weight / n
                dv = d[idx]
                if kind == MEAN:
                    phi = dv
                    contrib = np.full(idx.size, wn)
                else:
                    x = dv - level
                    if kind == SQ_OVERDOSE:
                        x = np.where(x < 0.0, 0.0, x)
                    elif kind == SQ_UNDERDOSE:
                        x = np.where(x > 0.0, 0.0, x)
                    phi = x * x
                    contrib = c * x
                g[idx] = g[idx] + contrib          # (term order per voxel: the terms are visited in order)
                gabs[idx] = gabs[idx] + np.abs(contrib)
                values[1 + t] = wn * float(np.sum(phi))
            f = 0.0
            for t in range(len(self.terms)):
                f = f + values[1 + t]
            values[0] = f
        return values, g, gabs


def project(x):
    return np.where(x > 0.0, x, 0.0)


def step_length(w, w_prev, grad, grad_prev, have_bb, step_min=1e-30, step_max=1e30):
    """Step 5 in float64 on float32 or float64 vectors."""
    w, grad = np.asarray(w, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if not have_bb:
            # |P(w - grad) - w| evaluated without cancellation (grad may be 1e-15 of w): -w where the projection acts, else -grad
            m = float(np.max(np.where(w - grad < 0.0, np.abs(w), np.abs(grad)))) if w.size else 0.0
            return 1.0 / m if m > 0.0 else 0.0
        s = w - np.asarray(w_prev, dtype=np.float64)
        y = grad - np.asarray(grad_prev, dtype=np.float64)
        ss, sy = float(np.dot(s, s)), float(np.dot(s, y))
        a = ss / sy if sy > 0.0 else step_max
        if not a >= step_min:
            a = step_min
        return step_max if a > step_max else a


class ReferenceOptimizer:
    """float32=True rounds g, grad and w to float32 where the device does (the products themselves stay what the callables give);
    float32=False is the iteration in float64 throughout."""

    def __init__(self, objective, matvec, rmatvec, w0, step_min=1e-30, step_max=1e30, float32=True):
        self.obj, self.matvec, self.rmatvec = objective, matvec, rmatvec
        self.ft = np.float32 if float32 else np.float64
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

    def step(self, dose=None, grad=None):
        """One iteration; dose (flat or volume) and grad (flat) replace the two products when given. Returns f_k."""
        if dose is None:
            dose = self.matvec(self.w)                                            # 1.
        values, g, _ = self.obj.eval(dose)                                        # 2.
        if grad is None:
            with np.errstate(over="ignore", invalid="ignore"):
                grad = self.rmatvec(g.astype(self.ft))                            # 3.
        return self.advance(float(values[0]), grad)

    def advance(self, f, grad):
        """Steps 4-7 for an objective value and a spot gradient obtained elsewhere."""
        self.history.append(f)
        grad = np.asarray(grad).reshape(-1).astype(self.ft)
        k = len(self.history) - 1
        if not np.isfinite(f):                                                    # 7.
            self.w = self.w_best.copy()
            self.have_bb = False
            self.guarded += 1
            return f
        if f < self.f_best:                                                       # 4.
            self.f_best, self.best_iteration, self.w_best = f, k, self.w.copy()
        self.alpha = step_length(self.w, self.w_prev, grad, self.grad_prev, self.have_bb, self.step_min, self.step_max)   # 5.
        self.have_bb = True
        self.w_prev, self.grad_prev = self.w.copy(), grad.copy()                  # 6.
        with np.errstate(over="ignore", invalid="ignore"):
            self.w = update(self.w, grad, self.alpha, self.ft)
        return f

    def run(self, n):
        for _ in range(n):
            self.step()
        return self


def update(w, grad, alpha, ft=np.float32):
    """Step 6: P(w - ft(alpha) * grad) in ft, the product rounded before the subtraction."""
    w, grad = np.asarray(w, dtype=ft), np.asarray(grad, dtype=ft)
    prod = (ft(alpha) * grad).astype(ft)
    return project((w - prod).astype(ft)).astype(ft)
