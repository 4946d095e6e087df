"""The numpy restatement of the constrained L-BFGS iteration (include/rtd.h "Constrained L-BFGS: hard dose constraints behind the line
search"), written from the header's text. A test helper, not product code.

It is lbfgs_reference.LbfgsReference on an objective whose eval is constraint_reference.ConstraintSet.eval with the multipliers and the
penalty the restatement holds: F = f + sum_c psi_c. With tree=True every trial is evaluated on the float32 volume r_k = float32(t_k)
with the trees of both references (the evaluation's tree for the terms and for psi of a per-voxel constraint, the chunk tree for a
mean), so that its bits can be compared with the device's; with tree=False everything is plain float64 on t_k. Around it: the outer
update at the CURRENT iterate (the multipliers by ConstraintSet.update on the tracked dose, the penalty rule of section 31, f_best
forgotten) and the forget of the L-BFGS memory (moved and the pairs held; ring head, stall factor and counters stay)."""
import numpy as np

import constraint_reference as CR
import lbfgs_reference as LB


class _Augmented:
    """What LbfgsReference asks of an objective: eval(dose) -> (values, g, _), here of F with the owner's multipliers."""

    def __init__(self, owner):
        self.owner = owner

    def eval(self, dose):
        o = self.owner
        values, con_values, g = o.evaluate(dose)
        o.con_values = con_values
        return values, g, None


class ConstrainedLbfgsReference(LB.LbfgsReference):
    def __init__(self, cset, matvec, rmatvec, w0, options=None, terms_value_of=None, tree=True, **lbfgs):
        """options: the keys of constraint_reference.default_options(). terms_value_of(float32 volume) -> the terms' values[0], for
        objectives numpy cannot restate to the bit (EUD terms); the terms' gradient is then not formed (step() needs grad)."""
        super().__init__(_Augmented(self), matvec, rmatvec, w0, tree=tree, **lbfgs)
        self.cs = cset
        self.opt = CR.default_options()
        self.opt.update(options or {})
        self.terms_value_of = terms_value_of
        self.lam = np.zeros(cset.n_entries, dtype=np.float32)
        self.mu = np.zeros(CR.MAX_CONSTRAINTS, dtype=np.float64)
        self.rho = float(self.opt["rho0"])
        self.v_prev = 0.0
        self.outer = []              # (iteration, rho, v)
        self.rho_increases = 0
        self.last_violation = None
        self.con_values = None       # of the last evaluation of an iterate: [terms' value, psi_c ...]
        self.trial_con = []          # of the last line search, per trial: [terms' value, psi_c ...]
        self.trial_mean = []         # ... and the means of the mean constraints (0 for the others)
        self._collect = False

    # -- F ----------------------------------------------------------------------------------------------------------------------
    def evaluate(self, dose):
        """ConstraintSet.eval of a dose with the multipliers held -> (values, con_values, g)."""
        if self.terms_value_of is None:
            return self.cs.eval(dose, self.lam, self.mu, self.rho)
        r = np.asarray(dose).astype(np.float32)
        vt = np.array([float(self.terms_value_of(r))], dtype=np.float64)
        return self.cs.eval(r, self.lam, self.mu, self.rho, g_terms=np.zeros(self.cs.obj.n_voxels, dtype=np.float32), values_terms=vt)

    def value(self, t):
        with np.errstate(over="ignore", invalid="ignore"):
            r = np.asarray(t).astype(np.float32) if self.tree else np.asarray(t, dtype=np.float64)
            values, con_values, _ = self.evaluate(r)
        if self._collect:
            self.trial_con.append(con_values.copy())
            d = r.astype(np.float64)
            self.trial_mean.append(np.array([self.cs.mean(c, d) if self.cs.is_mean(kind) else 0.0 for c, (kind, _, _) in enumerate(self.cs.cons)]))
        return float(values[0])

    # -- the outer update -------------------------------------------------------------------------------------------------------
    def outer_due(self):
        k = len(self.history)
        return k > 0 and k % int(self.opt["inner_iterations"]) == 0

    def decide(self, mx, cnt=None):
        """Section 31's step (e) on the violations of the update, then the forget."""
        v = max(float(np.max(mx)) if len(mx) else 0.0, 0.0)
        if self.outer and v > self.opt["feasibility_tol"] and v > self.opt["violation_shrink"] * self.v_prev:
            self.rho = min(self.rho * self.opt["rho_growth"], self.opt["rho_max"])
            self.rho_increases += 1
        self.v_prev = v
        self.outer.append((len(self.history), self.rho, v))
        self.f_best = np.inf
        self.last_violation = (np.asarray(mx).copy(), None if cnt is None else np.asarray(cnt).copy())
        self.moved = False
        self.count = 0

    def outer_update(self, dose):
        self.lam, self.mu, mx, cnt = self.cs.update(dose, self.rho, self.lam, self.mu, self.opt["lambda_max"], self.opt["feasibility_tol"])
        self.decide(mx, cnt)

    # -- one iteration ----------------------------------------------------------------------------------------------------------
    def step(self, d0=None, d1=None, grad=None, f=None, updated=None):
        """One iteration. d0, d1, grad, f as for LbfgsReference.step. updated = (lambda, mu, max_violation, n_violating): the outer
        update's results where they come from elsewhere (the device's public call); the decision is still taken here."""
        if d0 is not None:
            self.d0 = np.asarray(d0).reshape(-1).astype(self.ft)
        elif self.d0 is None:
            self.d0 = self.forward(self.w)
        out_update = self.outer_due()
        if out_update:
            if updated is None:
                self.outer_update(self.d0)
            else:
                self.lam, self.mu = np.asarray(updated[0], dtype=np.float32).copy(), np.asarray(updated[1], dtype=np.float64).copy()
                self.decide(updated[2], updated[3])
        f_before = self.history[-1] if self.history else None
        self.trial_con, self.trial_mean = [], []
        self._collect = False
        if f is None:
            f = self.value(self.d0)                                    # (before the trials are collected)
        self._collect = True
        try:
            out = super().step(d0=None, d1=d1, grad=grad, f=f)
        finally:
            self._collect = False
        if "F" in out:
            n = len(out["F"])
            self.trial_con, self.trial_mean = self.trial_con[-n:], self.trial_mean[-n:]
        out.update(outer=out_update, f_before=f_before, rho=self.rho, con_trial=self.trial_con, mean_trial=self.trial_mean)
        return out
