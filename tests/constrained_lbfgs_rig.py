"""The rig of tests/test_gpu_constrained_lbfgs.py: constraint_rig.ConstraintRig (the plan that pulls against three hard constraints)
with what lbfgs_terms_rig.LbfgsTermsRig knows about an L-BFGS optimiser's device arrays, optimisers from
rtd_optimizer_create_constrained_lbfgs, the restatement beside them, and the comparisons the tests share. A plain module (no tests),
with a message on every assert."""
import numpy as np

import constraint_reference as CR
import lbfgs_terms_reference as LT
from constrained_lbfgs_reference import ConstrainedLbfgsReference
import constraint_rig
import optimizer_reference as R
from constraint_rig import ConstraintRig
from gpu_support import bits
from lbfgs_rig import LbfgsRig, lbfgs_options
from lbfgs_terms_rig import LbfgsTermsRig
from raytracedicom_amd import abi

NC = abi.RTD_CON_MAX_CONSTRAINTS


def con_dict(con):
    return dict(rho0=con.rho0, rho_growth=con.rho_growth, rho_max=con.rho_max, violation_shrink=con.violation_shrink, feasibility_tol=con.feasibility_tol,
                lambda_max=con.lambda_max, inner_iterations=con.inner_iterations)


def same_floats(a, b):
    """Bit for bit, a NaN matching any NaN."""
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


class ConstrainedLbfgsRig(ConstraintRig, LbfgsTermsRig):
    """ConstraintRig's objective and constraints; LbfgsTermsRig's products (plain or compact), peek and line."""

    def _host(self, *args):
        return LbfgsRig._host(self, *args) if args else ConstraintRig._host(self)

    def set_mixed_constrained(self):
        """LbfgsTermsRig's mixed objective (plain, DVH and EUD terms on the target and the rest) over the rig's four ROIs, plus the
        three constraints."""
        self.set_terms(self.mixed_terms(), self.rois)
        for k, c in enumerate(self.constraints):
            assert self.obj.add_constraint(*c) == k, "constraint ids count from 0 in the order added"

    def con_lbfgs(self, start=None, con=None, compact=None, **kw):
        o = self.eng.create_constrained_lbfgs_optimizer(self.fields, self.obj, lbfgs_options(**kw) if kw else None, con, compact=self.compact if compact is None else compact)
        self.opts.append(o)
        if start is not None:
            self.set_weights(o, start)
        return o

    def start_vector(self, start):
        return np.concatenate([np.full(s, start, dtype=np.float32).reshape(-1) for s in self.shapes])

    def restatement(self, w0, con, tree=True, terms_value_of=None, **kw):
        return ConstrainedLbfgsReference(self.cset(tree=tree), self.matvec, self.rmatvec, w0, con_dict(con), terms_value_of=terms_value_of, tree=tree, **kw)

    def compressed(self):
        """The rig's plan restricted to the voxels that have rows (every ROI lies inside them), in float64: the same matrices, terms
        and constraints on a volume a tenth the size, so that the float64 restatements of the convergence test take seconds.
        -> (ReferenceObjective, ConstraintSet with plain sums, matvec, rmatvec)."""
        mats = ConstraintRig._host(self)
        has = np.zeros(self.nvox, dtype=bool)
        for rows, _, _, _ in mats:
            has[rows] = True
        for m in self.rois:
            assert not np.any(np.asarray(m, dtype=bool) & ~has), "a ROI reaches outside the voxels with rows"
        pos = np.cumsum(has) - 1
        n_c = int(has.sum())
        small = [(pos[rows], cols, data, n) for rows, cols, data, n in mats]
        obj = R.ReferenceObjective(n_c)
        for m in self.rois:
            obj.add_roi(pos[np.flatnonzero(m)])
        for t in self.terms:
            obj.add_term(*t)
        cs = CR.ConstraintSet(obj, tree=False)
        for c in self.constraints:
            cs.add(*c)

        def matvec(w):
            w = np.asarray(w, dtype=np.float64).reshape(-1)
            out, a = np.zeros(n_c), 0
            for rows, cols, data, n in small:
                out += np.bincount(rows, weights=data * w[a:a + n][cols], minlength=n_c)
                a += n
            return out

        def rmatvec(g):
            g = np.asarray(g, dtype=np.float64).reshape(-1)
            return np.concatenate([np.bincount(cols, weights=data * g[rows], minlength=n) for rows, cols, data, n in small])
        return obj, cs, matvec, rmatvec

    def con_line(self, o):
        """(con_trial [K][1 + n_constraints], mean_trial [K][n_constraints]) of the last line search."""
        self.eng.sync()
        b = o.lbfgs_constraint_line()
        K, n = int(b.n_trials), int(b.n_constraints)
        con = LbfgsRig._host(self, b.con_trial, 8 * (1 + NC), np.float64).reshape(8, 1 + NC)
        mean = LbfgsRig._host(self, b.mean_trial, 8 * NC, np.float64).reshape(8, NC)
        return con[:K, :1 + n], mean[:K, :n]


def check_trials(rig, opt, d0, d1):
    """After an iteration whose line search ran on d0 and d1: for every k < K, trial_values[k] has the bits of values[0] of
    rtd_objective_eval_constrained on the uploaded r_k with the optimiser's own multipliers and penalty, and con_trial[k] those of its
    con_values."""
    lb = opt.lbfgs_report()
    con, mean = rig.con_line(opt)
    b = opt.constraint_buffers()
    _, _, rho = rig.multipliers(opt)
    K = con.shape[0]
    for k, r in enumerate(LT.rounded_trials(d0, d1, K)):
        values, con_values = rig.obj.eval_constrained(rig.upload(r), b.lambda_, b.mu, rho, rig.dG)
        print("  trial %d: F %.17g, eval_constrained %.17g, psi %s" % (k, lb["trial_values"][k], values[0], con[k, 1:]))
        assert same_floats(lb["trial_values"][k], values[0]), "F_%d = %r is not rtd_objective_eval_constrained(r_%d) = %r" % (k, lb["trial_values"][k], k, values[0])
        assert same_floats(con[k], con_values), "con_trial[%d] = %r is not con_values = %r" % (k, con[k], con_values)
    return lb, con, mean


def step_and_compare(rig, opt, ref, k, d0, trials=True):
    """Iteration k on the device (one run(1)) and in the tree-order restatement fed the device's own d0, d1 and grad; the outer update
    is the restatement's own. Bit for bit: F, G, delta, the trials with their psi and means, the decision, w_full, the new w, the best
    weights, the tracked dose, the multipliers, the penalty, the outer history and both reports. -> (the record, the new dose)."""
    w = rig.all_weights(opt)
    assert np.array_equal(bits(w), bits(ref.w)), "iteration %d: the weights entering differ" % k
    opt.run(1)
    rep, hist = opt.result()
    lb = opt.lbfgs_report()
    dev = rig.peek(opt)
    out = ref.step(d0=d0, d1=dev["d1"], grad=dev["grad"])
    K = dev["n_trials"]
    print("iteration %d%s: F %.17g, pairs %d, gp %.9g, trials %s, accepted %d (a = %g), rho %g"
          % (k, " (outer update)" if out["outer"] else "", hist[k], lb["pairs"], lb["last_gp"], " ".join("%.9g" % v for v in lb["trial_values"][:K]), lb["last_trial"],
             lb["last_step"], out["rho"]))
    assert rep["iterations"] == k + 1 and same_floats(hist[k], out["f"]) and same_floats(rep["f_last"], out["f"]), "iteration %d: F %r, restated %r" % (k, hist[k], out["f"])
    lam, mu, rho = rig.multipliers(opt)
    assert np.array_equal(bits(lam), bits(ref.lam)) and np.array_equal(bits(mu), bits(ref.mu)) and rho == ref.rho, "iteration %d: the multipliers or rho differ" % k
    assert np.array_equal(bits(dev["gram"]), bits(out["G"])), "iteration %d: G differs in %d entries" % (k, int((bits(dev["gram"]) != bits(out["G"])).sum()))
    assert np.array_equal(bits(dev["delta"]), bits(out["delta"])), "iteration %d: delta %r, restated %r" % (k, dev["delta"], out["delta"])
    assert np.array_equal(bits(dev["w_full"]), bits(out["w_full"])), "iteration %d: w_full differs in %d entries" % (k, int((dev["w_full"] != out["w_full"]).sum()))
    assert lb["last_gp"] == out["gp"], "iteration %d: gp %r, restated %r" % (k, lb["last_gp"], out["gp"])
    assert same_floats(np.array(lb["trial_values"][:K]), np.array(out["F"])), "iteration %d: trials %r, restated %r" % (k, lb["trial_values"], out["F"])
    con, mean = rig.con_line(opt)
    assert same_floats(con, np.array(out["con_trial"])), "iteration %d: con_trial %r, restated %r" % (k, con, out["con_trial"])
    assert same_floats(mean, np.array(out["mean_trial"])), "iteration %d: mean_trial %r, restated %r" % (k, mean, out["mean_trial"])
    assert lb["last_trial"] == out["k"] and lb["last_step"] == out["a"] == rep["step"], "iteration %d: the decision %r, restated k %r a %r" % (k, lb, out["k"], out["a"])
    assert lb["pairs"] == ref.count and lb["pair_admitted"] == int(out["admitted"]) and lb["ring_head"] == ref.head, "iteration %d: the ring %r" % (k, lb)
    assert (lb["unit_steps"], lb["backtracked_steps"], lb["halvings"], lb["resets"], lb["stalls"]) == (ref.unit, ref.backtracked, ref.halvings, ref.resets, ref.stalls), \
        "iteration %d: the counters %r" % (k, lb)
    assert same_floats(rep["f_best"], ref.f_best) and rep["best_iteration"] == ref.best_iteration and rep["guarded"] == ref.guarded, "iteration %d: the best iterate %r" % (k, rep)
    w_new = rig.all_weights(opt)
    assert np.array_equal(bits(w_new), bits(ref.w)), "iteration %d: the new weights differ in %d entries" % (k, int((w_new != ref.w).sum()))
    # (w_best is written by the direction kernel of the iteration that finds a better value)
    assert np.array_equal(bits(rig.all_weights(opt, best=True)), bits(ref.w_best)), "iteration %d: the best weights differ" % k
    dose = rig.volume(opt.dose())
    assert np.array_equal(bits(dose), bits(ref.d0)), "iteration %d: the updated dose differs in %d voxels" % (k, int((dose != ref.d0).sum()))
    crep, outer = opt.constraint_report()
    assert outer == [(i, r, v) for i, r, v in ref.outer], "iteration %d: the outer history %r, restated %r" % (k, outer, ref.outer)
    assert crep["rho"] == ref.rho and crep["outer_updates"] == len(ref.outer) and crep["rho_increases"] == ref.rho_increases, "iteration %d: the report %r" % (k, crep)
    assert same_floats(crep["f_objective"], ref.con_values[0]) and same_floats(np.array(crep["psi"]), ref.con_values[1:]), "iteration %d: f_objective or psi %r" % (k, crep)
    if ref.last_violation is not None:
        assert np.array_equal(bits(np.array(crep["max_violation"])), bits(ref.last_violation[0])) and list(crep["n_violating"]) == list(ref.last_violation[1]), \
            "iteration %d: the violations %r, restated %r" % (k, crep, ref.last_violation)
    if trials:
        check_trials(rig, opt, d0, out["d1"])
    return out, dose


def same_state(rig, a, b, what):
    """Two constrained L-BFGS optimisers hold the same bits: constraint_rig.same_state's list, the L-BFGS report and arrays, the tracked
    dose and the line search's constraint arrays."""
    out = constraint_rig.same_state(rig, a, b, what)
    assert a.lbfgs_report() == b.lbfgs_report(), (what, a.lbfgs_report(), b.lbfgs_report())
    pa, pb = rig.peek(a), rig.peek(b)
    for name in ("w", "w_prev", "grad", "grad_prev", "w_full", "ring", "d1", "gram", "delta"):
        assert np.array_equal(bits(pa[name]), bits(pb[name])), (what, name)
    assert np.array_equal(bits(rig.volume(a.dose())), bits(rig.volume(b.dose()))), (what, "the tracked dose")
    for x, y in zip(rig.con_line(a), rig.con_line(b)):
        assert np.array_equal(bits(x), bits(y)), (what, "the line search's constraint arrays")
    return out
