"""The rig of tests/test_gpu_constraints.py, part two: gpu_plan_rigs.OptimizerRig with an objective that pulls against three hard
constraints which the weights the plan was made from satisfy strictly. A plain module beside gpu_plan_rigs.py, under the same rule
(test files import from here, never from each other), with a message on every assert."""
import numpy as np

import constraint_reference as CR
import optimizer_reference as R
from gpu_plan_rigs import OptimizerRig
from gpu_support import bits
from raytracedicom_amd import abi


def constrained_options(**kw):
    o = abi.default_constrained_options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class ConstraintRig(OptimizerRig):
    """The target (where Dij w_true exceeds half its maximum) carries SQ_DEVIATION at 1.3 x its mean dose: the objective wants more
    than the plan gave. Against it: MAX_DOSE on the organ (the voxels outside the target that received more than a quarter of the
    maximum) at 1.02 x its largest dose under w_true, MIN_DOSE on the target's core (above 80 % of the maximum) at 0.98 x its
    smallest, MAX_MEAN on everything outside the target at 1.02 x its mean."""

    def __init__(self, engine, scn):
        super().__init__(engine, scn)
        self.obj.destroy()
        dose_true = sum(d.matvec(w) for d, w in zip(self.mats, self.w_true))
        has = sum(np.bincount(d.indices, minlength=self.nvox) for d in self.mats) > 0
        target = dose_true > 0.5 * dose_true.max()
        other = has & ~target
        organ = other & (dose_true > 0.25 * dose_true.max())
        core = dose_true > 0.8 * dose_true.max()
        assert organ.sum() > 0 and core.sum() > 0, "the scene has no organ or no core"
        self.dose_true = dose_true
        self.rois = [target, other, organ, core]
        self.terms = [(R.SQ_DEVIATION, 0, 1.0, 1.3 * self.level), (R.SQ_OVERDOSE, 1, 1.0, 0.3 * self.level), (R.MEAN, 1, 1e-3 * self.level, 0.0)]
        self.constraints = [(CR.MAX_DOSE, 2, 1.02 * float(dose_true[organ].max())), (CR.MIN_DOSE, 3, 0.98 * float(dose_true[core].min())),
                            (CR.MAX_MEAN, 1, 1.02 * float(dose_true[other].mean()))]
        self.obj, self.ref = self.objective(constraints=True)
        self.extra = []

    def objective(self, constraints, extra_roi=None):
        """A device objective and its restatement with the rig's ROIs and terms; the constraints on request; extra_roi: one more ROI
        that nothing uses."""
        obj, ref = self.eng.create_objective(self.dims), R.ReferenceObjective(self.nvox)
        for m in self.rois + ([] if extra_roi is None else [extra_roi]):
            obj.add_roi(m)
            ref.add_roi(m)
        for t in self.terms:
            obj.add_term(*t)
            ref.add_term(*t)
        if constraints:
            for k, c in enumerate(self.constraints):
                assert obj.add_constraint(*c) == k, "constraint ids count from 0 in the order added"
        return obj, ref

    def cset(self, tree):
        cs = CR.ConstraintSet(self.ref, tree=tree)
        for c in self.constraints:
            cs.add(*c)
        return cs

    def constrained(self, start=None, con=None, options=None):
        o = self.eng.create_constrained_optimizer(self.fields, self.obj, options, con)
        self.opts.append(o)
        if start is not None:
            self.set_weights(o, start)
        return o

    def _host(self):
        if not hasattr(self, "_mats64"):
            self._mats64 = [(d.indices, d._col_of_entry(), d.data.astype(np.float64), d.shape[1]) for d in self.mats]
        return self._mats64

    def matvec(self, w):
        """The float64 product of OptimizerRig.matvec, by np.bincount (the 400 products of the convergence test in a second or two)."""
        w = np.asarray(w, dtype=np.float64).reshape(-1)
        out, a = np.zeros(self.nvox), 0
        for rows, cols, data, n in self._host():
            out += np.bincount(rows, weights=data * w[a:a + n][cols], minlength=self.nvox)
            a += n
        return out

    def rmatvec(self, g):
        g = np.asarray(g, dtype=np.float64).reshape(-1)
        return np.concatenate([np.bincount(cols, weights=data * g[rows], minlength=n) for rows, cols, data, n in self._host()])

    def split(self, w):
        offs = np.cumsum([0] + self.sizes)
        return [np.asarray(w[a:b], dtype=np.float32).reshape(s) for a, b, s in zip(offs, offs[1:], self.shapes)]

    def spot_grad(self, dG):
        """Dij_f^T g per field through rtd_field_dose_influence_apply_t, concatenated."""
        out = []
        for f, n in zip(self.fields, self.sizes):
            d = self.alloc(4 * n)
            f.dose_influence_apply_t(dG, d)
            g = np.empty(n, dtype=np.float32)
            self.eng.to_host(g, d)
            out.append(g)
        return np.concatenate(out)

    def multipliers(self, o):
        """(lambda float32[n_entries], mu float64[16], rho) of a constrained optimiser, from its device buffers."""
        b = o.constraint_buffers()
        self.eng.sync()
        lam, mu, rho = np.empty(max(1, b.n_entries), dtype=np.float32), np.empty(abi.RTD_CON_MAX_CONSTRAINTS, dtype=np.float64), np.empty(1, dtype=np.float64)
        self.eng.to_host(lam, b.lambda_)
        self.eng.to_host(mu, b.mu)
        self.eng.to_host(rho, b.rho)
        return lam[:b.n_entries], mu, float(rho[0])

    def violation_of(self, ws, tol=0.0):
        """The largest violation of the dose of the weights ws, through apply and rtd_objective_constraint_violations."""
        dDose = self.alloc(4 * self.nvox)
        self.dose_of(ws, dDose)
        mx, cnt = self.obj.constraint_violations(dDose, tol)
        return float(mx.max()), mx, cnt

    def driven_loop(self, start, n, con):
        """n iterations of the constrained iteration driven from here: the products through rtd_field_dose_influence_apply / _apply_t,
        the evaluation and the multiplier update through the public calls of the objective, the scalar decisions and the weight
        update by the restatement (with the optimiser's summation tree). -> the ConstrainedReference that kept the state, with lam,
        mu as the device left them."""
        w0 = np.concatenate([np.full(s, start, dtype=np.float32).reshape(-1) for s in self.shapes])
        opt = dict(rho0=con.rho0, rho_growth=con.rho_growth, rho_max=con.rho_max, violation_shrink=con.violation_shrink, feasibility_tol=con.feasibility_tol,
                   lambda_max=con.lambda_max, inner_iterations=con.inner_iterations)
        st = CR.ConstrainedReference(self.cset(tree=True), None, None, w0, opt, float32=True, tree=True)
        lay = self.obj.constraint_layout()
        dDose, dG = self.alloc(4 * self.nvox), self.alloc(4 * self.nvox)
        dLam, dMu = self.alloc(4 * max(1, lay.n_entries)), self.alloc(8 * abi.RTD_CON_MAX_CONSTRAINTS)
        for _ in range(n):
            outer = st.outer_due()
            if outer:
                st.restore()
            self.dose_of(self.split(st.w), dDose)
            if outer:
                mx, cnt = self.obj.update_multipliers(dDose, st.rho, dLam, dMu, con.lambda_max, con.feasibility_tol)
                st.decide(mx, cnt)
            values, con_values = self.obj.eval_constrained(dDose, dLam, dMu, st.rho, dG)
            st.con_values = con_values
            st.advance(float(values[0]), self.spot_grad(dG))
        st.lam = np.empty(max(1, lay.n_entries), dtype=np.float32)
        self.eng.to_host(st.lam, dLam)
        st.lam = st.lam[:lay.n_entries]
        self.eng.to_host(st.mu, dMu)
        return st

    def close(self):
        for o in self.extra:
            o.destroy()
        super().close()


def same_state(rig, a, b, what):
    """Two constrained optimisers hold the same bits: reports, histories, weights, best weights, multipliers, penalty, outer history."""
    ra, ha = a.result()
    rb, hb = b.result()
    assert ra == rb and np.array_equal(bits(ha), bits(hb)), (what, ra, rb)
    ca, oa = a.constraint_report()
    cb, ob = b.constraint_report()
    assert ca == cb and oa == ob, (what, ca, cb, oa, ob)
    for best in (False, True):
        for x, y in zip(rig.weights(a, best), rig.weights(b, best)):
            assert np.array_equal(bits(x), bits(y)), (what, "weights", best)
    la, ma, rha = rig.multipliers(a)
    lb, mb, rhb = rig.multipliers(b)
    assert np.array_equal(bits(la), bits(lb)) and np.array_equal(bits(ma), bits(mb)) and rha == rhb, (what, "multipliers")
    return ra, ha, ca, oa
