"""The restatement of the L-BFGS line search on an objective with DVH or EUD terms (rtd_optimizer_create_lbfgs_ex, include/rtd.h
"L-BFGS with DVH and EUD terms, and on the compact matrix"), beside lbfgs_reference. A test helper, not product
code.

With such terms every term of every trial is evaluated on the float32-rounded trial volume r_k = float32(t_k). Two variants of
lbfgs_reference.LbfgsReference restate that:
  LbfgsTermsReference   plain and DVH kinds in pure numpy by the evaluation's tree (the selection is an exact order statistic of a
                        float32 volume), so that its bits can be compared with the device's;
  LbfgsValueReference   the value of a rounded trial comes from a callable (the device's own rtd_objective_eval on the uploaded
                        volume): for objectives with EUD terms, whose pow numpy cannot restate to the bit."""
import numpy as np

import dvh_reference as D
import lbfgs_reference as LB
import optimizer_reference as R


def rounded_trials(d0, d1, K):
    """r_k = float32(t_k), t_0 = double(d1), t_k = double(d0) + 2^-k (double(d1) - double(d0)) -> K float32 volumes."""
    with np.errstate(over="ignore", invalid="ignore"):
        return [t.astype(np.float32) for t in LB.trial_doses(d0, d1, K)]


def tree_terms(obj, r):
    """The plain and DVH terms of a DvhReferenceObjective on the float32 volume r by the evaluation's tree -> [wn_t * sum phi_t, ...]:
    lbfgs_reference.objective_tree_terms with the two DVH kinds of k_obj_eval (D_v of this volume, a NaN dose kept)."""
    r = np.asarray(r, dtype=np.float32).reshape(-1)
    t64 = r.astype(np.float64)
    u = np.flatnonzero(obj.union())
    n_blocks = -(-u.size // 256)
    pos = np.full(obj.n_voxels, -1, dtype=np.int64)
    pos[u] = np.arange(u.size)
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for t, (kind, roi, weight, level) in enumerate(obj.terms):
            idx = obj.rois[roi]
            wn = weight / float(idx.size)
            dv = t64[idx]
            if kind == R.MEAN:
                phi_t = dv
            elif kind in (D.MAX_DVH, D.MIN_DVH):
                Dv = float(obj.dose_at_volume(r, [(roi, obj.vfrac[t])])[0])
                inside = (dv > level) & (dv <= Dv) if kind == D.MAX_DVH else (dv < level) & (dv >= Dv)
                x = np.where(np.isnan(dv), dv, np.where(inside, dv - level, 0.0))
                phi_t = x * x
            else:
                assert kind in (R.SQ_DEVIATION, R.SQ_OVERDOSE, R.SQ_UNDERDOSE), kind
                x = dv - level
                if kind == R.SQ_OVERDOSE:
                    x = np.where(x < 0.0, 0.0, x)
                elif kind == R.SQ_UNDERDOSE:
                    x = np.where(x > 0.0, 0.0, x)
                phi_t = x * x
            phi = np.zeros(n_blocks * 256)
            phi[pos[idx]] = phi_t
            w = LB._butterfly(phi.reshape(-1, 64)).reshape(n_blocks, 4)
            blocks = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
            acc = float(LB._butterfly(LB._lane_sums(LB._pad(blocks, 64).reshape(1, -1)))[0])
            out.append(float(wn * acc))
    return out


def tree_value(obj, r):
    f = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for v in tree_terms(obj, r):
            f = f + v
    return float(f)


class LbfgsTermsReference(LB.LbfgsReference):
    """The tree-order restatement on a DvhReferenceObjective with plain and DVH terms: the value of a trial is that of its float32
    rounding."""

    def value(self, t):
        assert self.tree
        with np.errstate(over="ignore", invalid="ignore"):
            return tree_value(self.obj, np.asarray(t).astype(np.float32))


class LbfgsValueReference(LB.LbfgsReference):
    """The tree-order restatement whose trial values come from value_of(float32 volume) -> float."""

    def __init__(self, objective, matvec, rmatvec, w0, value_of, **kw):
        super().__init__(objective, matvec, rmatvec, w0, tree=True, **kw)
        self.value_of = value_of

    def value(self, t):
        with np.errstate(over="ignore", invalid="ignore"):
            return float(self.value_of(np.asarray(t).astype(np.float32)))
