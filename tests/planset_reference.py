"""The numpy restatement of what a plan set adds to the plain optimiser (include/rtd.h, the plan-set block).
A test helper, not product code.

blend: rtd_planset_blend's arithmetic, float64 products and sums in plan order from 0.0, rounded once to float32.
ReferenceSet: P ReferenceOptimizers of tests/optimizer_reference.py side by side, one per variant table, each on an objective of the
same ROIs: a plan set is nothing else, and no plan sees another."""
import numpy as np

import optimizer_reference as R


def blend(ws, coeffs):
    """ws: the plans' weight arrays (equal shapes, float32); coeffs: one finite coefficient >= 0 per plan -> float32 of ws' shape."""
    ws = [np.asarray(w, dtype=np.float32) for w in ws]
    coeffs = [float(c) for c in coeffs]
    assert len(ws) == len(coeffs) >= 1 and all(w.shape == ws[0].shape for w in ws), "one coefficient per plan, plans of one shape"
    assert all(np.isfinite(c) and c >= 0.0 for c in coeffs), "coefficients must be finite and >= 0: %r" % (coeffs,)
    acc = np.zeros(ws[0].shape, dtype=np.float64)
    for c, w in zip(coeffs, ws):
        acc = acc + np.float64(c) * w.astype(np.float64)              # (numpy does not contract)
    return acc.astype(np.float32)


def variant_objective(base, variant):
    """A ReferenceObjective with the ROIs of `base` and the terms of one variant table [(kind, roi, weight, level), ...]."""
    assert len(variant) == len(base.terms), "a variant has one entry per term: %d vs %d" % (len(variant), len(base.terms))
    o = R.ReferenceObjective(base.n_voxels)
    for r in base.rois:
        o.add_roi(r)
    for (kind, roi, weight, level), (k0, r0, _, _) in zip(variant, base.terms):
        assert (kind, roi) == (k0, r0), "a variant keeps the kind and the ROI of its term: %r vs %r" % ((kind, roi), (k0, r0))
        o.add_term(kind, roi, weight, level)
    return o


class ReferenceSet:
    def __init__(self, base, variants, matvec, rmatvec, w0s, **kw):
        """w0s: one start vector per plan."""
        assert len(variants) == len(w0s), "one start vector per plan"
        self.plans = [R.ReferenceOptimizer(variant_objective(base, v), matvec, rmatvec, w0, **kw) for v, w0 in zip(variants, w0s)]

    def run(self, n):
        for p in self.plans:
            p.run(n)
        return self

    def blend(self, coeffs, best=True):
        return blend([p.w_best if best else p.w for p in self.plans], coeffs)
