"""The numpy restatement of the voxel-wise worst case over error scenarios (include/rtd.h "The voxel-wise worst case over error
scenarios"): the extremes of a voxel over the scenario doses (extremes), the composite evaluation
(eval_voxelwise) and the whole iteration on S pairs of callables (VoxelwiseReferenceOptimizer). A test helper, not product code.

It follows the header line by line: the doses compared in the precision they come in (float32 volumes from the device; the float64
products of a host matrix stay float64, as optimizer_reference keeps them), the lowest index winning a tie, a NaN becoming both extremes;
per voxel the terms in term order, one float64 sum per receiving scenario, and a single sum when one scenario holds both extremes.
Steps 4-7 of the plain iteration are optimizer_reference.ReferenceOptimizer.advance; step 5 is robust_reference.combine."""
import numpy as np

import optimizer_reference as R
import robust_reference as Q


def extremes(doses):
    """doses: [S][n] -> (lo, s_lo, hi, s_hi), lo / hi in the doses' own dtype (in which they are compared: the device's volumes are
    float32) with the bits of the scenario that supplied them."""
    d = np.asarray(doses)
    assert d.ndim == 2 and d.shape[0] >= 1
    S, n = d.shape
    hi, lo = d[0].copy(), d[0].copy()
    s_hi, s_lo = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for s in range(1, S):
            up, down = d[s] > hi, d[s] < lo                           # (strict: the lower index keeps a tie, -0 == +0)
            hi[up], s_hi[up] = d[s][up], s
            lo[down], s_lo[down] = d[s][down], s
    nan = np.isnan(d)
    any_nan = nan.any(axis=0)
    first = np.argmax(nan, axis=0)                                    # the lowest scenario with a NaN
    cols = np.flatnonzero(any_nan)
    hi[cols] = lo[cols] = d[first[cols], cols]
    s_hi[cols] = s_lo[cols] = first[cols]
    return lo, s_lo, hi, s_hi


def eval_voxelwise(objective, doses):
    """objective: optimizer_reference.ReferenceObjective; doses: [S][n_voxels].
    -> (values float64[1 + terms], G float64[S][n_voxels] NOT yet rounded to float32 (0 where nothing is received and outside the
    union), active: bit s set iff float32(G[s]) has an entry != 0 inside the union, Gabs float64[S][n_voxels] = the sum of |c_t x_t|
    behind every entry of G: the scale of its rounding bound)."""
    d = np.asarray(doses)
    S, n = d.shape
    assert n == objective.n_voxels
    lo, s_lo, hi, s_hi = extremes(d)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    two = s_hi != s_lo
    g_hi, g_lo = np.zeros(n), np.zeros(n)                              # the two sums of a voxel; g_lo is used only where `two`
    a_hi, a_lo = np.zeros(n), np.zeros(n)
    values = np.zeros(1 + len(objective.terms), dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for t, (kind, roi, weight, level) in enumerate(objective.terms):
            idx = objective.rois[roi]
            nn = float(idx.size)
            c, wn = 2.0 * weight / nn, weight / nn
            h, l = hi[idx], lo[idx]
            if kind == R.MEAN:
                phi = h
                g_hi[idx] = g_hi[idx] + wn
                a_hi[idx] = a_hi[idx] + abs(wn)
            else:
                if kind == R.SQ_UNDERDOSE:
                    low = np.ones(idx.size, dtype=bool)
                elif kind == R.SQ_DEVIATION:
                    low = ~(np.abs(h - level) >= np.abs(l - level))
                else:
                    low = np.zeros(idx.size, dtype=bool)
                x = np.where(low, l, h) - level
                if kind == R.SQ_OVERDOSE:
                    x = np.where(x < 0.0, 0.0, x)
                elif kind == R.SQ_UNDERDOSE:
                    x = np.where(x > 0.0, 0.0, x)
                phi = x * x
                contrib = c * x
                to_lo = low & two[idx]
                a, b = idx[to_lo], idx[~to_lo]
                g_lo[a] = g_lo[a] + contrib[to_lo]
                g_hi[b] = g_hi[b] + contrib[~to_lo]
                a_lo[a] = a_lo[a] + np.abs(contrib[to_lo])
                a_hi[b] = a_hi[b] + np.abs(contrib[~to_lo])
            values[1 + t] = wn * float(np.sum(phi))
        f = 0.0
        for t in range(len(objective.terms)):
            f = f + values[1 + t]
        values[0] = f
    union = np.flatnonzero(objective.union())
    G, Gabs = np.zeros((S, n)), np.zeros((S, n))
    G[s_hi[union], union] = g_hi[union]
    Gabs[s_hi[union], union] = a_hi[union]
    u2 = union[two[union]]
    G[s_lo[u2], u2] = g_lo[u2]
    Gabs[s_lo[u2], u2] = a_lo[u2]
    active = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(S):
            if np.any(G[s].astype(np.float32) != 0):
                active |= 1 << s
    return values, G, active, Gabs


def decide(F, active, S):
    """Step 3 -> (values float64[S] = F, lambdas float64[S], worst)."""
    lam = np.array([1.0 if (active >> s) & 1 else 0.0 for s in range(S)])
    on = np.flatnonzero(lam)
    return np.full(S, float(F)), lam, int(on[0]) if on.size else 0


def combine(grads, lambdas, n, ft=np.float32):
    """robust_reference.combine; +0 everywhere when no scenario is active."""
    if not np.any(np.asarray(lambdas) != 0.0):
        return np.zeros(n, dtype=ft)
    return Q.combine(grads, lambdas, ft)


class VoxelwiseReferenceOptimizer(R.ReferenceOptimizer):
    """matvecs / rmatvecs: one pair of callables per scenario, as robust_reference.RobustReferenceOptimizer. scenario_values / lambdas
    / worst belong to the iterate that entered the last step, as on the device."""

    def __init__(self, objective, matvecs, rmatvecs, w0, **kw):
        super().__init__(objective, None, None, w0, **kw)
        self.matvecs, self.rmatvecs = list(matvecs), list(rmatvecs)
        self.scenario_values = self.lambdas = None
        self.worst = 0

    def composite(self, w):
        """F of the composite at w."""
        return float(eval_voxelwise(self.obj, np.stack([np.asarray(mv(w)).reshape(-1) for mv in self.matvecs]))[0][0])

    def step(self, doses=None, grads=None):
        """One iteration; doses [S][n_voxels] and grads [S][n] (rows of inactive scenarios are not read) replace the products when
        given."""
        S = len(self.matvecs)
        if doses is None:
            doses = np.stack([np.asarray(mv(self.w)).reshape(-1) for mv in self.matvecs])
        values, G, active, _ = eval_voxelwise(self.obj, doses)
        self.scenario_values, self.lambdas, self.worst = decide(values[0], active, S)
        if grads is None:
            with np.errstate(over="ignore", invalid="ignore"):
                grads = [np.asarray(rmv(G[s].astype(self.ft))).astype(self.ft) if self.lambdas[s] else None for s, rmv in enumerate(self.rmatvecs)]
        return self.advance(float(values[0]), combine(grads, self.lambdas, self.w.size, self.ft))
