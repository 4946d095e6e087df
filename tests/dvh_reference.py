"""The numpy restatement of the dose-volume part of the objective (include/rtd.h): dose at volume, the
cumulative histogram and the two DVH-point kinds inside eval. A test helper, not product code.

DvhReferenceObjective extends optimizer_reference.ReferenceObjective: a DVH term is a term like the others (it takes the next term
number) with a volume fraction beside it. D_v is np.sort(d)[::-1][k - 1] on the float32 doses of the ROI with
k = min(N, max(1, ceil(v * N))): on finite doses without -0 numpy's order is the order of the monotone key."""
import math

import numpy as np

from optimizer_reference import MEAN, SQ_DEVIATION, SQ_OVERDOSE, SQ_UNDERDOSE, ReferenceObjective

MAX_DVH, MIN_DVH = 4, 5


def rank(v, n):
    """The k of 'k-th largest of n' for a volume fraction v in (0, 1]."""
    return min(int(n), max(1, int(math.ceil(float(v) * float(n)))))


class DvhReferenceObjective(ReferenceObjective):
    def __init__(self, n_voxels):
        super().__init__(n_voxels)
        self.vfrac = {}     # term number -> volume fraction, for the DVH terms

    def add_dvh_term(self, kind, roi, weight, level, volume_fraction):
        assert kind in (MAX_DVH, MIN_DVH) and 0 <= roi < len(self.rois) and weight > 0 and 0.0 < volume_fraction <= 1.0
        self.vfrac[len(self.terms)] = float(volume_fraction)
        self.terms.append((int(kind), int(roi), float(weight), float(level)))

    def dose_at_volume(self, dose, queries):
        """queries: [(roi, volume_fraction), ...] -> float32[n]."""
        d = np.asarray(dose, dtype=np.float32).reshape(-1)
        out = np.empty(len(queries), dtype=np.float32)
        for q, (roi, v) in enumerate(queries):
            dv = d[self.rois[roi]]
            out[q] = np.sort(dv)[::-1][rank(v, dv.size) - 1]
        return out

    def dvh(self, dose, n_bins, dose_max):
        """-> uint32[rois, n_bins]: voxels of the ROI with float64(d) >= (b * dose_max) / n_bins."""
        d = np.asarray(dose, dtype=np.float32).reshape(-1).astype(np.float64)
        edges = np.arange(n_bins, dtype=np.float64) * float(dose_max) / float(n_bins)
        out = np.empty((len(self.rois), n_bins), dtype=np.uint32)
        for r, idx in enumerate(self.rois):
            out[r] = (d[idx][:, None] >= edges[None, :]).sum(0)
        return out

    def eval(self, dose):
        """As ReferenceObjective.eval, with the two DVH kinds: x = d - level where the voxel lies between the level and the term's
        dose at volume D of this dose (D held constant), 0 elsewhere, a NaN dose kept. A float64 dose (host
        products) is selected from as it is; a float32 dose gives exactly what dose_at_volume gives."""
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
                    if kind in (MAX_DVH, MIN_DVH):
                        D = float(np.sort(dv)[::-1][rank(self.vfrac[t], dv.size) - 1])     # (of a float32 dose: the float32 selection)
                        inside = (dv > level) & (dv <= D) if kind == MAX_DVH else (dv < level) & (dv >= D)
                        x = np.where(np.isnan(dv), dv, np.where(inside, dv - level, 0.0))
                    else:
                        x = dv - level
                        if kind == SQ_OVERDOSE:
                            x = np.where(x < 0.0, 0.0, x)
                        elif kind == SQ_UNDERDOSE:
                            x = np.where(x > 0.0, 0.0, x)
                    phi = x * x
                    contrib = c * x
                g[idx] = g[idx] + contrib
                gabs[idx] = gabs[idx] + np.abs(contrib)
                values[1 + t] = wn * float(np.sum(phi))
            f = 0.0
            for t in range(len(self.terms)):
                f = f + values[1 + t]
            values[0] = f
        return values, g, gabs


__all__ = ["DvhReferenceObjective", "rank", "MAX_DVH", "MIN_DVH", "SQ_DEVIATION", "SQ_OVERDOSE", "SQ_UNDERDOSE", "MEAN"]
