"""The numpy restatement of the generalised equivalent uniform dose and the three EUD kinds inside eval (include/rtd.h, DESIGN.md
section 20). A test helper, not product code.

EudReferenceObjective extends dvh_reference.DvhReferenceObjective: an EUD term is a term like the others (it takes the next term
number) with an exponent beside it. The arithmetic is the header's, step by step, in float64: x = d / L clamped to [2^-15, 2^15] (a
NaN stays), p = x ** a, S = sum(p) / N, E = L * S ** (1 / a), y = E - L (one-sided for the MAX and MIN kinds), value = weight * y * y,
K = ((2 * weight * y) * E) / ((L * N) * S), and K * (p / x) per unclamped voxel. numpy's sum has its own order: a sum of N positive
numbers differs from any other order by at most N 2^-52 relative, which is what the tests allow."""
import numpy as np

from dvh_reference import MAX_DVH, MEAN, MIN_DVH, SQ_DEVIATION, SQ_OVERDOSE, SQ_UNDERDOSE, DvhReferenceObjective

SQ_EUD, SQ_MAX_EUD, SQ_MIN_EUD = 6, 7, 8
LO, HI = 2.0 ** -15, 2.0 ** 15


def clamp(d, level):
    """-> (x, clamped) of step 1 for float64 doses d."""
    x = np.asarray(d, dtype=np.float64) / float(level)
    lo, hi = x < LO, x > HI
    x = np.where(lo, LO, x)
    x = np.where(hi, HI, x)
    return x, lo | hi


def geud(d, level, a):
    """Steps 1-3 on the doses of one ROI -> (E, S, x, p, clamped)."""
    with np.errstate(over="ignore", invalid="ignore"):
        x, clamped = clamp(d, level)
        p = np.power(x, float(a))
        S = float(np.sum(p)) / float(x.size)
        E = float(level) * float(np.power(S, 1.0 / float(a)))
    return E, S, x, p, clamped


class EudReferenceObjective(DvhReferenceObjective):
    def __init__(self, n_voxels):
        super().__init__(n_voxels)
        self.expo = {}      # term number -> exponent, for the EUD terms

    def add_eud_term(self, kind, roi, weight, level, exponent):
        assert kind in (SQ_EUD, SQ_MAX_EUD, SQ_MIN_EUD) and 0 <= roi < len(self.rois) and weight > 0 and level > 0
        assert 2.0 ** -4 <= abs(exponent) <= 64.0
        self.expo[len(self.terms)] = float(exponent)
        self.terms.append((int(kind), int(roi), float(weight), float(level)))

    def eud(self, dose, queries):
        """queries: [(roi, level, exponent), ...] -> float64[n]."""
        d = np.asarray(dose).reshape(-1).astype(np.float64)
        return np.array([geud(d[self.rois[roi]], level, a)[0] for roi, level, a in queries], dtype=np.float64)

    def eud_term(self, d, t):
        """Term t on the flat float64 dose d -> (value, contrib per voxel of its ROI, E)."""
        kind, roi, weight, level = self.terms[t]
        idx = self.rois[roi]
        E, S, x, p, clamped = geud(d[idx], level, self.expo[t])
        with np.errstate(over="ignore", invalid="ignore"):
            y = E - level
            if kind == SQ_MAX_EUD:
                y = 0.0 if y < 0.0 else y
            elif kind == SQ_MIN_EUD:
                y = 0.0 if y > 0.0 else y
            value = weight * y * y
            K = ((2.0 * weight * y) * E) / ((level * float(idx.size)) * S)
            contrib = np.where(clamped | (y == 0.0), 0.0, K * (p / x))
        return value, contrib, E

    def eval(self, dose):
        """As DvhReferenceObjective.eval, with the three EUD kinds. Every term is evaluated on its own (the other kinds by the parent,
        with that one term: 0.0 + its contribution, which is exact) and the contributions are added per voxel in term order."""
        d = np.asarray(dose).reshape(-1).astype(np.float64)
        assert d.size == self.n_voxels
        g = np.zeros(self.n_voxels, dtype=np.float64)
        gabs = np.zeros(self.n_voxels, dtype=np.float64)
        values = np.zeros(1 + len(self.terms), dtype=np.float64)
        for t in range(len(self.terms)):
            idx = self.rois[self.terms[t][1]]
            if t in self.expo:
                values[1 + t], contrib, _ = self.eud_term(d, t)
                cabs = np.abs(contrib)
            else:
                one = DvhReferenceObjective(self.n_voxels)
                one.rois = self.rois
                one.terms = [self.terms[t]]
                if t in self.vfrac:
                    one.vfrac = {0: self.vfrac[t]}
                v1, g1, a1 = one.eval(d)
                values[1 + t], contrib, cabs = v1[1], g1[idx], a1[idx]
            g[idx] = g[idx] + contrib
            gabs[idx] = gabs[idx] + cabs
        f = 0.0
        for t in range(len(self.terms)):
            f = f + values[1 + t]
        values[0] = f
        return values, g, gabs


__all__ = ["EudReferenceObjective", "geud", "clamp", "SQ_EUD", "SQ_MAX_EUD", "SQ_MIN_EUD", "LO", "HI", "MAX_DVH", "MIN_DVH", "SQ_DEVIATION",
           "SQ_OVERDOSE", "SQ_UNDERDOSE", "MEAN"]
