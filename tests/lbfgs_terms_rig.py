"""The rig of tests/test_gpu_lbfgs_terms.py: lbfgs_rig.LbfgsRig with objectives of every term kind, L-BFGS optimisers from
rtd_optimizer_create_lbfgs_ex (plain or on the compact matrices), a look at the line search's own arrays, and the comparison of one
iteration's K trials with rtd_objective_eval, rtd_objective_dose_at_volume and rtd_objective_eud on the float32 trial volumes. A plain
module (no tests)."""
import numpy as np

import eud_reference as E
import lbfgs_terms_reference as LT
from gpu_support import bits
from lbfgs_rig import LbfgsRig, lbfgs_options, step_and_compare
from raytracedicom_amd import abi

MAXT = abi.RTD_OBJ_MAX_TERMS


class LbfgsTermsRig(LbfgsRig):
    def __init__(self, engine, scn):
        super().__init__(engine, scn)
        self.compact = False
        self.dVal = self.alloc(4 * self.nvox)
        self.dGrad = self.alloc(4 * max(self.sizes))

    # -- objectives -------------------------------------------------------------------------------------------------------------
    def set_terms(self, terms, rois):
        """terms: ("plain", kind, roi, weight, level) | ("dvh", kind, roi, weight, level, volume_fraction) | ("eud", kind, roi, weight,
        level, exponent), over the ROI masks or index lists `rois`: the engine's objective (self.obj) and an EudReferenceObjective
        (self.ref). The optimisers on the objective it replaces are destroyed with it."""
        for o in self.opts:
            o.destroy()
        self.opts = []
        self.obj.destroy()
        self.obj = self.eng.create_objective(self.dims)
        self.ref = E.EudReferenceObjective(self.nvox)
        self.eng.device_zero(self.dG, 4 * self.nvox)                  # (an evaluation writes the voxels of its own ROIs only)
        for m in rois:
            self.obj.add_roi(m)
            self.ref.add_roi(m)
        add = {"plain": "add_term", "dvh": "add_dvh_term", "eud": "add_eud_term"}
        for t in terms:
            getattr(self.obj, add[t[0]])(*t[1:])
            getattr(self.ref, add[t[0]])(*t[1:])

    def mixed_terms(self):
        """On the rig's target (ROI 0) and the other voxels with rows (ROI 1): a plain term, a MAX_DVH, two MIN_DVH on the same ROI with
        different fractions, an SQ_MAX_EUD with a = 4 and an SQ_MIN_EUD with a negative exponent."""
        L = self.level
        return [("plain", E.SQ_DEVIATION, 0, 1.0, L), ("dvh", E.MAX_DVH, 1, 2.0, 0.3 * L, 0.1), ("dvh", E.MIN_DVH, 0, 5.0, 0.95 * L, 0.98),
                ("dvh", E.MIN_DVH, 0, 2.0, 0.9 * L, 0.5), ("eud", E.SQ_MAX_EUD, 1, 1.0, 0.3 * L, 4.0), ("eud", E.SQ_MIN_EUD, 0, 1.0, L, -8.0)]

    def set_mixed(self):
        self.set_terms(self.mixed_terms(), [self.ref.rois[0], self.ref.rois[1]])

    # -- optimisers and products ------------------------------------------------------------------------------------------------
    def make_compact(self, release_plain=False):
        """The compact form of every field's matrix; from here the rig's own products (product, dose_of) are the compact ones."""
        for f in self.fields:
            f.dose_influence_compact(release_plain=release_plain)
        self.compact = True

    def lbfgs_ex(self, start=None, compact=None, **kw):
        o = self.eng.create_lbfgs_optimizer_ex(self.fields, self.obj, lbfgs_options(**kw) if kw else None, compact=self.compact if compact is None else compact)
        self.opts.append(o)
        if start is not None:
            self.set_weights(o, start)
        return o

    def dose_of(self, ws, dDose):
        if not self.compact:
            return super().dose_of(ws, dDose)
        self.eng.device_zero(dDose, 4 * self.nvox)
        for f, w in zip(self.fields, ws):
            d = self.alloc(w.nbytes, zero=False)
            self.eng.to_device(d, np.ascontiguousarray(w, dtype=np.float32))
            f.dose_influence_apply_compact(d, dDose, init=False)
        self.eng.sync()

    def gradient_of(self, g):
        """The concatenated Dij_f^T g of the host voxel gradient g through the public products (compact ones on a compact rig)."""
        self.eng.to_device(self.dVal, np.ascontiguousarray(g, dtype=np.float32))
        out = []
        for f, s in zip(self.fields, self.shapes):
            (f.dose_influence_apply_t_compact if self.compact else f.dose_influence_apply_t)(self.dVal, self.dGrad)
            o = np.empty(int(np.prod(s)), dtype=np.float32)
            self.eng.to_host(o, self.dGrad)
            out.append(o)
        return np.concatenate(out)

    # -- the line search's arrays -----------------------------------------------------------------------------------------------
    def line(self, o):
        self.eng.sync()
        b = o.lbfgs_line_buffers()
        K = int(b.n_trials)
        out = {"K": K, "n_terms": int(b.n_terms), "d0": self.volume(b.d0), "d1": self.volume(b.d1), "thr": None, "eud": None,
               "coupled": bool(b.thresholds)}
        assert bool(b.thresholds) == bool(b.eud), "the threshold and EUD pointers are not both set or both NULL"
        if b.thresholds:
            out["thr"] = self._host(b.thresholds, K * MAXT, np.float32).reshape(K, MAXT)
            out["eud"] = self._host(b.eud, K * MAXT * 3, np.float64).reshape(K, MAXT, 3)
        return out

    def upload(self, r):
        self.eng.to_device(self.dVal, np.ascontiguousarray(r, dtype=np.float32))
        return self.dVal

    def value_of(self, r):
        """rtd_objective_eval on the uploaded float32 volume -> values[0]."""
        return float(self.obj.eval(self.upload(r), self.dG)[0])

    def value_restatement(self, w0, **kw):
        return LT.LbfgsValueReference(self.ref, self.matvec, self.rmatvec, w0, self.value_of, **kw)

    def terms_restatement(self, w0, **kw):
        return LT.LbfgsTermsReference(self.ref, self.matvec, self.rmatvec, w0, tree=True, **kw)


def _same(a, b):
    """Bit for bit; two NaNs count as the same (the sign and payload of a NaN that arithmetic produces are not specified)."""
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def _trial_mismatches(rig, ln, lb, k, r):
    """What of trial k's device results differs from the evaluation, the selection and the power sums on the float32 volume r."""
    p = rig.upload(r)
    vals = rig.obj.eval(p, rig.dG)
    print("  trial %d: F %.17g, eval %.17g" % (k, lb["trial_values"][k], vals[0]))
    bad = []
    if not _same(np.array([lb["trial_values"][k]]), vals[:1]):
        bad.append("F_%d = %r is not rtd_objective_eval(r_%d) = %r" % (k, lb["trial_values"][k], k, vals[0]))
    finite = not np.isnan(r).any()
    for t, (kind, roi, weight, level) in enumerate(rig.ref.terms):
        if t in rig.ref.vfrac:
            q = [(roi, rig.ref.vfrac[t])]
            if not _same(ln["thr"][k, t:t + 1], rig.obj.dose_at_volume(p, q)):
                bad.append("thr[%d][%d] against rtd_objective_dose_at_volume" % (k, t))
            if finite and not _same(ln["thr"][k, t:t + 1], rig.ref.dose_at_volume(r, q)):
                bad.append("thr[%d][%d] against numpy" % (k, t))
        elif t in rig.ref.expo:
            if not _same(ln["eud"][k, t, 0:1], rig.obj.eud(p, [(roi, level, rig.ref.expo[t])])):
                bad.append("E of term %d at trial %d" % (t, k))
            if not _same(ln["eud"][k, t, 2:3], vals[1 + t:2 + t]):
                bad.append("the value of term %d at trial %d" % (t, k))
        elif ln["thr"][k, t] != 0.0 or ln["eud"][k, t].any():
            bad.append("entries of the plain term %d at trial %d" % (t, k))
    return bad


def check_trials(rig, opt, d0, d1):
    """After an iteration whose line search ran on d0 and d1: for every k < K, trial_values[k] has the bits of rtd_objective_eval on
    r_k, thr[k][t] is the dose at volume of r_k (numpy's exact order statistic, and the device's rtd_objective_dose_at_volume), the
    E of every EUD term is rtd_objective_eud on r_k and its value the evaluation's. A trial volume that holds NaNs is formed with
    either sign on them: the monotone key sorts a NaN by its bits, and the sign of the NaN that x0 + a (x1 - x0) gives is the
    arithmetic's choice."""
    ln = rig.line(opt)
    lb = opt.lbfgs_report()
    K = ln["K"]
    assert ln["coupled"] and ln["n_terms"] == len(rig.ref.terms), ln["n_terms"]
    assert np.array_equal(bits(ln["d1"]), bits(np.asarray(d1, dtype=np.float32).reshape(-1))), "d1 of the line buffers is not the trial dose"
    for k, r in enumerate(LT.rounded_trials(d0, d1, K)):
        bad = _trial_mismatches(rig, ln, lb, k, r)
        nan = np.isnan(r)
        if bad and nan.any():
            flipped = r.copy()
            flipped.view(np.uint32)[nan] ^= np.uint32(0x80000000)
            bad = _trial_mismatches(rig, ln, lb, k, flipped)
        assert not bad, bad


def step_terms(rig, opt, ref, k, d0, fresh=False):
    """Iteration k through lbfgs_rig.step_and_compare (ref: a restatement whose trial values are those of the rounded trials) and
    check_trials. d0: the tracked dose entering it; it is also what the line buffers show before the call unless the dose is stale
    (fresh: after creation or set_weights). -> (the restatement's record, the new tracked dose)."""
    if not fresh:
        assert np.array_equal(bits(rig.line(opt)["d0"]), bits(np.asarray(d0, dtype=np.float32).reshape(-1))), "iteration %d: d0 of the line buffers" % k
    out, dose = step_and_compare(rig, opt, ref, k, d0)
    if rig.line(opt)["coupled"]:
        check_trials(rig, opt, d0, out["d1"])
    return out, dose


def check_products(rig, opt, out, d0):
    """The iteration's two products against the rig's public calls (the compact ones on a compact rig): grad = Dij^T g of the voxel
    gradient rtd_objective_eval leaves for d0, d1 = Dij w_full."""
    rig.obj.eval(rig.upload(d0), rig.dG)
    g = rig.volume(rig.dG)
    grad = rig.gradient_of(g)
    assert np.array_equal(bits(grad), bits(out["grad"])), "grad is not the rig's product (%d entries differ)" % int((grad != out["grad"]).sum())
    d1 = rig.product(out["w_full"])
    assert np.array_equal(bits(d1), bits(out["d1"])), "d1 is not the rig's product (%d voxels differ)" % int((d1 != out["d1"]).sum())
