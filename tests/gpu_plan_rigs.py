"""The rigs of the plan-optimiser tests (tests/test_gpu_optimizer.py, _dvh, _robust, _voxelwise, _plan_sizes): a plain module beside
gpu_support.py, under the same rule — test files import from here, never from each other — and with a message on every assert."""
import numpy as np

import dvh_reference as D
import optimizer_reference as R
from gpu_support import bits, options, switches
from raytracedicom_amd import abi, robust

SHIFT_MM = 5.0
FACTORS = (0.965, 1.035)
MODES = (abi.RTD_ROBUST_EXPECTED, abi.RTD_ROBUST_WORST_CASE)


class OptimizerRig:
    """One engine, the scenario's fields with their matrices, and the plan objective of the convergence test: the target is where
    Dij w_true exceeds half its maximum (SQ_DEVIATION to its mean there, weight 1, + SQ_UNDERDOSE at 95 %, weight 5), the other voxels
    that have rows carry SQ_OVERDOSE at 30 % (weight 1) + MEAN (weight 1e-3 x level)."""

    def __init__(self, engine, scn, pure_overdose=False):
        self.engine = engine
        self.eng = engine.Engine(0)
        self.eng.set_options(options(0.0))
        self.eng.set_luts(scn.luts)
        self.eng.set_ct(scn.ct)
        self.dims = tuple(scn.dims)
        self.nvox = int(np.prod(self.dims))
        self.fields = [self.eng.create_field(b, self.dims) for b in scn.beams]
        self.mats = [f.dose_influence() for f in self.fields]
        self.shapes = [b.spotWeights.shape for b in scn.beams]
        self.sizes = [int(np.prod(s)) for s in self.shapes]
        self.w_true = [(40.0 + 120.0 * np.random.default_rng(21 + i).random(s)).astype(np.float32) for i, s in enumerate(self.shapes)]
        dose_true = sum(d.matvec(w) for d, w in zip(self.mats, self.w_true))
        has = sum(np.bincount(d.indices, minlength=self.nvox) for d in self.mats) > 0
        target = dose_true > 0.5 * dose_true.max()
        other = has & ~target
        self.level = float(dose_true[target].mean())
        self.obj = self.eng.create_objective(self.dims)
        self.ref = R.ReferenceObjective(self.nvox)
        if pure_overdose:
            terms = [(R.SQ_OVERDOSE, 0, 1.0, 0.3 * self.level)]
            rois = [has]
        else:
            terms = [(R.SQ_DEVIATION, 0, 1.0, self.level), (R.SQ_UNDERDOSE, 0, 5.0, 0.95 * self.level),
                     (R.SQ_OVERDOSE, 1, 1.0, 0.3 * self.level), (R.MEAN, 1, 1e-3 * self.level, 0.0)]
            rois = [target, other]
        for m in rois:
            self.obj.add_roi(m)
            self.ref.add_roi(m)
        for t in terms:
            self.obj.add_term(*t)
            self.ref.add_term(*t)
        self.opts = []
        self.bufs = []

    def alloc(self, nbytes, zero=True):
        p = self.eng.device_alloc(nbytes)
        self.bufs.append(p)
        if zero:
            self.eng.device_zero(p, nbytes)
        return p

    def optimizer(self, start=None, options=None):
        """start: None (the fields' own weights), or a scalar / per-field list of arrays set through set_weights."""
        o = self.eng.create_optimizer(self.fields, self.obj, options)
        self.opts.append(o)
        if start is not None:
            self.set_weights(o, start)
        return o

    def set_weights(self, o, start):
        for i, s in enumerate(self.shapes):
            w = np.full(s, start, dtype=np.float32) if np.isscalar(start) else np.ascontiguousarray(start[i], dtype=np.float32)
            d = self.alloc(w.nbytes, zero=False)
            self.eng.to_device(d, w)
            o.set_weights(i, d)
        self.eng.sync()

    def weights(self, o, best=False):
        return [o.weights(i, best=best) for i in range(len(self.fields))]

    def volume(self, ptr):
        out = np.empty(self.nvox, dtype=np.float32)
        self.eng.to_host(out, ptr)
        return out

    def dose_of(self, ws, dDose):
        """Zero, then apply(init = 0) per field in list order, into dDose."""
        self.eng.device_zero(dDose, 4 * self.nvox)
        for f, w in zip(self.fields, ws):
            d = self.alloc(w.nbytes, zero=False)
            self.eng.to_device(d, np.ascontiguousarray(w, dtype=np.float32))
            f.dose_influence_apply(d, dDose, init=False)
        self.eng.sync()

    def matvec(self, w):
        w = np.asarray(w, dtype=np.float64)
        offs = np.cumsum([0] + self.sizes)
        return sum(d.matvec(w[a:b]) for d, a, b in zip(self.mats, offs, offs[1:]))

    def rmatvec(self, g):
        return np.concatenate([d.rmatvec(g) for d in self.mats])

    def close(self):
        for o in self.opts:
            o.destroy()
        self.obj.destroy()
        for p in self.bufs:
            self.eng.device_free(p)
        for f in self.fields:
            f.destroy()
        self.eng.close()


class RobustRig(OptimizerRig):
    """The rig of the optimiser tests (its fields are scenario 0) with four more scenarios of the same beams beside it, every field
    with its matrix. Objectives are the rig's own (section 12) or made here (with DVH terms, as tests/test_gpu_dvh.py makes its plan)."""

    def __init__(self, engine, scn, shift=SHIFT_MM):
        super().__init__(engine, scn)
        self.sfields, self.smats = [self.fields], [self.mats]
        for beams in robust.scenario_beams(scn.beams, [(shift, 0.0, 0.0), (-shift, 0.0, 0.0)]):
            self._add(beams)
        for factor in FACTORS:
            self.eng.set_luts(robust.range_scaled_luts(scn.luts, factor))
            self._add(scn.beams)
        self.eng.set_luts(scn.luts)
        self.S = len(self.sfields)
        self.objs = []
        self.n = sum(self.sizes)

    def _add(self, beams):
        fs = [self.eng.create_field(b, self.dims) for b in beams]
        self.sfields.append(fs)
        self.smats.append([f.dose_influence() for f in fs])

    def dvh_objective(self):
        """The plan of tests/test_gpu_dvh.py on the nominal scenario's dose of w_true."""
        dose_true = self.matvec(np.concatenate([w.reshape(-1) for w in self.w_true]))
        has = sum(np.bincount(d.indices, minlength=self.nvox) for d in self.mats) > 0
        target = dose_true > 0.5 * dose_true.max()
        other = has & ~target
        L = float(dose_true[target].mean())
        d25 = float(np.sort(dose_true[other].astype(np.float32))[::-1][D.rank(0.25, int(other.sum())) - 1])
        obj, ref = self.eng.create_objective(self.dims), D.DvhReferenceObjective(self.nvox)
        self.objs.append(obj)
        for m in (target, other):
            obj.add_roi(m)
            ref.add_roi(m)
        for t in ((R.SQ_DEVIATION, 0, 1.0, L), (D.MIN_DVH, 0, 5.0, 0.95 * L, 0.98), (D.MAX_DVH, 1, 3.0, 0.5 * d25, 0.25)):
            for o in (obj, ref):
                (o.add_dvh_term if len(t) == 5 else o.add_term)(*t)
        return obj, ref

    def margin_objective(self, half_width_mm):
        """The rig's objective (section 12's terms and weights) with the target cut to the voxels within half_width_mm of the beam
        axis across the beam (world x at gantry angle 0; the grid spans 256 mm from -128): a target narrower than the spot pattern,
        so that a plan has spots left to paint a margin with. -> (device, restated)."""
        dose_true = self.matvec(np.concatenate([w.reshape(-1) for w in self.w_true]))
        has = sum(np.bincount(d.indices, minlength=self.nvox) for d in self.mats) > 0
        x = (np.arange(self.nvox) % self.dims[0]) * (256.0 / self.dims[0]) - 128.0
        target = (dose_true > 0.5 * dose_true.max()) & (np.abs(x) <= half_width_mm)
        other = has & ~target
        L = float(dose_true[target].mean())
        obj, ref = self.eng.create_objective(self.dims), R.ReferenceObjective(self.nvox)
        self.objs.append(obj)
        for o in (obj, ref):
            o.add_roi(target)
            o.add_roi(other)
            for t in ((R.SQ_DEVIATION, 0, 1.0, L), (R.SQ_UNDERDOSE, 0, 5.0, 0.95 * L), (R.SQ_OVERDOSE, 1, 1.0, 0.3 * L), (R.MEAN, 1, 1e-3 * L, 0.0)):
                o.add_term(*t)
        return obj, ref

    def robust(self, mode, start=None, probabilities=None, scen=None, obj=None, no_batch=False):
        sf = self.sfields if scen is None else [self.sfields[s] for s in scen]
        with switches(**({"RTD_ROBUST_NO_BATCH": "1"} if no_batch else {})):
            o = self.eng.create_robust_optimizer(sf, self.obj if obj is None else obj, mode, probabilities)
        self.opts.append(o)
        if start is not None:
            self.set_weights(o, start)
        return o

    def all_weights(self, o, best=False):
        return np.concatenate([w.reshape(-1) for w in self.weights(o, best)])

    def scenario_dose_of(self, s, ws, dDose):
        """Zero, then apply(init = 0) per field of scenario s in list order, into dDose."""
        self.eng.device_zero(dDose, 4 * self.nvox)
        for f, w in zip(self.sfields[s], ws):
            d = self.alloc(w.nbytes, zero=False)
            self.eng.to_device(d, np.ascontiguousarray(w, dtype=np.float32))
            f.dose_influence_apply(d, dDose, init=False)
        self.eng.sync()

    def scenario_grad(self, obj, s, dose_ptr, dG, dGrad):
        """rtd_objective_eval on a volume and apply_t of scenario s's fields on its g -> (values, concatenated float32 gradient)."""
        self.eng.device_zero(dG, 4 * self.nvox)
        vals = obj.eval(dose_ptr, dG)
        out = []
        for f, n in zip(self.sfields[s], self.sizes):
            f.dose_influence_apply_t(dG, dGrad)
            g = np.empty(n, dtype=np.float32)
            self.eng.to_host(g, dGrad)
            out.append(g)
        return vals, np.concatenate(out)

    def host_products(self):
        offs = np.cumsum([0] + self.sizes)
        mv = [(lambda w, ms=ms: sum(d.matvec(np.asarray(w, dtype=np.float64)[a:b]) for d, a, b in zip(ms, offs, offs[1:]))) for ms in self.smats]
        rmv = [(lambda g, ms=ms: np.concatenate([d.rmatvec(g) for d in ms])) for ms in self.smats]
        return mv, rmv

    def close(self):
        for o in self.opts:
            o.destroy()
        self.opts = []
        for o in self.objs:
            o.destroy()
        for fs in self.sfields[1:]:
            for f in fs:
                f.destroy()
        super().close()


def same(rig, a, b):
    """Two optimisers with the same report, history, weights and best weights, bit for bit -> (report, history)."""
    ra, ha = a.result()
    rb, hb = b.result()
    assert ra == rb and np.array_equal(bits(ha), bits(hb)), (ra, rb, ha, hb)
    for best in (False, True):
        for x, y in zip(rig.weights(a, best), rig.weights(b, best)):
            assert np.array_equal(bits(x), bits(y)), "%s differ in %d of %d" % ("best weights" if best else "weights", int((bits(x) != bits(y)).sum()), x.size)
    return ra, ha
