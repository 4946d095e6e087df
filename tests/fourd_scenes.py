"""The scene and rig of tests/test_gpu_fourd_optimizer.py: a plain module beside gpu_support.py, under the same rule — test files
import from here, never from each other — and with a message on every assert.

The scene: the 96^3 heterogeneous phantom with two fields, three breathing phases (the CT shifted by 0, 2 and 4 voxels along z, every
phase's fields created and their matrices computed under that phase's CT), a reference grid of 80 x 96 x 72 voxels with an
index-to-world of its own, and per phase a smooth random displacement field of 13 x 11 x 9 nodes (a few mm) plus the phase's shift."""
import numpy as np

import fourd_reference as fr
import optimizer_reference as OR
from gpu_support import bits, hetero_scene, options, switches
from raytracedicom_amd import abi, fourd

F = np.float32
SHIFTS = (0, 2, 4)                                                    # voxels along z
REF_DIMS = (80, 96, 72)
DVF_DIMS = (13, 11, 9)
PHASE_WEIGHTS = (0.5, 0.3, 0.2)


def shape_of(dims):
    return (dims[2], dims[1], dims[0])


class FourDRig:
    def __init__(self, engine, synth):
        self.engine = engine
        scn = hetero_scene(synth, 96, (0.0, 90.0))
        self.scn = scn
        self.eng = engine.Engine(0)
        self.eng.set_options(options(0.0))
        self.eng.set_luts(scn.luts)
        self.dims = tuple(scn.dims)
        self.nvox = int(np.prod(self.dims))
        self.ref_dims = REF_DIMS
        self.nref = int(np.prod(REF_DIMS))
        voxel = scn.spacing[0]
        self.phase_to_world = (np.diag(scn.spacing), np.array([-128.0, -128.0, -106.0]))
        ref_spacing = (3.0, voxel, 3.2)
        self.ref_to_world = (np.diag(ref_spacing), np.array([-118.0, -128.0, -100.0]))
        extent = [s * (n - 1) for s, n in zip(ref_spacing, REF_DIMS)]
        self.dvf_to_world = (np.diag([e / (n - 1) for e, n in zip(extent, DVF_DIMS)]), self.ref_to_world[1])
        self.sfields, self.smats = [], []
        for shift in SHIFTS:                                          # (the CT of the phase stands while its fields are created and computed)
            self.eng.set_ct(np.roll(scn.ct, shift, axis=0))
            fs = [self.eng.create_field(b, self.dims) for b in scn.beams]
            self.sfields.append(fs)
            self.smats.append([f.dose_influence() for f in fs])
        self.fields = self.sfields[0]
        self.shapes = [b.spotWeights.shape for b in scn.beams]
        self.sizes = [int(np.prod(s)) for s in self.shapes]
        self.offs = np.cumsum([0] + self.sizes)
        self.w0 = np.concatenate([np.asarray(b.spotWeights, dtype=F).reshape(-1) for b in scn.beams])
        rng = np.random.default_rng(77)
        self.dvfs = []
        for shift in SHIFTS:
            d = (3.0 * rng.standard_normal((3,) + shape_of(DVF_DIMS))).astype(F)
            d[2] += F(shift * voxel)                                  # the matching place of phase p lies shift voxels further along z
            self.dvfs.append(d)
        self.warps = fourd.phase_warps(self.eng, self.ref_to_world, self.phase_to_world, self.dvfs, self.dvf_to_world)
        self.still = fourd.phase_warps(self.eng, self.ref_to_world, self.phase_to_world, [np.zeros_like(d) for d in self.dvfs], self.dvf_to_world)
        self.opts, self.objs, self.bufs = [], [], []
        # the loop's volumes: per phase a dose and a g volume, acc and g on the reference grid, the workspace, a gradient
        P = len(SHIFTS)
        self.dDose = [self.alloc(4 * self.nvox) for _ in range(P)]
        self.dGs = [self.alloc(4 * self.nvox) for _ in range(P)]
        self.dAcc, self.dG = self.alloc(4 * self.nref), self.alloc(4 * self.nref)
        self.nws = self.eng.warp_t_phases_workspace_bytes(self.dims, P)
        self.dWs = self.alloc(self.nws)
        self.dGrad = self.alloc(4 * max(self.sizes))
        self.obj = self.plan_objective()

    def alloc(self, nbytes, zero=True):
        p = self.eng.device_alloc(nbytes)
        self.bufs.append(p)
        if zero:
            self.eng.device_zero(p, nbytes)
        return p

    def volume(self, ptr, n):
        out = np.empty(n, dtype=F)
        self.eng.to_host(out, ptr)
        return out

    def phase_doses(self, w, phases=None):
        """dose_p = zero, then apply(init = 0) per field in list order, into dDose[p], for the flat weight vector w."""
        for p in (range(len(SHIFTS)) if phases is None else phases):
            self.eng.device_zero(self.dDose[p], 4 * self.nvox)
            for f, a, b in zip(self.sfields[p], self.offs, self.offs[1:]):
                d = self.alloc(4 * (b - a), zero=False)
                self.eng.to_device(d, np.ascontiguousarray(w[a:b], dtype=F))
                f.dose_influence_apply(d, self.dDose[p], init=False)

    def accumulated(self, w, warps=None, weights=PHASE_WEIGHTS):
        """The accumulated dose of w on the reference grid through the public calls -> flat float32."""
        self.phase_doses(w)
        self.eng.warp_sum_device(self.dDose, self.dims, list(self.warps if warps is None else warps), weights, self.dAcc, self.ref_dims)
        return self.volume(self.dAcc, self.nref)

    def rois(self):
        """Target: where the accumulated dose of the start weights exceeds half its maximum; other: the rest of where it is positive."""
        acc = self.accumulated(self.w0)
        target = acc > 0.5 * acc.max()
        other = (acc > 0) & ~target
        assert target.sum() > 100 and other.sum() > 1000, "the scene has no target: %d, %d" % (target.sum(), other.sum())
        return acc, target, other

    def plan_objective(self):
        """Section 12's terms on the reference grid, the target level 1.1 times the start's mean there."""
        acc, target, other = self.rois()
        L = 1.1 * float(acc[target].mean())
        obj = self.eng.create_objective(self.ref_dims)
        self.objs.append(obj)
        obj.add_roi(target)
        obj.add_roi(other)
        for t in ((OR.SQ_DEVIATION, 0, 1.0, L), (OR.SQ_UNDERDOSE, 0, 5.0, 0.95 * L), (OR.SQ_OVERDOSE, 1, 1.0, 0.3 * L), (OR.MEAN, 1, 1e-3 * L, 0.0)):
            obj.add_term(*t)
        return obj

    def dvh_eud_objective(self):
        acc, target, other = self.rois()
        L = 1.1 * float(acc[target].mean())
        obj = self.eng.create_objective(self.ref_dims)
        self.objs.append(obj)
        obj.add_roi(target)
        obj.add_roi(other)
        obj.add_term(OR.SQ_DEVIATION, 0, 1.0, L)
        obj.add_dvh_term(abi.RTD_OBJ_MIN_DVH, 0, 5.0, 0.95 * L, 0.98)
        obj.add_eud_term(abi.RTD_OBJ_SQ_MAX_EUD, 1, 2.0, 0.1 * L, 4.0)
        return obj

    def optimizer(self, obj=None, warps=None, weights=PHASE_WEIGHTS, phases=None, no_batch=False):
        sf = self.sfields if phases is None else [self.sfields[p] for p in phases]
        ws = list(self.warps if warps is None else warps)
        ws = ws if phases is None else [ws[p] for p in phases]
        with switches(**({"RTD_4D_NO_BATCH": "1"} if no_batch else {})):
            o = self.eng.create_4d_optimizer(sf, ws, self.obj if obj is None else obj, weights)
        self.opts.append(o)
        return o

    def weights(self, o, best=False):
        return [o.weights(i, best=best) for i in range(len(self.fields))]

    def python_loop(self, obj, n_it, warps=None, weights=PHASE_WEIGHTS):
        """The iteration driven from here with the public calls: apply per field and phase, warp_sum, Objective.eval,
        warp_dose_t_phases, apply_t, the float64 combine, then ReferenceOptimizer.advance -> the ReferenceOptimizer."""
        ws = list(self.warps if warps is None else warps)
        ref = OR.ReferenceOptimizer(None, None, None, self.w0)
        self.eng.device_zero(self.dG, 4 * self.nref)                  # (the evaluation writes g on the ROI union only)
        for _ in range(n_it):
            self.phase_doses(ref.w)
            self.eng.warp_sum_device(self.dDose, self.dims, ws, weights, self.dAcc, self.ref_dims)
            vals = obj.eval(self.dAcc, self.dG)
            self.eng.warp_dose_t_phases_device(self.dG, self.ref_dims, ws, weights, self.dGs, self.dims, self.dWs, self.nws)
            grads = []
            for p, fs in enumerate(self.sfields):
                parts = []
                for f, n in zip(fs, self.sizes):
                    f.dose_influence_apply_t(self.dGs[p], self.dGrad)
                    parts.append(self.volume(self.dGrad, n))
                grads.append(np.concatenate(parts))
            ref.advance(float(vals[0]), fr.combine(grads))
        return ref

    def equals_loop(self, o, ref):
        rep, hist = o.result()
        want = np.array(ref.history, dtype=np.float64)
        assert hist.size == want.size and np.array_equal(bits(hist), bits(want)), "history: device %s, loop %s" % (hist, want)
        got_w = np.concatenate([x.reshape(-1) for x in self.weights(o)])
        got_b = np.concatenate([x.reshape(-1) for x in self.weights(o, best=True)])
        assert np.array_equal(bits(got_w), bits(ref.w)), "weights differ in %d of %d" % ((bits(got_w) != bits(ref.w)).sum(), got_w.size)
        assert np.array_equal(bits(got_b), bits(ref.w_best)), "best weights differ in %d of %d" % ((bits(got_b) != bits(ref.w_best)).sum(), got_b.size)
        return rep, hist

    def drop(self, o):
        o.destroy()
        self.opts.remove(o)

    def close(self):
        for o in self.opts:
            o.destroy()
        for o in self.objs:
            o.destroy()
        for p in self.bufs:
            self.eng.device_free(p)
        self.warps.free()
        self.still.free()
        for fs in self.sfields:
            for f in fs:
                f.destroy()
        self.eng.close()
