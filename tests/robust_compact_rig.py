"""The rig of tests/test_gpu_robust_compact.py: RobustRig (tests/gpu_plan_rigs.py) with a compact form on every field and the compact
calls in place of the plain ones. A plain module beside gpu_plan_rigs.py, under its rule: test files import from here, never from
each other, and every assert carries a message."""
import copy

import numpy as np

import dij_compact_reference as DC
from gpu_plan_rigs import FACTORS, SHIFT_MM, OptimizerRig, RobustRig
from gpu_support import bits, hetero_scene, switches
from raytracedicom_amd import robust, scenarios

F = np.float32


def wide_slice_scene(synth):
    """The wide-slice scene of tests/test_gpu_dij_compact.py: a 64^3 CT under a dose grid of 512 x 256 x 8 voxels, whose slices hold
    131 072 voxels, so the compact CSC side keeps 32-bit rows by itself. -> a scene whose dims are the dose grid's."""
    scn = hetero_scene(synth, 64, [0.0], spots=3, pitch=8.0, layers=1)
    dims = (512, 256, 8)
    s = np.array([dims[0] / 64.0, dims[1] / 64.0, dims[2] / 64.0])
    t = scn.beams[0].gantryToDoseIdx
    m = (s[:, None] * np.asarray(t.m, dtype=np.float64).reshape(3, 3)).astype(F)
    v = (s * np.asarray(t.v, dtype=np.float64).reshape(3) + (s - 1.0) / 2.0).astype(F)   # dose index i = s c + (s - 1) / 2 of CT index c
    out = copy.copy(scn)
    out.beams = [scn.beams[0].replace(gantryToDoseIdx=scenarios.Float3AffineTransform(m, v))]
    out.dims = dims
    return out


class RobustCompactRig(RobustRig):
    """RobustRig's scenarios (0 nominal, 1 and 2 the shifts, 3 and 4 the range factors), of which `scen` are built, in that order; every
    field with its matrix and its compact form. wide: the indices (into the built list) of the scenarios whose compact forms are built
    under RTD_DIJC_ROWS32=1; tree: (G, E) for RTD_DIJC_LANES / RTD_DIJC_PER; compact=False leaves the forms to the caller."""

    def __init__(self, engine, scn, scen=(0, 1, 2, 3, 4), wide=(), tree=None, compact=True, shift=SHIFT_MM):
        OptimizerRig.__init__(self, engine, scn)
        assert scen[0] == 0, "scenario 0 is the rig's own fields"
        self.sfields, self.smats = [self.fields], [self.mats]
        shifted = robust.scenario_beams(scn.beams, [(shift, 0.0, 0.0), (-shift, 0.0, 0.0)])
        for k in scen[1:]:
            if k <= 2:
                self._add(shifted[k - 1])
            else:
                self.eng.set_luts(robust.range_scaled_luts(scn.luts, FACTORS[k - 3]))
                self._add(scn.beams)
                self.eng.set_luts(scn.luts)
        self.S = len(self.sfields)
        self.objs = []
        self.n = sum(self.sizes)
        self.wide, self.tree = tuple(wide), tree
        if compact:
            self.build_compact()

    def build_compact(self, release=False):
        """The compact form of every field (a second call keeps the forms that stand and releases the plain ones, if asked)."""
        env = {} if self.tree is None else {"RTD_DIJC_LANES": str(self.tree[0]), "RTD_DIJC_PER": str(self.tree[1])}
        for s, fs in enumerate(self.sfields):
            with switches(**dict(env, **({"RTD_DIJC_ROWS32": "1"} if s in self.wide else {}))):
                for f in fs:
                    f.dose_influence_compact(release_plain=release)

    def infos(self):
        return [[f.dose_influence_compact_info() for f in fs] for fs in self.sfields]

    def keep(self, o, start=None):
        self.opts.append(o)
        if start is not None:
            self.set_weights(o, start)
        return o

    def robust(self, mode, start=None, probabilities=None, scen=None, obj=None, no_batch=False):
        sf = self.sfields if scen is None else [self.sfields[s] for s in scen]
        with switches(**({"RTD_ROBUST_NO_BATCH": "1"} if no_batch else {})):
            o = self.eng.create_robust_compact_optimizer(sf, self.obj if obj is None else obj, mode, probabilities)
        return self.keep(o, start)

    def voxelwise(self, start=None, scen=None, obj=None, no_batch=False):
        sf = self.sfields if scen is None else [self.sfields[s] for s in scen]
        with switches(**({"RTD_ROBUST_NO_BATCH": "1"} if no_batch else {})):
            o = self.eng.create_voxelwise_compact_optimizer(sf, self.obj if obj is None else obj)
        return self.keep(o, start)

    def compact(self, obj=None, start=None):
        return self.keep(self.eng.create_compact_optimizer(self.fields, self.obj if obj is None else obj), start)

    def retire(self):
        for o in self.opts:
            o.destroy()
        self.opts = []

    def scenario_dose_of(self, s, ws, dDose):
        """Zero, then apply_compact(init = 0) per field of scenario s in list order, into dDose."""
        self.eng.device_zero(dDose, 4 * self.nvox)
        for f, w in zip(self.sfields[s], ws):
            d = self.alloc(w.nbytes, zero=False)
            self.eng.to_device(d, np.ascontiguousarray(w, dtype=F))
            f.dose_influence_apply_compact(d, dDose, init=False)
        self.eng.sync()

    def scenario_grad(self, obj, s, dose_ptr, dG, dGrad):
        """rtd_objective_eval on a volume and apply_t_compact of scenario s's fields on its g -> (values, concatenated float32 gradient)."""
        self.eng.device_zero(dG, 4 * self.nvox)
        vals = obj.eval(dose_ptr, dG)
        out = []
        for f, n in zip(self.sfields[s], self.sizes):
            f.dose_influence_apply_t_compact(dG, dGrad)
            g = np.empty(n, dtype=F)
            self.eng.to_host(g, dGrad)
            out.append(g)
        return vals, np.concatenate(out)

    def restated_dose(self, s, ws):
        """Scenario s's dose of the weights ws by the numpy restatement of the compact form and its forward tree
        (tests/dij_compact_reference.py), from the matrices copied off the device: a zeroed volume, then per field in list order the
        tree's row sums added to the voxels whose rows have entries."""
        out = np.zeros(self.nvox, dtype=F)
        for f, d, w in zip(self.sfields[s], self.smats[s], ws):
            info, box = f.dose_influence_compact_info(), tuple(f.dose_influence_compact_device().box)
            scale, _, codes = DC.quantize(d.indptr, d.data)
            n_rows = int(box[3]) * int(box[4]) * int(box[5])
            rows = DC.box_rows(d.indices, self.dims, box)
            sums, count = DC.apply_tree(d.indptr, rows, codes, scale, w, n_rows, info["lanes_per_row"], info["entries_per_lane"])
            vox, has = DC.box_voxels(self.dims, box), count > 0
            out[vox[has]] = out[vox[has]] + sums[has]
        return out


def same_run(rig, a, b):
    """Two robust optimisers with the same record and the same scenario doses, bit for bit (beside gpu_plan_rigs.same)."""
    va, vb = a.scenario_values(), b.scenario_values()
    assert np.array_equal(bits(va[0]), bits(vb[0])) and np.array_equal(bits(va[1]), bits(vb[1])) and va[2] == vb[2], (va, vb)
    for s in range(len(va[0])):
        x, y = rig.volume(a.scenario_dose(s)), rig.volume(b.scenario_dose(s))
        assert np.array_equal(bits(x), bits(y)), "scenario %d: doses differ in %d voxels" % (s, int((bits(x) != bits(y)).sum()))
