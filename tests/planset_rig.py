"""The rigs of tests/test_gpu_planset.py: the products with P right-hand sides checked against the restated trees, and a plan set beside
the P plain optimisers it must equal bit for bit. A plain module like gpu_plan_rigs.py (no tests, no plugin); pytest does not rewrite
its asserts, so every assert carries a message."""
import ctypes as C

import numpy as np

import tree_reference as T
from gpu_plan_rigs import OptimizerRig
from gpu_support import bits, box_mask
from raytracedicom_amd import abi, pareto

PAD = np.uint32(0x7FC00ABC)                                            # a quiet NaN with a payload: the pattern of every slot nobody may write


def pad_filled(n):
    return np.full(n, PAD, dtype=np.uint32).view(np.float32)


class SetProducts:
    """One field of a FieldRig with its matrix, and per plan number a random w >= 0, a signed g and their restated trees (made once,
    shared by every case that uses that plan number: the trees are the expensive part)."""

    def __init__(self, rig, f, d, info, seed):
        self.rig, self.f, self.d, self.info, self.seed = rig, f, d, info, seed
        self.nvox, self.nspot = d.shape[0], int(np.prod(f._beam.spotWeights.shape))
        self.box = box_mask(rig, info).reshape(-1)
        assert np.all(self.box[d.indices]), "the row box is the dose box"
        self.has = np.bincount(d.indices, minlength=self.nvox) > 0
        assert (self.box & ~self.has).any() and not self.box.all(), "box voxels without entries and voxels outside the box both exist"
        self.plans = {}

    def plan(self, p):
        if p not in self.plans:
            rng = np.random.default_rng(self.seed + 1000 * p)
            w = (100.0 * rng.random(self.nspot)).astype(np.float32)
            g = (rng.random(self.nvox) - 0.5).astype(np.float32)
            d = self.d
            tree, tree_t = T.apply_tree(d.indptr, d.indices, d.data, w, n_rows=self.nvox), T.apply_t_tree(d.indptr, d.indices, d.data, g)
            assert tree.max() > 0 and np.abs(tree_t).max() > 0, "plan %d: a product is zero everywhere" % p
            self.plans[p] = (w, g, tree, tree_t)
        return self.plans[p]

    def check(self, n_plans, stride):
        """apply_set (init = 1 into the NaN pattern, init = 0 into a non-zero volume) and apply_t_set, plan-minor at `stride`: every
        slot p < n_plans bit for bit the restated tree of that plan's vector alone (box voxels without entries +0 under init = 1 and
        untouched under init = 0, nothing outside the box written), every pad slot p >= n_plans still the pattern."""
        eng, f, nvox, nspot, box, has = self.rig.eng, self.f, self.nvox, self.nspot, self.box, self.has
        ws, gs, trees, trees_t = zip(*[self.plan(p) for p in range(n_plans)])
        rng = np.random.default_rng(self.seed + 7)
        bufs = [eng.device_alloc(4 * n * stride) for n in (nspot, nvox, nvox, nspot)]
        dW, dVol, dG, dOut = bufs
        try:
            eng.to_device(dW, pareto.interleave(ws, stride, fill=np.nan))
            eng.to_device(dG, pareto.interleave(gs, stride, fill=np.nan))
            # init = 1 into the pattern
            eng.to_device(dVol, pad_filled(nvox * stride))
            f.dose_influence_apply_set(dW, dVol, n_plans, stride, init=True)
            got = np.empty(nvox * stride, dtype=np.float32)
            eng.to_host(got, dVol)
            got = got.reshape(nvox, stride)
            for p in range(n_plans):
                want = pad_filled(nvox).copy()
                want[box] = trees[p][box]
                differ = np.flatnonzero(bits(got[:, p]) != bits(want))
                print("apply_set(%d, %d) init=1, plan %d: %d of %d voxels differ from the restated tree (first %s)" % (n_plans, stride, p, differ.size, nvox, differ[:4]))
                assert differ.size == 0, "apply_set init=1: plan %d differs at %d voxels, first %s" % (p, differ.size, differ[:4])
            assert np.all(bits(got[:, n_plans:]) == PAD), "apply_set init=1 wrote a pad slot: %d words changed" % int((bits(got[:, n_plans:]) != PAD).sum())
            # init = 0 into a non-zero volume
            base = (1.0 + rng.random(nvox * stride)).astype(np.float32).reshape(nvox, stride)
            base[:, n_plans:] = pad_filled(nvox * (stride - n_plans)).reshape(nvox, stride - n_plans)
            eng.to_device(dVol, base)
            f.dose_influence_apply_set(dW, dVol, n_plans, stride, init=False)
            got = np.empty(nvox * stride, dtype=np.float32)
            eng.to_host(got, dVol)
            got = got.reshape(nvox, stride)
            for p in range(n_plans):
                want = base[:, p].copy()
                want[has] = base[has, p] + trees[p][has]              # (float32 + float32, the volume's value first)
                differ = np.flatnonzero(bits(got[:, p]) != bits(want))
                assert differ.size == 0, "apply_set init=0: plan %d differs at %d voxels, first %s" % (p, differ.size, differ[:4])
            assert np.all(bits(got[:, n_plans:]) == PAD), "apply_set init=0 wrote a pad slot"
            # the transposed product
            eng.to_device(dOut, pad_filled(nspot * stride))
            f.dose_influence_apply_t_set(dG, dOut, n_plans, stride)
            got_t = np.empty(nspot * stride, dtype=np.float32)
            eng.to_host(got_t, dOut)
            got_t = got_t.reshape(nspot, stride)
            for p in range(n_plans):
                differ = np.flatnonzero(bits(got_t[:, p]) != bits(trees_t[p]))
                print("apply_t_set(%d, %d), plan %d: %d of %d spots differ from the restated tree (first %s)" % (n_plans, stride, p, differ.size, nspot, differ[:4]))
                assert differ.size == 0, "apply_t_set: plan %d differs at %d spots, first %s" % (p, differ.size, differ[:4])
            assert np.all(bits(got_t[:, n_plans:]) == PAD), "apply_t_set wrote a pad slot"
        finally:
            for b in bufs:
                eng.device_free(b)


class PlanSetRig(OptimizerRig):
    """OptimizerRig (its fields, matrices and the plan objective obj / ref) with plan sets on variants of that objective, and per
    variant the plain objective and the plain optimiser a plan must equal."""

    def __init__(self, engine, scn):
        super().__init__(engine, scn)
        self.terms = list(self.ref.terms)                             # [(kind, roi, weight, level)]
        self.sets, self.plain_objs = [], []

    def variants(self, weight_factors, level_factors, weight_term=2, level_terms=(0, 1)):
        """One table per plan: the objective's terms with the weight of term weight_term (the overdose term) times weight_factors[p]
        and the levels of level_terms (the target's terms) times level_factors[p]."""
        out = []
        for wf, lf in zip(weight_factors, level_factors):
            out.append([(k, r, w * wf if t == weight_term else w, l * lf if t in level_terms else l) for t, (k, r, w, l) in enumerate(self.terms)])
        return out

    def planset(self, variants, options=None):
        s = self.eng.create_planset(self.fields, self.obj, variants, options)
        self.sets.append(s)
        return s

    def plain(self, variant, start=None, options=None):
        """A plain objective with the rig's ROIs and the variant's terms, and a plain optimiser on it -> (optimiser, objective)."""
        o = self.eng.create_objective(self.dims)
        self.plain_objs.append(o)
        for r in self.ref.rois:
            o.add_roi(r)
        for t in variant:
            o.add_term(*t)
        opt = self.eng.create_optimizer(self.fields, o, options)
        self.opts.append(opt)
        if start is not None:
            self.set_weights(opt, start)
        return opt, o

    def set_plan_weights(self, s, plan, start):
        for i, shp in enumerate(self.shapes):
            w = np.full(shp, start, dtype=np.float32) if np.isscalar(start) else np.ascontiguousarray(start[i], dtype=np.float32)
            dW = self.alloc(w.nbytes, zero=False)
            self.eng.to_device(dW, w)
            s.set_weights(plan, i, dW)
        self.eng.sync()

    def _raw_results(self, s, plan, opt):
        """Report and history of a plan and of its plain optimiser through the C calls, which fill both for a start that was not
        finite too (and return RTD_ERR_INVALID_ARG then, every time) -> ((report, history, status), the same of the optimiser)."""
        L, h, out = self.engine.lib(), self.eng._h, []
        for call in (lambda r, p, n: L.rtd_planset_result(h, s._h, plan, r, p, n), lambda r, p, n: L.rtd_optimizer_result(h, opt._h, r, p, n)):
            rep = abi.RtdOptimizerReport()
            call(C.byref(rep), None, 0)
            hist = np.zeros(rep.history_len, dtype=np.float64)
            st = call(C.byref(rep), hist.ctypes.data_as(C.POINTER(C.c_double)), rep.history_len)
            out.append((rep.as_dict(), hist, st))
        return out

    def same_as_plain(self, s, plan, opt, obj, what="", bad_start=False):
        """Plan `plan` of the set against its plain optimiser: w, w_best, the dose volume, every field of the report, the history and
        values() against Objective.eval on the plan's dose; all bit for bit -> (report, history). bad_start: the plan's start was not
        finite, which both results report with RTD_ERR_INVALID_ARG beside the filled report."""
        tag = "%splan %d" % (what, plan)
        if bad_start:
            (rs, hs, ss), (rp, hp, sp) = self._raw_results(s, plan, opt)
            assert ss == sp == abi.RTD_ERR_INVALID_ARG, "%s: a start that was not finite is reported by both: %d, %d" % (tag, ss, sp)
        else:
            rs, hs = s.result(plan)
            rp, hp = opt.result()
        assert rs == rp, "%s: reports differ: %r vs %r" % (tag, rs, rp)
        assert hs.size == hp.size and np.array_equal(bits(hs), bits(hp)), "%s: histories differ: %r vs %r" % (tag, hs, hp)
        for best in (False, True):
            for i in range(len(self.fields)):
                a, b = s.weights(plan, i, best=best), opt.weights(i, best=best)
                n = int((bits(a) != bits(b)).sum())
                assert n == 0, "%s: %s of field %d differ in %d of %d" % (tag, "w_best" if best else "w", i, n, a.size)
        dD, dG = self.alloc(4 * self.nvox), self.alloc(4 * self.nvox)
        s.dose(plan, dev_out=dD)
        mine, theirs = self.volume(dD), self.volume(opt.dose())
        n = int((bits(mine) != bits(theirs)).sum())
        assert n == 0, "%s: the dose volumes differ in %d of %d voxels" % (tag, n, mine.size)
        vals = obj.eval(dD, dG)
        got = s.values()[plan]
        assert np.array_equal(bits(got), bits(vals)), "%s: values() %r, Objective.eval on the plan's dose %r" % (tag, got, vals)
        if rs["iterations"]:
            assert got[0] == rs["f_last"], "%s: values()[0] %r is not f_last %r" % (tag, got[0], rs["f_last"])
        return rs, hs

    def close(self):
        for s in self.sets:
            s.destroy()
        for o in self.opts:
            o.destroy()
        self.opts = []
        for o in self.plain_objs:
            o.destroy()
        super().close()
