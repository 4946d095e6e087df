"""GPU tests of the variable-RBE dose (include/rtd.h "Variable-RBE dose"): rtd_rbe_*, rtd_optimizer_set_rbe,
rtd_optimizer_rbe_dose.

The reference is tests/rbe_reference.py, the numpy restatement of the contract in float32 in the stated order: the class volume, R, g_d
and g_n are compared bit for bit. The bounds against known answers are those of tests/test_rbe_reference.py (1e-6 relative, a factor 3
above the float32 steps' worst error). The ray-weight cut-off is 0 throughout (Dij needs it)."""
import ctypes as C

import numpy as np
import pytest

import optimizer_reference as OR
import rbe_reference as R
from gpu_plan_rigs import OptimizerRig, same
from gpu_support import FieldRig, bits, hetero_scene, options, rig_fixture
from raytracedicom_amd import abi, luts, rbe, scenarios

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = F(-12345.5)
BETA_X = 0.05

opt_rig_of = rig_fixture(OptimizerRig, "opt_rig_of")


def tissue(model, abx):
    return rbe.tissue(model, abx * BETA_X, BETA_X)


class Vols:
    """Device float volumes of one size on an engine, freed together."""

    def __init__(self, eng, n):
        self.eng, self.n, self.ptrs = eng, int(n), []

    def new(self, host=None, fill=None, extra=0):
        p = self.eng.device_alloc(4 * (self.n + extra))
        self.ptrs.append(p)
        if host is not None:
            self.eng.to_device(p, np.ascontiguousarray(host, dtype=F))
        elif fill is not None:
            self.eng.to_device(p, np.full(self.n + extra, fill, dtype=F))
        return p

    def get(self, p):
        out = np.empty(self.n, dtype=F)
        self.eng.to_host(out, p)
        return out

    def close(self):
        for p in self.ptrs:
            self.eng.device_free(p)


def _mask(dims, lo, hi):
    m = np.zeros((dims[2], dims[1], dims[0]), dtype=bool)
    m[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    return m.reshape(-1)


def test_forward_and_backward_are_the_restatement(engine):
    """A 37 x 21 x 13 grid (odd: no line starts aligned, every tail is taken), three tissues, two overlapping boxes assigned in order, one
    through assign_voxels and one through an Roi from roi_from_mask. d holds zeros, tiny and large values; n is in part independent of d
    (n > 0 where d == 0, a negative entry and a NaN: the e >= 0 rule). The whole grid, a box whose x range is 3 .. 33, output in place
    of an input, and pointers that are not 16-byte aligned (the one-voxel-per-lane path): bit for bit, and nothing outside the box."""
    dims = (37, 21, 13)
    nvox = 37 * 21 * 13
    t0, t1, t2 = tissue("mcnamara", 10.0), tissue("carabe", 2.0), tissue("wedenberg", 3.0)
    rng = np.random.default_rng(11)
    d = (80.0 * rng.random(nvox)).astype(F)
    kind = rng.integers(0, 8, nvox)
    d[kind == 0] = 0.0
    d[kind == 1] = (10.0 ** rng.uniform(-30, -4, nvox)).astype(F)[kind == 1]
    d[kind == 2] = (10.0 ** rng.uniform(2, 4, nvox)).astype(F)[kind == 2]
    n = (d * (20.0 * rng.random(nvox)).astype(F)).astype(F)
    free = rng.random(nvox) < 0.25
    n[free] = (40.0 * rng.random(nvox)).astype(F)[free]                # independent of d, n > 0 where d == 0 among them
    assert np.any((d == 0) & (n > 0))
    d[5], n[5], n[nvox - 7] = F(1.0), F(-50.0), F(np.nan)             # e < 0 (A = a0 - 50 a1 outweighs B * B), and a NaN
    g = (rng.random(nvox) - 0.5).astype(F)
    g[rng.random(nvox) < 0.1] = 0.0
    box_a, box_b = _mask(dims, (2, 1, 0), (20, 12, 8)), _mask(dims, (11, 6, 4), (35, 19, 12))
    ref = R.Rbe(dims, t0)
    eng = engine.Engine(0)
    vols = Vols(eng, nvox)
    model = roi = None
    dMask = eng.device_alloc(nvox)
    try:
        model = eng.create_rbe(dims, t0)
        for o in (ref, model):
            assert o.add_tissue(t1) == 1 and o.add_tissue(t2) == 2
        ref.assign(box_a, 1)
        ref.assign(box_b, 2)
        model.assign(np.flatnonzero(box_a).astype(np.int32), 1)        # rtd_rbe_assign_voxels
        eng.to_device(dMask, box_b.astype(np.uint8))
        roi = eng.roi_from_mask(dMask, dims)
        model.assign(roi, 2)                                           # rtd_rbe_assign_roi: the later one wins where the boxes overlap
        assert np.array_equal(model.classes(), ref.classes) and np.bincount(ref.classes, minlength=3).min() > 0
        assert np.all(ref.classes[box_a & box_b] == 2)
        dD, dN, dG = vols.new(d), vols.new(n), vols.new(g)
        sub = ((3, 2, 1), (33, 18, 11))
        for box in (None, sub):
            dR, dA, dB = vols.new(fill=SENTINEL), vols.new(fill=SENTINEL), vols.new(fill=SENTINEL)
            model.dose(dD, dN, dR, box=box)
            model.backward(dD, dN, dG, dA, dB, box=box)
            sent = np.full(nvox, SENTINEL, dtype=F)
            want_r = ref.dose(d, n, sent, box)
            want_a, want_b = ref.backward(d, n, g, sent, sent, box)
            for name, got, want in (("R", vols.get(dR), want_r), ("g_d", vols.get(dA), want_a), ("g_n", vols.get(dB), want_b)):
                diff = bits(got) != bits(want)
                inside = ref.box_mask(box)
                assert not diff.any(), "%s, box %r: %d of %d voxels differ (%d of them inside the box); first at %d: got %r, want %r (d %r, n %r, class %d)" % (
                    name, box, int(diff.sum()), nvox, int((diff & inside).sum()), int(np.flatnonzero(diff)[0]), got[diff][0], want[diff][0], d[diff][0], n[diff][0],
                    int(ref.classes[diff][0]))
            assert np.isfinite(want_r[ref.box_mask(box)]).all()
            if box is not None:
                assert np.all(want_r[~ref.box_mask(box)] == SENTINEL) and (~ref.box_mask(box)).sum() == nvox - 31 * 17 * 11
        full_r = ref.dose(d, n, np.zeros(nvox, dtype=F))
        full_a, full_b = ref.backward(d, n, g, np.zeros(nvox, dtype=F), np.zeros(nvox, dtype=F))
        assert full_r[5] == 0 and full_r[nvox - 7] == 0 and full_a[5] == 0 and full_b[nvox - 7] == 0
        assert full_r.max() > 100.0 and 0 < full_r[full_r > 0].min() < 1e-20 and np.abs(full_b).max() > 0
        # in place: R over d; g_d over g_R and g_n over n
        dD2, dN2, dG2 = vols.new(d), vols.new(n), vols.new(g)
        model.dose(dD2, dN, dD2)
        assert np.array_equal(bits(vols.get(dD2)), bits(full_r))
        model.backward(dD, dN2, dG2, dG2, dN2)
        assert np.array_equal(bits(vols.get(dG2)), bits(full_a)) and np.array_equal(bits(vols.get(dN2)), bits(full_b))
        # volumes that start 4 bytes behind an allocation: no 16-byte access is possible
        ptrs = []
        for host in (d, n, g, None, None, None):
            p = vols.new(fill=SENTINEL, extra=1) + 4
            if host is not None:
                eng.to_device(p, host)
            ptrs.append(p)
        model.dose(ptrs[0], ptrs[1], ptrs[3])
        model.backward(ptrs[0], ptrs[1], ptrs[2], ptrs[4], ptrs[5])
        for p, want in zip(ptrs[3:], (full_r, full_a, full_b)):
            assert np.array_equal(bits(vols.get(p)), bits(want))
    finally:
        vols.close()
        eng.device_free(dMask)
        if roi is not None:
            roi.close()
        if model is not None:
            model.destroy()
        eng.close()


class FieldCase:
    """One field of the small heterogeneous scene on its own engine, with its matrix and its LET values under luts.synth_let, and the
    dose Dw and the LET-weighted dose Nw of one weight vector as device volumes."""

    def __init__(self, engine, synth):
        scn = hetero_scene(synth, 96, [30.0])
        self.beam = scn.beams[0]
        self.rig = FieldRig(engine, scn, options(0.0))
        self.eng = self.rig.eng
        self.f = self.rig.field(self.beam)
        self.eng.set_let_table(luts.synth_let(synth))
        self.d = self.f.dose_influence()
        self.f.let_influence()
        self.nvox = int(np.prod(self.rig.dims))
        self.vols = Vols(self.eng, self.nvox)
        self.w = (1.0 + 99.0 * np.random.default_rng(41).random(self.beam.spotWeights.shape)).astype(F)
        self.dW = self.eng.device_alloc(self.w.nbytes)
        self.eng.to_device(self.dW, self.w)
        self.dD, self.dN = self.vols.new(fill=0.0), self.vols.new(fill=0.0)
        self.f.dose_influence_apply(self.dW, self.dD, init=False)
        self.f.let_apply(self.dW, self.dN, init=False)
        self.Dw, self.Nw = self.vols.get(self.dD), self.vols.get(self.dN)

    def close(self):
        self.vols.close()
        self.eng.device_free(self.dW)
        self.rig.close()


@pytest.fixture(scope="module")
def field_case(engine, synth):
    c = FieldCase(engine, synth)
    yield c
    c.close()


def test_constant_model_on_a_real_field(field_case):
    """Rbe.dose(Dw, Nw) under the constant model is 1.1 * Dw within 1e-6 relative (the float32 steps' worst error is 2.8e-7), and the
    restatement bit for bit; the RBE factor through let_average is 1.1 where there is dose and 0 elsewhere."""
    c = field_case
    model = c.eng.create_rbe(c.rig.dims, tissue("constant", 2.0))
    try:
        dR = c.vols.new(fill=SENTINEL)
        model.dose(c.dD, c.dN, dR)
        got = c.vols.get(dR)
        want = 1.1 * c.Dw.astype(np.float64)
        live = c.Dw > 0
        err = np.abs(got.astype(np.float64) - want)
        print("constant model: %d voxels with dose, worst |R - 1.1 d| / (1.1 d) = %.3g" % (int(live.sum()), float((err[live] / want[live]).max())))
        assert live.sum() > 1000 and np.all(err <= 1e-6 * want)
        assert np.array_equal(bits(got), bits(R.forward(R.coefficients(tissue("constant", 2.0)), c.Dw, c.Nw)))
        c.eng.let_average(dR, c.dD, c.nvox, dR, dose_floor=0.0)       # the RBE factor R / d: the same division
        fac = c.vols.get(dR)
        assert np.all(fac[~live] == 0) and np.all(np.abs(fac[live].astype(np.float64) - 1.1) <= 1.1 * (1e-6 + 2.0 ** -24))
    finally:
        model.destroy()


def test_mcnamara_in_water(engine, synth):
    """A one-layer field in water (the scene of the LETd test), the weights scaled to a peak dose of 2 Gy, McNamara at alpha/beta = 10 Gy:
    the RBE factor R / d along the central axis does not fall from the entrance to the voxel nearest the peak, and exceeds 1.1 at the
    distal edge. (alpha/beta = 10 Gy: at 2 Gy the LET term of RBEmax then outweighs the fall of the RBE with dose all along the plateau;
    at 2 Gy and alpha/beta = 2 Gy the factor of the float64 formulas dips by some 1e-3 in the plateau before it rises.)"""
    n = 64
    scn = scenarios.water_cube(synth, n=n, n_layers=1, spots=5, pitch=5.0)
    b = scn.beams[0]
    rig = FieldRig(engine, scn, options(0.0))
    model = None
    nvox = n ** 3
    vols = Vols(rig.eng, nvox)
    try:
        f = rig.field(b)
        f.dose_influence()
        rig.eng.set_let_table(luts.synth_let(synth))
        f.let_influence()
        plan = f.fetch("layer_plan").reshape(1, 8)
        model = rig.eng.create_rbe(scn.dims, tissue("mcnamara", 10.0))
        dD, dN, dZ, dR = vols.new(fill=0.0), vols.new(fill=0.0), vols.new(fill=0.0), vols.new(fill=0.0)
        dW = rig.eng.device_alloc(4 * b.spotWeights.size)
        try:
            rig.eng.to_device(dW, np.full(b.spotWeights.shape, 1.0, dtype=F))
            f.dose_influence_apply(dW, dD, init=True)
            peak = float(vols.get(dD).max())
            assert peak > 0
            rig.eng.to_device(dW, np.full(b.spotWeights.shape, 2.0 / peak, dtype=F))
            f.dose_influence_apply(dW, dD, init=True)
            f.let_apply(dW, dN, init=True)
            f.water_depth(dZ)
        finally:
            rig.eng.device_free(dW)
        model.dose(dD, dN, dR)
        dose, depth = vols.get(dD).reshape(n, n, n), vols.get(dZ).reshape(n, n, n)
        floor = 0.01 * float(dose.max())
        rig.eng.let_average(dR, dD, nvox, dR, dose_floor=floor)
        fac = vols.get(dR).reshape(n, n, n)
        axis = (slice(None), n // 2, n // 2)                          # the spot map is centred on x = y = 0 = voxel 32
        z_dose, z_depth, z_fac = dose[axis], depth[axis], fac[axis]
        live = np.nonzero(z_dose > floor)[0]
        order = live[np.argsort(z_depth[live], kind="stable")]        # from the entrance inwards
        upto = int(np.argmin(np.abs(z_depth[order] - float(plan[0, 2]))))
        run = z_fac[order][:upto + 1]
        print("dose along the axis (Gy):", " ".join("%.3g" % v for v in z_dose[order]))
        print("R / d along the axis, entrance to distal edge:", " ".join("%.4g" % v for v in z_fac[order]))
        assert abs(float(dose.max()) - 2.0) < 1e-3 and upto >= 10
        assert np.all(np.diff(run) >= 0) and run[-1] > run[0] > 1.0
        assert z_fac[order][-1] > 1.1 and np.all(z_fac[order][upto:] > 1.1)
    finally:
        vols.close()
        if model is not None:
            model.destroy()
        rig.close()


def _box(dims, centre, half):
    lo = [max(c - half, 0) for c in centre]
    hi = [min(c + half, n - 1) for c, n in zip(centre, dims)]
    return _mask(dims, lo, hi)


def test_optimizer_with_an_rbe_model(opt_rig_of, synth):
    """Two fields; SQ_DEVIATION on a target box at 1.1 x its true mean dose and SQ_OVERDOSE on a box behind it (along field 0), both on
    the RBE-weighted dose; McNamara with two tissues (alpha/beta 10 Gy, and 2 Gy in the box behind). History, weights and best weights
    over 10 iterations equal, bit for bit, a loop driven from Python with the public calls: apply, let_apply, Rbe.dose, Objective.eval,
    Rbe.backward, apply_t, let_apply_t, the float32 add and the step rule of tests/optimizer_reference.py. f_best <= f_0. rbe_dose() is
    the R of the iterate that entered the last iteration and dose() its physical dose. The history differs from that without the model;
    an optimiser whose model was removed equals one that never had one, and one that ran with it goes on as section 12's iteration does from the
    same state; run(3) captured into a graph equals the direct call."""
    import torch
    rig = opt_rig_of(hetero_scene(synth, 96, (0.0, 90.0)))
    eng = rig.eng
    eng.set_let_table(luts.synth_let(synth))
    for f in rig.fields:
        f.let_influence()
    w_true = np.concatenate([w.reshape(-1) for w in rig.w_true])
    offs = np.cumsum([0] + rig.sizes)
    dose_true = rig.matvec(w_true)
    v = int(np.argmax(dose_true))
    nx, ny, nz = rig.dims
    centre = (v % nx, (v // nx) % ny, v // (nx * ny))
    target = _box(rig.dims, centre, 5)
    behind = _box(rig.dims, (centre[0], centre[1], centre[2] - 9), 3)  # field 0 travels towards -z
    assert dose_true[behind].max() > 0 and dose_true[target].min() > 0
    obj = eng.create_objective(rig.dims)
    model = eng.create_rbe(rig.dims, tissue("mcnamara", 10.0))
    opts = []
    try:
        late = model.add_tissue(tissue("mcnamara", 2.0))
        model.assign(behind, late)
        obj.add_roi(target)
        obj.add_roi(behind)
        obj.add_term(abi.RTD_OBJ_SQ_DEVIATION, 0, 1.0, 1.1 * float(dose_true[target].mean()))
        obj.add_term(abi.RTD_OBJ_SQ_OVERDOSE, 1, 1.0, 0.25 * 1.1 * float(dose_true[behind].max()))

        def make(with_model=True):
            o = eng.create_optimizer(rig.fields, obj)
            opts.append(o)
            if with_model:
                o.set_rbe(model)
            return o
        n_it = 10
        opt = make()
        opt.run(n_it)
        rep, hist = opt.result()
        # the same loop from Python
        w0 = np.concatenate([np.asarray(f._beam.spotWeights, dtype=F).reshape(-1) for f in rig.fields])
        ref = OR.ReferenceOptimizer(None, None, None, w0)
        dD, dN, dR, dGR, dG1, dG2 = (rig.alloc(4 * rig.nvox) for _ in range(6))
        dGrad = [rig.alloc(4 * n) for n in rig.sizes]
        for _ in range(n_it):
            ws = [ref.w[a:b].reshape(s) for a, b, s in zip(offs, offs[1:], rig.shapes)]
            rig.dose_of(ws, dD)
            eng.device_zero(dN, 4 * rig.nvox)
            for f, wf in zip(rig.fields, ws):
                dW = rig.alloc(wf.nbytes, zero=False)
                eng.to_device(dW, np.ascontiguousarray(wf, dtype=F))
                f.let_apply(dW, dN, init=False)
            model.dose(dD, dN, dR)
            vals = obj.eval(dR, dGR)
            model.backward(dD, dN, dGR, dG1, dG2)
            a, b = [], []
            for f, n, dg in zip(rig.fields, rig.sizes, dGrad):
                for call, dgv, out in ((f.dose_influence_apply_t, dG1, a), (f.let_apply_t, dG2, b)):
                    call(dgv, dg)
                    part = np.empty(n, dtype=F)
                    eng.to_host(part, dg)
                    out.append(part)
            grad = (np.concatenate(a) + np.concatenate(b)).astype(F)
            ref.advance(float(vals[0]), grad)
        want_hist = np.array(ref.history, dtype=np.float64)
        print("device history:", " ".join("%.6g" % x for x in hist))
        print("python history:", " ".join("%.6g" % x for x in want_hist))
        assert hist.size == n_it and np.array_equal(bits(hist), bits(want_hist))
        got_w = np.concatenate([x.reshape(-1) for x in rig.weights(opt)])
        got_b = np.concatenate([x.reshape(-1) for x in rig.weights(opt, best=True)])
        assert np.array_equal(bits(got_w), bits(ref.w)) and np.array_equal(bits(got_b), bits(ref.w_best))
        assert np.abs(np.concatenate(b)).max() > 0                     # (the gradient did go through N^T as well)
        assert rep["f_best"] <= hist[0] and rep["f_best"] == want_hist.min() and want_hist.min() < want_hist[0]
        # R and d of the iterate that entered the last iteration
        r_last = rig.volume(dR)
        assert r_last.max() > 0 and np.array_equal(bits(rig.volume(opt.rbe_dose())), bits(r_last))
        assert np.array_equal(bits(rig.volume(opt.dose())), bits(rig.volume(dD))) and not np.array_equal(r_last, rig.volume(dD))
        # the model removed after it ran: section 12's iteration goes on from the same state (weights, step memory, best iterate)
        opt.set_rbe(None)
        opt.run(2)
        dG3 = rig.alloc(4 * rig.nvox)
        for _ in range(2):
            ws = [ref.w[a0:b0].reshape(s) for a0, b0, s in zip(offs, offs[1:], rig.shapes)]
            rig.dose_of(ws, dD)
            vals = obj.eval(dD, dG3)
            parts = []
            for f, n, dg in zip(rig.fields, rig.sizes, dGrad):
                f.dose_influence_apply_t(dG3, dg)
                part = np.empty(n, dtype=F)
                eng.to_host(part, dg)
                parts.append(part)
            ref.advance(float(vals[0]), np.concatenate(parts))
        _, hist2 = opt.result()
        assert hist2.size == n_it + 2 and np.array_equal(bits(hist2), bits(np.array(ref.history, dtype=np.float64)))
        assert np.array_equal(bits(np.concatenate([x.reshape(-1) for x in rig.weights(opt)])), bits(ref.w))
        # removed before any run: the optimiser of section 12
        plain, removed = make(with_model=False), make()
        removed.set_rbe(None)
        with pytest.raises(rig.engine.RtdError):
            removed.rbe_dose()
        plain.run(5)
        _, hp = plain.result()
        assert not np.array_equal(hp, hist[:5])
        removed.run(5)
        same(rig, plain, removed)
        # launches only: run(3) with the model, captured and replayed once, equals the direct call
        direct, captured = make(), make()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        eng.sync()
        eng.set_stream(s.cuda_stream)
        try:
            with torch.cuda.stream(s):
                direct.run(3)
                s.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    captured.run(3)
                g.replay()
            torch.cuda.synchronize()
        finally:
            eng.set_stream(None)
        _, hd = same(rig, direct, captured)
        assert np.array_equal(bits(hd), bits(hist[:3]))
    finally:
        for o in opts:
            o.destroy()
        obj.destroy()
        model.destroy()


def test_repeatable_and_without_side_effects(field_case):
    """Two runs give the same bits, and apply, apply_t and the LET products give the same bits before and after the RBE calls."""
    c = field_case
    rig = c.rig
    g = (np.random.default_rng(2).random(rig.shape) - 0.5).astype(F)
    before = (rig.product(c.f, c.w), rig.apply_t(c.f, g), rig._spot_call(c.f, c.f.let_apply_t, g))
    model = c.eng.create_rbe(rig.dims, tissue("mcnamara", 3.0))
    try:
        model.assign(np.arange(0, c.nvox, 3, dtype=np.int32), model.add_tissue(tissue("carabe", 10.0)))
        dG = c.vols.new(g)
        runs = []
        for _ in range(2):
            dR, dA, dB = c.vols.new(fill=SENTINEL), c.vols.new(fill=SENTINEL), c.vols.new(fill=SENTINEL)
            model.dose(c.dD, c.dN, dR)
            model.backward(c.dD, c.dN, dG, dA, dB)
            runs.append((c.vols.get(dR), c.vols.get(dA), c.vols.get(dB)))
        for x, y in zip(*runs):
            assert np.array_equal(bits(x), bits(y))
        assert runs[0][0].max() > 0 and np.abs(runs[0][2]).max() > 0
        assert np.array_equal(bits(c.vols.get(c.dD)), bits(c.Dw)) and np.array_equal(bits(c.vols.get(c.dN)), bits(c.Nw))
    finally:
        model.destroy()
    after = (rig.product(c.f, c.w), rig.apply_t(c.f, g), rig._spot_call(c.f, c.f.let_apply_t, g))
    for x, y in zip(before, after):
        assert np.array_equal(bits(x), bits(y))


def test_refusals(engine, synth):
    """Every INVALID_ARG / NOT_READY case of the header; after each refusal the objects still work."""
    L = engine.lib()
    INV, NR, OK = abi.RTD_ERR_INVALID_ARG, abi.RTD_ERR_NOT_READY, abi.RTD_OK
    scn = hetero_scene(synth, 64, [0.0], spots=3, layers=1)
    b = scn.beams[0]
    dims = tuple(scn.dims)
    nvox = 64 ** 3
    eng = engine.Engine(0)
    objs, opts, fields, models, rois = [], [], [], [], []
    vols = Vols(eng, nvox)
    try:
        eng.set_options(options(0.0))
        eng.set_luts(synth)
        eng.set_ct(scn.ct)
        good = tissue("mcnamara", 2.0)
        u3, out = abi.uint3(dims), C.c_void_p()
        create = lambda d, t, o=out: L.rtd_rbe_create(eng._h, d, C.byref(t) if t is not None else None, C.byref(o) if o is not None else None)   # noqa: E731
        # create: pointers, dims, the tissue
        assert create(None, good) == INV and create(u3, None) == INV and create(u3, good, None) == INV
        assert create(abi.uint3((0, 64, 64)), good) == INV and create(abi.uint3((64, 64, 0)), good) == INV
        assert create(abi.uint3((2048, 2048, 512)), good) == INV      # 2^31 voxels

        def spoiled(field, value, index=None):
            t = tissue("mcnamara", 2.0)
            if index is None:
                setattr(t, field, value)
            else:
                getattr(t, field)[index] = value
            return t
        bad = [spoiled("alpha_x", v) for v in (0.0, -0.1, np.nan, np.inf)] + [spoiled("beta_x", v) for v in (0.0, -0.05, np.nan, np.inf)] + \
              [spoiled(fld, v, i) for fld in ("rbe_max", "rbe_min") for i in (0, 1) for v in (np.nan, -np.inf)] + [spoiled("reserved", 1, 0), spoiled("reserved", 7, 1)]
        for t in bad:
            assert create(u3, t) == INV and not out.value
        model = eng.create_rbe(dims, good)
        models.append(model)
        mh = model._h
        cid = C.c_int32(-5)
        for t in bad:
            assert L.rtd_rbe_add_tissue(eng._h, mh, C.byref(t), C.byref(cid)) == INV and cid.value == -5
        assert L.rtd_rbe_add_tissue(eng._h, mh, None, C.byref(cid)) == INV and L.rtd_rbe_add_tissue(eng._h, mh, C.byref(good), None) == INV
        assert L.rtd_rbe_add_tissue(eng._h, None, C.byref(good), C.byref(cid)) == INV
        second = tissue("wedenberg", 3.0)
        assert model.add_tissue(second) == 1
        # assignments
        i3 = C.POINTER(C.c_int32)
        idx = np.array([0, 5, nvox - 1], dtype=np.int32)
        av = lambda a, c, n=None: L.rtd_rbe_assign_voxels(eng._h, mh, a.ctypes.data_as(i3) if a is not None else None, a.size if n is None else n, c)   # noqa: E731
        assert av(idx, 2) == INV and av(idx, -1) == INV and av(None, 1, 3) == INV
        assert av(np.array([0, -1], dtype=np.int32), 1) == INV and av(np.array([7, nvox], dtype=np.int32), 1) == INV
        assert not model.classes().any()                               # nothing was written
        small = eng.device_alloc(32 * 64 * 64)
        eng.to_device(small, np.ones(32 * 64 * 64, dtype=np.uint8))
        other = eng.roi_from_mask(small, (32, 64, 64))
        rois.append(other)
        mask = np.zeros(nvox, dtype=np.uint8)
        mask[1000:3000] = 1
        dMask = eng.device_alloc(nvox)
        eng.to_device(dMask, mask)
        roi = eng.roi_from_mask(dMask, dims)
        rois.append(roi)
        eng.device_free(small)
        eng.device_free(dMask)
        assert L.rtd_rbe_assign_roi(eng._h, mh, other._h, 1) == INV   # an ROI on other dims
        assert L.rtd_rbe_assign_roi(eng._h, mh, roi._h, 2) == INV and L.rtd_rbe_assign_roi(eng._h, mh, roi._h, -1) == INV
        assert L.rtd_rbe_assign_roi(eng._h, mh, None, 1) == INV and L.rtd_rbe_assign_roi(eng._h, None, roi._h, 1) == INV
        assert not model.classes().any()
        assert L.rtd_rbe_classes_device(eng._h, mh, None) == INV
        # dose and backward: pointers and boxes
        rng = np.random.default_rng(9)
        d = (4.0 * rng.random(nvox)).astype(F)
        n = (d * (10.0 * rng.random(nvox)).astype(F)).astype(F)
        g = (rng.random(nvox) - 0.5).astype(F)
        dD, dN, dG, dR, dA, dB = vols.new(d), vols.new(n), vols.new(g), vols.new(fill=SENTINEL), vols.new(fill=SENTINEL), vols.new(fill=SENTINEL)
        vp = C.c_void_p
        six = lambda *v: (C.c_int32 * 6)(*v)                           # noqa: E731
        dose = lambda a, bb, box, o: L.rtd_rbe_dose(eng._h, mh, vp(a), vp(bb), box, vp(o))   # noqa: E731
        back = lambda a, bb, gg, box, x, y: L.rtd_rbe_backward(eng._h, mh, vp(a), vp(bb), vp(gg), box, vp(x), vp(y))   # noqa: E731
        assert dose(None, dN, None, dR) == INV and dose(dD, None, None, dR) == INV and dose(dD, dN, None, None) == INV
        assert L.rtd_rbe_dose(eng._h, None, vp(dD), vp(dN), None, vp(dR)) == INV
        for args in ((None, dN, dG, None, dA, dB), (dD, None, dG, None, dA, dB), (dD, dN, None, None, dA, dB), (dD, dN, dG, None, None, dB),
                     (dD, dN, dG, None, dA, None), (dD, dN, dG, None, dA, dA)):
            assert back(*args) == INV
        for box in (six(-1, 0, 0, 5, 5, 5), six(0, 0, 0, 64, 5, 5), six(0, 0, 0, 5, 64, 5), six(0, 0, 0, 5, 5, 64), six(6, 0, 0, 5, 5, 5), six(0, 9, 0, 5, 8, 5),
                    six(0, 0, 3, 5, 5, 2)):
            assert dose(dD, dN, box, dR) == INV and back(dD, dN, dG, box, dA, dB) == INV
        for p in (dR, dA, dB):
            assert np.all(vols.get(p) == SENTINEL)                     # nothing was written

        ref = R.Rbe(dims, good)
        ref.add_tissue(second)

        def works():
            """The object still computes what the restatement computes, on a box."""
            box = ((1, 2, 3), (62, 40, 9))
            model.dose(dD, dN, dR, box=box)
            model.backward(dD, dN, dG, dA, dB, box=box)
            sent = np.full(nvox, SENTINEL, dtype=F)
            wa, wb = ref.backward(d, n, g, sent, sent, box)
            assert np.array_equal(model.classes(), ref.classes)
            assert np.array_equal(bits(vols.get(dR)), bits(ref.dose(d, n, sent, box)))
            assert np.array_equal(bits(vols.get(dA)), bits(wa)) and np.array_equal(bits(vols.get(dB)), bits(wb))
        works()
        model.assign(roi, 1)
        ref.assign(mask.astype(bool), 1)
        works()
        # a 257th class
        full = eng.create_rbe((4, 4, 4), good)
        models.append(full)
        for k in range(1, 256):
            assert full.add_tissue(second) == k
        assert L.rtd_rbe_add_tissue(eng._h, full._h, C.byref(second), C.byref(cid)) == INV and cid.value == -5
        full.assign(np.array([63], dtype=np.int32), 255)
        assert full.classes()[63] == 255
        # the optimiser
        f, f2 = eng.create_field(b, dims), eng.create_field(b, dims)
        fields += [f, f2]
        dmat = f.dose_influence()
        f2.dose_influence()
        has = np.bincount(dmat.indices, minlength=nvox) > 0

        def objective():
            o = eng.create_objective(dims)
            objs.append(o)
            o.add_roi(has)
            o.add_term(abi.RTD_OBJ_SQ_OVERDOSE, 0, 1.0, 0.0)
            return o
        obj, let_obj = objective(), objective()
        opt, two = eng.create_optimizer([f], obj), eng.create_optimizer([f, f2], obj)
        rob = eng.create_robust_optimizer([[f], [f2]], obj, abi.RTD_ROBUST_EXPECTED)
        vox = eng.create_voxelwise_optimizer([[f], [f2]], obj)
        opts += [opt, two, rob, vox]
        sr = lambda o, m: L.rtd_optimizer_set_rbe(eng._h, o._h if o is not None else None, m._h if m is not None else None)   # noqa: E731
        sl = lambda o, lo: L.rtd_optimizer_set_let_objective(eng._h, o._h, lo._h if lo is not None else None)   # noqa: E731
        pd = C.c_void_p()
        assert sr(None, model) == INV
        assert sr(opt, model) == NR                                    # no LET table, no LET values
        eng.set_let_table(luts.synth_let(synth))
        f.let_influence()
        assert sr(two, model) == NR                                    # f2 has a matrix and no LET values
        f2.let_influence()
        assert sr(rob, model) == INV and sr(vox, model) == INV
        assert sr(opt, full) == INV                                    # an RBE object on other dims
        assert L.rtd_optimizer_rbe_dose(eng._h, opt._h, C.byref(pd)) == NR and L.rtd_optimizer_rbe_dose(eng._h, opt._h, None) == INV
        assert sr(opt, None) == OK                                     # nothing to remove
        # one or the other
        assert sl(opt, let_obj) == OK
        assert sr(opt, model) == INV
        opt.run(1)
        assert sl(opt, None) == OK
        assert sr(opt, model) == OK and sr(two, model) == OK
        assert sl(opt, let_obj) == INV
        assert sl(opt, None) == OK                                     # (removing what is not there leaves the model's volumes alone)
        opt.run(2)
        two.run(2)
        assert opt.result()[0]["iterations"] == 3 and two.result()[0]["iterations"] == 2 and opt.rbe_dose() and np.isfinite(opt.result()[1]).all()
        # a table set after set_rbe: the run is refused until the LET values are made again
        eng.set_let_table(luts.synth_let(synth).copy())
        assert L.rtd_optimizer_run(eng._h, opt._h, 1) == NR
        assert opt.result()[0]["iterations"] == 3
        f.let_influence()
        f2.let_influence()
        opt.run(1)
        assert opt.result()[0]["iterations"] == 4
        assert sr(opt, None) == OK and L.rtd_optimizer_rbe_dose(eng._h, opt._h, C.byref(pd)) == NR
        opt.run(1)
        assert opt.result()[0]["iterations"] == 5
        works()
    finally:
        for o in opts:
            o.destroy()
        for o in objs:
            o.destroy()
        for m in models:
            m.destroy()
        for r in rois:
            r.close()
        vols.close()
        for fl in fields:
            fl.destroy()
        eng.close()
