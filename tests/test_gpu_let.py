"""GPU tests of the dose-averaged LET (include/rtd.h "Dose-averaged LET"): rtd_set_let_table,
rtd_field_water_depth, rtd_field_let_influence and its products, rtd_let_average, rtd_optimizer_set_let_objective.

The reference is tests/let_reference.py, the numpy restatement of the three rules in float32 in the stated order: depth and matrix
values are compared bit for bit. The products are held to the bounds the dose products are held to (gpu_support.row_bound /
col_bound with gamma(n)): they are the same kernels on a second values array. The ray-weight cut-off is 0 throughout (Dij needs it).

Every scene is made once per module (a field, its matrix, its LET values under luts.synth_let) and shared; a test that puts another
table in puts the module's table back."""
import ctypes as C
import math

import numpy as np
import pytest

import asym_scenes
import let_reference as R
import optimizer_reference as OR
from gpu_plan_rigs import OptimizerRig, same
from gpu_support import FieldRig, bits, box_mask, col_bound, gamma, hetero_scene, nuc_luts, options, rig_fixture, row_bound, worst_ratio  # noqa: F401
from raytracedicom_amd import abi, luts, scenarios

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = F(-12345.5)

opt_rig_of = rig_fixture(OptimizerRig, "opt_rig_of")


def scene_of(synth, name):
    """-> (scenario, beam, dose dims or None for the CT's)."""
    if name == "hetero":                       # the small heterogeneous scene of tests/test_gpu_dose_influence_apply.py
        scn = hetero_scene(synth, 96, [30.0])
        return scn, scn.beams[0], None
    if name == "short_trace":                  # the same with a trace that ends inside the patient: box voxels behind the last step
        scn = hetero_scene(synth, 96, [30.0], steps=150)
        return scn, scn.beams[0], None
    scn = asym_scenes.scene(synth, "A")        # non-cubic CT, coarse dose grid, oblique beam
    b = scn.beams[0]
    if name == "oblique_parallel":
        b = b.replace(sourceDist=(math.inf, math.inf))
    else:
        assert name == "finite_source" and all(math.isfinite(v) for v in b.sourceDist)
    return scn, b, scn.dose_dims


class Case:
    """One field on its own engine: computed, with its matrix (unless matrix=False), the engine's table = luts.synth_let and the
    LET values made from it; and what the restatement needs of it."""

    def __init__(self, engine, synth, name, matrix=True):
        scn, self.beam, dims = scene_of(synth, name)
        self.rig = FieldRig(engine, scn, options(0.0), dims)
        self.eng = self.rig.eng
        self.f = self.rig.field(self.beam)
        self.table = luts.synth_let(synth)
        self.eng.set_let_table(self.table)
        if matrix:
            self.d = self.f.dose_influence()
            self.f.let_influence()
        else:
            self.rig.compute(self.f)
        _, self.info = self.f.finish()
        W, H, L = self.info["ray_dims"]
        self.S = self.beam.tracerSteps
        self.wepl = self.f.fetch("wepl").reshape(self.S, H, W).copy()
        self.plan = self.f.fetch("layer_plan").reshape(L, 8).copy()
        self.tr = R.Transfer(self.beam, self.info)
        self.nx, self.ny, self.nz = self.rig.dims
        self.spots_per_layer = int(np.prod(self.beam.spotWeights.shape[1:]))
        self._n = None

    def let_values(self):
        va, nnz = self.f.let_influence_device()
        assert nnz == self.d.nnz and va
        out = np.empty(nnz, dtype=F)
        self.eng.to_host(out, va)
        return out

    def restated_values(self, table):
        if self._n is None or self._n[0] is not table:
            rows = np.unique(self.d.indices)
            depth = np.full(self.d.shape[0], np.nan, dtype=F)
            depth[rows] = R.water_depth(self.tr, self.wepl, rows % self.nx, (rows // self.nx) % self.ny, rows // (self.nx * self.ny))
            self._n = (table, R.let_values(self.d.data, self.d.indices, self.d.indptr, self.spots_per_layer, self.plan, table, depth))
        return self._n[1]

    def let_apply(self, w, into=None, init=True):
        """N w on the device into a copy of `into` (default: a NaN-filled volume) -> the volume."""
        rig = self.rig
        vol = np.full(rig.shape, np.nan, dtype=F) if into is None else np.ascontiguousarray(into, dtype=F)
        w = np.ascontiguousarray(w, dtype=F)
        dW = self.eng.device_alloc(w.nbytes)
        try:
            self.eng.to_device(dW, w)
            self.eng.to_device(rig.dDose, vol)
            self.f.let_apply(dW, rig.dDose, init=init)
            out = np.empty(rig.shape, dtype=F)
            self.eng.to_host(out, rig.dDose)
        finally:
            self.eng.device_free(dW)
        return out

    def let_product(self, w):
        return self.let_apply(w, into=np.zeros(self.rig.shape, dtype=F), init=True).reshape(-1)

    def let_apply_t(self, g):
        return self.rig._spot_call(self.f, self.f.let_apply_t, g)

    def close(self):
        self.rig.close()


@pytest.fixture(scope="module")
def case_of(engine, synth):
    made = {}

    def get(name, matrix=True):
        if name not in made:
            made[name] = Case(engine, synth, name, matrix)
        return made[name]
    yield get
    for c in made.values():
        c.close()


MATRIX_CASES = ["hetero", "oblique_parallel", "finite_source"]


@pytest.mark.parametrize("name", MATRIX_CASES + ["short_trace"])
def test_water_depth_is_the_restatement(case_of, name):
    """Bit for bit inside the field's dose box; the sentinel outside it. short_trace: box voxels behind the last traced step carry the
    clamped depth; the oblique boxes hold voxels beside the ray grid, clamped likewise."""
    c = case_of(name, matrix=name != "short_trace")
    rig = c.rig
    rig.eng.to_device(rig.dDose, np.full(rig.shape, SENTINEL, dtype=F))
    c.f.water_depth(rig.dDose)
    got = np.empty(rig.shape, dtype=F)
    rig.eng.to_host(got, rig.dDose)
    lo, hi = c.info["dose_box_min"], c.info["dose_box_max"]
    box = box_mask(rig, c.info)
    assert box.any() and (name not in ("hetero", "short_trace") or not box.all())   # (on the coarse grid the box may be the whole grid)
    want = np.full(rig.shape, SENTINEL, dtype=F)
    want[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = R.box_depth(c.tr, c.wepl, lo, hi)
    diff = bits(got) != bits(want)
    assert not diff.any(), "%d of %d voxels differ (%d of them inside the box); first: got %r, want %r" % (
        int(diff.sum()), diff.size, int((diff & box).sum()), got[diff][:1], want[diff][:1])
    assert np.isfinite(got[box]).all() and got[box].min() >= 0 and got[box].max() > 10.0
    x = np.arange(lo[0], hi[0] + 1)[None, None, :]
    y = np.arange(lo[1], hi[1] + 1)[None, :, None]
    z = np.arange(lo[2], hi[2] + 1)[:, None, None]
    pi, pj, pk = c.tr.trace_index(x, y, z)
    W, H, _ = c.info["ray_dims"]
    print("%s: box %s .. %s; voxels behind the last step %d, in front of step 0 %d, beside the ray grid %d" % (
        name, lo, hi, int((pk >= c.S - 1).sum()), int((pk < 0).sum()), int(((pi < 0) | (pi >= W - 1) | (pj < 0) | (pj >= H - 1)).sum())))
    if name == "short_trace":
        behind = pk >= F(c.S - 1)
        assert behind.shape == (hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1) and behind.any()
        # ... and there the depth does not depend on how far behind: it is the blend of the last step's depths
        last = R.step_depth(c.wepl, c.tr.first)[-1]
        inner = behind & (pi >= 0) & (pi < W - 1) & (pj >= 0) & (pj < H - 1)
        sub = got[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1]
        assert inner.any() and sub[inner].min() >= last.min() * (1 - 2.0 ** -21) and sub[inner].max() <= last.max() * (1 + 2.0 ** -21)


@pytest.mark.parametrize("name", MATRIX_CASES)
def test_matrix_values_are_the_restatement(case_of, name):
    """The CSC LET values equal float32(D * L) of the restatement bit for bit; a one-hot w through let_apply(init=1) reproduces column j
    of N exactly and zero elsewhere in the box, which pins the row-major copy against the CSC one."""
    c = case_of(name)
    d = c.d
    got, want = c.let_values(), c.restated_values(c.table)
    diff = bits(got) != bits(want)
    assert not diff.any(), "%d of %d entries differ; first: got %r, want %r (D %r)" % (int(diff.sum()), diff.size, got[diff][:1], want[diff][:1], d.data[diff][:1])
    assert got.max() > 0 and not np.array_equal(got, d.data)
    box = box_mask(c.rig, c.info).reshape(-1)
    lens = np.diff(d.indptr)
    per = c.spots_per_layer
    for layer in range(d.shape[1] // per):
        j = layer * per + int(np.argmax(lens[layer * per:(layer + 1) * per]))   # the layer's longest column
        assert lens[j] > 0
        e = np.zeros(d.shape[1], dtype=F)
        e[j] = 1.0
        out = c.let_apply(e.reshape(c.beam.spotWeights.shape)).reshape(-1)
        expect = np.full(d.shape[0], np.nan, dtype=F)
        expect[box] = 0.0
        rows = d.indices[d.indptr[j]:d.indptr[j + 1]]
        assert np.all(box[rows])
        expect[rows] = want[d.indptr[j]:d.indptr[j + 1]]
        assert np.array_equal(bits(out), bits(expect)), (name, j)


def test_constant_table_doubles_the_dose_products(case_of, synth):
    """With a constant table of 2.0: let_apply(w) = 2 * apply(w) and let_apply_t(g) = 2 * apply_t(g) bit for bit (every product is
    doubled exactly and every sum with it), and let_average gives exactly 2.0 where the dose exceeds the floor and 0 elsewhere."""
    c = case_of("hetero")
    rig, f, b = c.rig, c.f, c.beam
    rng = np.random.default_rng(41)
    w = (1.0 + 99.0 * rng.random(b.spotWeights.shape)).astype(F)
    g = (np.where(rng.random(rig.shape) < 0.5, -1.0, 1.0) * (0.25 + 0.25 * rng.random(rig.shape))).astype(F)
    try:
        c.eng.set_let_table(np.full_like(c.table, 2.0))
        f.let_influence()
        a, t = rig.product(f, w), rig.apply_t(f, g)
        la, lt = c.let_product(w), c.let_apply_t(g)
        assert a.max() > 0 and np.abs(t).max() > 0
        assert np.array_equal(bits(la), bits((2.0 * a).astype(F))) and np.array_equal(bits(lt), bits((2.0 * t).astype(F)))
        mags = np.abs(c.d.data.astype(np.float64))
        assert mags.min() * 0.25 >= 2.0 ** -126 and mags.max() * 200.0 * c.d.shape[1] < 2.0 ** 126   # (the range the doubling claim holds for)
        floor = float(F(0.01 * a.max()))
        n = a.size
        dA, dL, dO = (c.eng.device_alloc(4 * n) for _ in range(3))
        try:
            c.eng.to_device(dA, a)
            c.eng.to_device(dL, la)
            c.eng.to_device(dO, np.full(n, np.nan, dtype=F))
            c.eng.let_average(dL, dA, n, dO, dose_floor=floor)
            out = np.empty(n, dtype=F)
            c.eng.to_host(out, dO)
            want = np.where(a > F(floor), F(2.0), F(0.0)).astype(F)
            assert (want == 2.0).any() and ((want == 0.0) & (a > 0)).any()
            assert np.array_equal(bits(out), bits(want))
            c.eng.let_average(dL, dA, n, dL, dose_floor=floor)        # in place on the LET-weighted dose ...
            c.eng.to_host(out, dL)
            assert np.array_equal(bits(out), bits(want))
            c.eng.to_device(dL, la)
            c.eng.let_average(dL, dA, n, dA, dose_floor=floor)        # ... and on the dose
            c.eng.to_host(out, dA)
            assert np.array_equal(bits(out), bits(want))
        finally:
            for p in (dA, dL, dO):
                c.eng.device_free(p)
    finally:
        c.eng.set_let_table(c.table)
        f.let_influence()
    assert np.array_equal(bits(c.let_values()), bits(c.restated_values(c.table)))   # the module's table is back


def test_products_against_float64_and_adjointness(case_of, engine):
    """With synth_let: every element of N w and of N^T g within gamma(n) * sum |a| |x| of its float64 evaluation from the copied arrays
    (the bounds the dose products are held to), and <N w, g> = <w, N^T g> within the sum of those bounds."""
    c = case_of("hetero")
    dn = engine.DoseInfluence(c.d.indptr, c.d.indices, c.let_values(), c.d.dose_dims, c.d.spot_shape)
    rng = np.random.default_rng(17)
    w = (100.0 * rng.random(c.beam.spotWeights.shape)).astype(F)
    g = (rng.random(c.rig.shape) - 0.5).astype(F)
    got = c.let_product(w).astype(np.float64)
    n, s = row_bound(dn, w)
    err = np.abs(got - dn.matvec(w))
    print("let_apply: worst |gpu - ref| / bound = %.3g, longest row %d" % (worst_ratio(err, gamma(n) * s), int(n.max())))
    assert got.max() > 0 and np.all(err <= gamma(n) * s), worst_ratio(err, gamma(n) * s)
    got_t = c.let_apply_t(g).reshape(-1).astype(np.float64)
    nt, st = col_bound(dn, g)
    err_t = np.abs(got_t - dn.rmatvec(g))
    print("let_apply_t: worst |gpu - ref| / bound = %.3g, longest column %d" % (worst_ratio(err_t, gamma(nt) * st), int(nt.max())))
    assert np.abs(got_t).max() > 0 and np.all(err_t <= gamma(nt) * st), worst_ratio(err_t, gamma(nt) * st)
    lhs = float(np.dot(got, g.reshape(-1).astype(np.float64)))
    rhs = float(np.dot(w.reshape(-1).astype(np.float64), got_t))
    bound = float(np.dot(gamma(n) * s, np.abs(g.reshape(-1).astype(np.float64))) + np.dot(gamma(nt) * st, np.abs(w.reshape(-1).astype(np.float64))))
    print("<N w, g> = %.9g, <w, N^T g> = %.9g, difference %.3g of the bound %.3g" % (lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound


def test_letd_rises_towards_the_peak_in_water(engine, synth):
    """A one-layer field in water: LETd along the central axis is non-decreasing from the entrance to the voxel nearest the peak, and
    it is the table's value at the voxel's depth there (all spots have the layer's energy) within the rounding of the two sums."""
    n = 64
    scn = scenarios.water_cube(synth, n=n, n_layers=1, spots=5, pitch=5.0)
    b = scn.beams[0]
    rig = FieldRig(engine, scn, options(0.0))
    try:
        f = rig.field(b)
        d = f.dose_influence()
        table = luts.synth_let(synth)
        rig.eng.set_let_table(table)
        f.let_influence()
        _, info = f.finish()
        plan = f.fetch("layer_plan").reshape(1, 8)
        w = np.full(b.spotWeights.shape, 100.0, dtype=F)
        nvox = n ** 3
        dW, dD, dN, dZ = rig.eng.device_alloc(w.nbytes), rig.eng.device_alloc(4 * nvox), rig.eng.device_alloc(4 * nvox), rig.eng.device_alloc(4 * nvox)
        try:
            rig.eng.to_device(dW, w)
            for p in (dD, dN, dZ):
                rig.eng.device_zero(p, 4 * nvox)
            f.dose_influence_apply(dW, dD, init=False)               # per field: apply into one volume, let_apply into another
            f.let_apply(dW, dN, init=False)
            f.water_depth(dZ)
            dose, depth, letd = (np.empty((n, n, n), dtype=F) for _ in range(3))
            rig.eng.to_host(dose, dD)
            rig.eng.to_host(depth, dZ)
            floor = 0.01 * float(dose.max())
            rig.eng.let_average(dN, dD, nvox, dN, dose_floor=floor)  # then one let_average
            rig.eng.to_host(letd, dN)
        finally:
            for p in (dW, dD, dN, dZ):
                rig.eng.device_free(p)
        axis = (slice(None), n // 2, n // 2)                          # the spot map is centred on x = y = 0 = voxel 32
        z_dose, z_depth, z_let = dose[axis], depth[axis], letd[axis]
        live = np.nonzero(z_dose > floor)[0]
        assert live.size > 10
        peak_depth = float(plan[0, 2])
        order = live[np.argsort(z_depth[live], kind="stable")]        # from the entrance inwards
        upto = int(np.argmin(np.abs(z_depth[order] - peak_depth)))
        run = z_let[order][:upto + 1]
        print("LETd along the axis (keV/um), entrance to peak:", " ".join("%.3g" % v for v in run))
        assert upto >= 10 and np.all(np.diff(run) >= 0) and run[-1] > 2.0 * run[0] > 0
        want = R.lookup(table, plan[0, 0], plan[0, 1], z_depth[order][:upto + 1])
        nmax = int(np.bincount(d.indices, minlength=nvox).max())
        assert np.all(np.abs(run - want) <= (2 * gamma(nmax) + 2 * 2.0 ** -24) * want)
        assert info["uniform_sigma"] in (0, 1)
    finally:
        rig.close()


def test_repeatable_and_without_side_effects(case_of, engine, synth):
    """Two calls and a second handle give the same bits; let_influence, water_depth and the products leave the CSC arrays, apply,
    apply_t, spot_gradient and a following compute + transfer bit-identical to before."""
    c = case_of("hetero")
    rng = np.random.default_rng(2)
    w = (100.0 * rng.random(c.beam.spotWeights.shape)).astype(F)
    g = (rng.random(c.rig.shape) - 0.5).astype(F)
    first = (c.let_values(), c.let_product(w), c.let_apply_t(g))
    c.f.let_influence()
    again = (c.let_values(), c.let_product(w), c.let_apply_t(g))
    for a, b in zip(first, again):
        assert np.array_equal(bits(a), bits(b))
    scn, beam, dims = scene_of(synth, "hetero")
    rig = FieldRig(engine, scn, options(0.0), dims)
    try:
        f = rig.field(beam)
        dose0, _, _ = rig.compute(f)
        d = f.dose_influence()
        before = (rig.product(f, w), rig.apply_t(f, g), rig.grad(f, g), f.fetch("bev").copy())
        other = Case.__new__(Case)
        other.rig, other.eng, other.f, other.beam, other.d = rig, rig.eng, f, beam, d
        rig.eng.set_let_table(c.table)
        f.let_influence()
        rig.eng.to_device(rig.dDose, np.zeros(rig.shape, dtype=F))
        f.water_depth(rig.dDose)
        second = (other.let_values(), other.let_product(w), other.let_apply_t(g))
        for a, b in zip(first, second):
            assert np.array_equal(bits(a), bits(b))
        after = (rig.product(f, w), rig.apply_t(f, g), rig.grad(f, g), f.fetch("bev").copy())
        for a, b in zip(before, after):
            assert np.array_equal(bits(a), bits(b))
        cp, ri, va, nnz = f.dose_influence_device()
        indptr, indices, data = np.empty_like(d.indptr), np.empty_like(d.indices), np.empty_like(d.data)
        rig.eng.to_host(indptr, cp)
        rig.eng.to_host(indices, ri)
        rig.eng.to_host(data, va)
        assert nnz == d.nnz and np.array_equal(indptr, d.indptr) and np.array_equal(indices, d.indices) and np.array_equal(bits(data), bits(d.data))
        dose1, _, _ = rig.compute(f)                                  # a following compute + transfer
        assert dose0.max() > 0 and np.array_equal(bits(dose1), bits(dose0))
    finally:
        rig.close()


def test_products_are_hipgraph_capturable(engine, synth):
    """After let_influence, let_apply + let_apply_t only launch on the handle's stream: captured into one graph (a single chain) on a
    caller's stream and replayed twice, they give the bits of the direct calls."""
    import torch
    n = 96
    scn = hetero_scene(synth, n, [25.0], layers=2)
    b = scn.beams[0]
    dev = torch.device("cuda:0")
    eng = engine.Engine(0)
    eng.set_options(options(0.0))
    eng.set_luts(scn.luts)
    eng.set_ct(scn.ct)
    eng.set_let_table(luts.synth_let(synth))
    fld = eng.create_field(b, scn.dims)
    fld.dose_influence()
    fld.let_influence()
    eng.sync()
    gen = torch.Generator().manual_seed(5)
    w = (100.0 * torch.rand(b.spotWeights.shape, generator=gen)).to(dev)
    gvol = (torch.rand((n, n, n), generator=gen) - 0.5).to(dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.set_stream(s.cuda_stream)
    ref_d = torch.full((n, n, n), float("nan"), dtype=torch.float32, device=dev)
    ref_t = torch.full(tuple(b.spotWeights.shape), float("nan"), dtype=torch.float32, device=dev)
    out_d, out_t = ref_d.clone(), ref_t.clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        fld.let_apply(w.data_ptr(), ref_d.data_ptr(), init=True)
        fld.let_apply_t(gvol.data_ptr(), ref_t.data_ptr())
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            fld.let_apply(w.data_ptr(), out_d.data_ptr(), init=True)
            fld.let_apply_t(gvol.data_ptr(), out_t.data_ptr())
        for _ in range(2):
            g.replay()
    torch.cuda.synchronize()
    assert float(torch.nan_to_num(ref_d).max()) > 0 and float(ref_t.abs().max()) > 0
    assert torch.equal(ref_d.view(torch.int32), out_d.view(torch.int32)) and torch.equal(ref_t.view(torch.int32), out_t.view(torch.int32))
    eng.set_stream(None)
    fld.destroy()
    eng.close()


def _box(dims, centre, half):
    m = np.zeros((dims[2], dims[1], dims[0]), dtype=bool)
    lo = [max(c - half, 0) for c in centre]
    hi = [min(c + half, n - 1) for c, n in zip(centre, dims)]
    m[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    return m.reshape(-1)


def test_optimizer_with_a_let_objective(opt_rig_of, synth):
    """Two fields; dose objective SQ_DEVIATION on a target box, LET objective SQ_OVERDOSE on a box behind it (along field 0). History and
    weights over 10 iterations equal, bit for bit, a loop driven from Python with the public calls: apply, let_apply, two
    Objective.eval, apply_t, let_apply_t, the float32 add and the step rule of tests/optimizer_reference.py. f_best <= f_0. An
    optimiser whose LET objective was removed equals one that never had one. A run after set_let_objective allocates nothing: it is
    captured into a graph."""
    import torch
    rig = opt_rig_of(hetero_scene(synth, 96, (0.0, 90.0)))
    eng = rig.eng
    table = luts.synth_let(synth)
    eng.set_let_table(table)
    lets = []
    for f, d in zip(rig.fields, rig.mats):
        f.let_influence()
        va, nnz = f.let_influence_device()
        v = np.empty(nnz, dtype=F)
        eng.to_host(v, va)
        lets.append(rig.engine.DoseInfluence(d.indptr, d.indices, v, d.dose_dims, d.spot_shape))
    w_true = np.concatenate([w.reshape(-1) for w in rig.w_true])
    offs = np.cumsum([0] + rig.sizes)
    dose_true = rig.matvec(w_true)
    let_true = sum(m.matvec(w_true[a:b]) for m, a, b in zip(lets, offs, offs[1:]))
    v = int(np.argmax(dose_true))
    nx, ny, nz = rig.dims
    centre = (v % nx, (v // nx) % ny, v // (nx * ny))
    target = _box(rig.dims, centre, 5)
    behind = _box(rig.dims, (centre[0], centre[1], centre[2] - 9), 3)  # field 0 travels towards -z
    assert let_true[behind].max() > 0 and dose_true[target].min() > 0
    obj_d, obj_l = eng.create_objective(rig.dims), eng.create_objective(rig.dims)
    opts = []
    try:
        obj_d.add_roi(target)
        obj_d.add_term(abi.RTD_OBJ_SQ_DEVIATION, 0, 1.0, float(dose_true[target].mean()))
        obj_l.add_roi(behind)
        obj_l.add_term(abi.RTD_OBJ_SQ_OVERDOSE, 0, 1.0, 0.25 * float(let_true[behind].max()))

        def make(let=True):
            o = eng.create_optimizer(rig.fields, obj_d)
            opts.append(o)
            if let:
                o.set_let_objective(obj_l)
            return o
        n_it = 10
        opt = make()
        opt.run(n_it)
        rep, hist = opt.result()
        vals3 = opt.let_values()
        # the same loop from Python
        w0 = np.concatenate([np.asarray(f._beam.spotWeights, dtype=F).reshape(-1) for f in rig.fields])
        ref = OR.ReferenceOptimizer(None, None, None, w0)
        dD, dN, dG1, dG2 = (rig.alloc(4 * rig.nvox) for _ in range(4))
        dGrad = [rig.alloc(4 * n) for n in rig.sizes]
        f_parts = []
        for _ in range(n_it):
            ws = [ref.w[a:b].reshape(s) for a, b, s in zip(offs, offs[1:], rig.shapes)]
            rig.dose_of(ws, dD)
            eng.device_zero(dN, 4 * rig.nvox)
            for f, wf in zip(rig.fields, ws):
                dW = rig.alloc(wf.nbytes, zero=False)
                eng.to_device(dW, np.ascontiguousarray(wf, dtype=F))
                f.let_apply(dW, dN, init=False)
            v1, v2 = obj_d.eval(dD, dG1), obj_l.eval(dN, dG2)
            a, b = [], []
            for f, n, dg in zip(rig.fields, rig.sizes, dGrad):
                for call, dgv, out in ((f.dose_influence_apply_t, dG1, a), (f.let_apply_t, dG2, b)):
                    call(dgv, dg)
                    part = np.empty(n, dtype=F)
                    eng.to_host(part, dg)
                    out.append(part)
            grad = (np.concatenate(a) + np.concatenate(b)).astype(F)
            f_parts.append((float(v1[0]) + float(v2[0]), float(v1[0]), float(v2[0])))
            ref.advance(f_parts[-1][0], grad)
        want_hist = np.array(ref.history, dtype=np.float64)
        print("device history:", " ".join("%.6g" % x for x in hist))
        print("python history:", " ".join("%.6g" % x for x in want_hist))
        assert hist.size == n_it and np.array_equal(bits(hist), bits(want_hist))
        got_w = np.concatenate([x.reshape(-1) for x in rig.weights(opt)])
        got_b = np.concatenate([x.reshape(-1) for x in rig.weights(opt, best=True)])
        assert np.array_equal(bits(got_w), bits(ref.w)) and np.array_equal(bits(got_b), bits(ref.w_best))
        assert f_parts[0][2] > 0 and np.array_equal(bits(vals3), bits(np.array(f_parts[-1], dtype=np.float64)))
        assert rep["f_best"] <= hist[0] and rep["f_best"] == want_hist.min()
        # the LET dose volume is that of the iterate that entered the last iteration
        assert np.array_equal(bits(rig.volume(opt.let_dose())), bits(rig.volume(dN)))
        # removed again: the optimiser of section 12
        plain, removed = make(let=False), make()
        removed.set_let_objective(None)
        plain.run(5)
        removed.run(5)
        _, hp = same(rig, plain, removed)
        assert not np.array_equal(hp, hist[:5])
        with pytest.raises(rig.engine.RtdError):
            removed.let_dose()
        # launches only: run(3) with a LET objective, captured and replayed once, equals the direct call
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
        obj_d.destroy()
        obj_l.destroy()


def test_refusals(engine, synth, nuc_luts):
    """Every NOT_READY / INVALID_ARG case of the header; after each refusal the objects still work."""
    L = engine.lib()
    scn = hetero_scene(synth, 64, [0.0], spots=3, layers=1)
    b = scn.beams[0]
    table = luts.synth_let(synth)
    tp = lambda t: abi.fptr(t)                                        # noqa: E731
    nE, nS = table.shape
    bare = engine.Engine(0)
    try:                                                              # LUTs are not set
        assert L.rtd_set_let_table(bare._h, tp(table), nE, nS) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_set_let_table(bare._h, None, 0, 0) == abi.RTD_OK
    finally:
        bare.close()
    eng = engine.Engine(0)
    objs, opts, fields, bufs = [], [], [], []
    try:
        eng.set_options(options(0.0))
        eng.set_luts(synth)
        eng.set_ct(scn.ct)
        nvox = 64 ** 3
        dVol, dSp = eng.device_alloc(4 * nvox), eng.device_alloc(4 * b.spotWeights.size)
        bufs += [dVol, dSp]
        vol, sp = C.c_void_p(dVol), C.c_void_p(dSp)
        eng.device_zero(dVol, 4 * nvox)
        eng.to_device(dSp, np.ones(b.spotWeights.shape, dtype=F))
        # the table: dimensions, entries
        assert L.rtd_set_let_table(eng._h, tp(table), nE - 1, nS) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_set_let_table(eng._h, tp(table), nE, nS - 1) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_set_let_table(eng._h, tp(np.ascontiguousarray(table.T)), nS, nE) == abi.RTD_ERR_INVALID_ARG
        for bad in (-1.0, np.nan, np.inf):
            t = table.copy()
            t[nE // 2, nS // 3] = bad
            assert L.rtd_set_let_table(eng._h, tp(t), nE, nS) == abi.RTD_ERR_INVALID_ARG, bad
        f = eng.create_field(b, scn.dims)
        fields.append(f)
        # water_depth
        assert L.rtd_field_water_depth(eng._h, f._h, vol) == abi.RTD_ERR_NOT_READY
        r = eng.create_field(b, scn.dims, remote=True)
        assert L.rtd_field_water_depth(eng._h, r._h, vol) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_let_influence(eng._h, r._h) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_let_influence_apply(eng._h, r._h, sp, vol, 1) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_let_influence_apply_t(eng._h, r._h, vol, sp) == abi.RTD_ERR_INVALID_ARG
        r.destroy()
        # no matrix, no table
        pv, nnz = C.c_void_p(), C.c_size_t(0)
        assert L.rtd_field_let_influence(eng._h, f._h) == abi.RTD_ERR_NOT_READY
        d = f.dose_influence()
        assert d.nnz > 0
        assert L.rtd_field_water_depth(eng._h, f._h, None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_let_influence(eng._h, f._h) == abi.RTD_ERR_NOT_READY          # a matrix, no table
        assert L.rtd_field_let_influence_apply(eng._h, f._h, sp, vol, 1) == abi.RTD_ERR_NOT_READY
        const2 = np.full_like(table, 2.0)
        eng.set_let_table(const2)
        for call in (lambda: L.rtd_field_let_influence_apply(eng._h, f._h, sp, vol, 1), lambda: L.rtd_field_let_influence_apply_t(eng._h, f._h, vol, sp),
                     lambda: L.rtd_field_let_influence_device(eng._h, f._h, C.byref(pv), C.byref(nnz))):
            assert call() == abi.RTD_ERR_NOT_READY                    # a table, no let_influence yet
        f.let_influence()
        assert L.rtd_field_let_influence_apply(eng._h, f._h, None, vol, 1) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_let_influence_apply(eng._h, f._h, sp, None, 1) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_let_influence_apply_t(eng._h, f._h, None, sp) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_let_influence_apply_t(eng._h, f._h, vol, None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_let_influence_device(eng._h, f._h, None, C.byref(nnz)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_let_influence_device(eng._h, f._h, C.byref(pv), None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_let_average(eng._h, None, vol, nvox, C.c_float(0.0), vol) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_let_average(eng._h, vol, vol, nvox, C.c_float(-1.0), vol) == abi.RTD_ERR_INVALID_ARG

        def works():
            """N 1 = 2 * Dij 1 under the constant table: the field and its LET values still work."""
            out, ref = np.empty(nvox, dtype=F), np.empty(nvox, dtype=F)
            for call, res in ((f.let_apply, out), (f.dose_influence_apply, ref)):
                eng.device_zero(dVol, 4 * nvox)
                call(dSp, dVol, init=False)
                eng.to_host(res, dVol)
            assert ref.max() > 0 and np.array_equal(bits(out), bits((2.0 * ref).astype(F)))
        works()
        # a new table: NOT_READY until let_influence again (removing the table likewise)
        eng.set_let_table(const2.copy())
        assert L.rtd_field_let_influence_apply(eng._h, f._h, sp, vol, 1) == abi.RTD_ERR_NOT_READY
        assert L.rtd_field_let_influence_apply_t(eng._h, f._h, vol, sp) == abi.RTD_ERR_NOT_READY
        f.let_influence()
        works()
        eng.set_let_table(None)
        assert L.rtd_field_let_influence_apply(eng._h, f._h, sp, vol, 1) == abi.RTD_ERR_NOT_READY
        assert L.rtd_field_let_influence(eng._h, f._h) == abi.RTD_ERR_NOT_READY
        eng.set_let_table(const2)
        f.let_influence()
        works()
        # a new matrix discards the LET values
        d2 = f.dose_influence()
        assert d2.nnz == d.nnz
        assert L.rtd_field_let_influence_apply(eng._h, f._h, sp, vol, 1) == abi.RTD_ERR_NOT_READY
        assert L.rtd_field_let_influence_device(eng._h, f._h, C.byref(pv), C.byref(nnz)) == abi.RTD_ERR_NOT_READY
        # the optimiser's LET objective
        f2 = eng.create_field(b, scn.dims)
        fields.append(f2)
        f2.dose_influence()
        has = np.bincount(d.indices, minlength=nvox) > 0

        def objective(dims=scn.dims, terms=True):
            o = eng.create_objective(dims)
            objs.append(o)
            if dims == scn.dims:
                o.add_roi(has)
                if terms:
                    o.add_term(abi.RTD_OBJ_SQ_OVERDOSE, 0, 1.0, 0.0)
            return o
        obj, let_obj = objective(), objective()
        opt = eng.create_optimizer([f], obj)
        opts.append(opt)
        so = lambda o, lo: L.rtd_optimizer_set_let_objective(eng._h, o._h, lo._h if lo is not None else None)   # noqa: E731
        assert so(opt, let_obj) == abi.RTD_ERR_NOT_READY             # the field's LET values went with the old matrix
        f.let_influence()
        assert L.rtd_optimizer_set_let_objective(eng._h, None, let_obj._h) == abi.RTD_ERR_INVALID_ARG
        assert so(opt, objective(terms=False)) == abi.RTD_ERR_INVALID_ARG
        assert so(opt, objective(dims=(32, 64, 64))) == abi.RTD_ERR_INVALID_ARG
        assert so(opt, obj) == abi.RTD_ERR_INVALID_ARG               # the optimiser's own objective object
        pd, v3 = C.c_void_p(), (C.c_double * 3)()
        assert L.rtd_optimizer_let_dose(eng._h, opt._h, C.byref(pd)) == abi.RTD_ERR_NOT_READY
        assert L.rtd_optimizer_let_values(eng._h, opt._h, v3) == abi.RTD_ERR_NOT_READY
        two = eng.create_optimizer([f, f2], obj)
        opts.append(two)
        assert so(two, let_obj) == abi.RTD_ERR_NOT_READY             # f2 has a matrix and no LET values
        rob = eng.create_robust_optimizer([[f], [f2]], obj, abi.RTD_ROBUST_EXPECTED)
        vox = eng.create_voxelwise_optimizer([[f], [f2]], obj)
        opts += [rob, vox]
        f2.let_influence()
        assert so(rob, let_obj) == abi.RTD_ERR_INVALID_ARG
        assert so(vox, let_obj) == abi.RTD_ERR_INVALID_ARG
        # after the refusals everything works: set, run, read, remove
        assert so(opt, let_obj) == abi.RTD_OK and so(two, let_obj) == abi.RTD_OK
        opt.run(2)
        two.run(2)
        vals = opt.let_values()
        rep, hist = opt.result()
        assert hist.size == 2 and vals[0] == hist[-1] == vals[1] + vals[2] and vals[2] > 0
        assert opt.let_dose() and two.result()[0]["iterations"] == 2
        # a table set after set_let_objective: the run is refused until the LET values are made again
        eng.set_let_table(const2.copy())
        assert L.rtd_optimizer_run(eng._h, opt._h, 1) == abi.RTD_ERR_NOT_READY
        f.let_influence()
        f2.let_influence()
        opt.run(1)
        assert opt.result()[0]["iterations"] == 3
        assert so(opt, None) == abi.RTD_OK
        assert L.rtd_optimizer_let_dose(eng._h, opt._h, C.byref(pd)) == abi.RTD_ERR_NOT_READY
        opt.run(1)
        works()
        # nuclear_corr: no water depth (and no matrix, as before)
        engn = engine.Engine(0)
        try:
            engn.set_options(options(0.0, nuclear=abi.RTD_NUC_SOUKUP))
            engn.set_luts(nuc_luts)
            engn.set_ct(scn.ct)
            fn = engn.create_field(b, scn.dims)
            dv = engn.device_alloc(4 * nvox)
            engn.device_zero(dv, 4 * nvox)
            fn.compute(dv)
            fn.finish()
            assert L.rtd_field_water_depth(engn._h, fn._h, C.c_void_p(dv)) == abi.RTD_ERR_INVALID_ARG
            fn.compute(dv)                                            # still usable
            fn.finish()
            engn.device_free(dv)
            fn.destroy()
        finally:
            engn.close()
    finally:
        for o in opts:
            o.destroy()
        for o in objs:
            o.destroy()
        for p in bufs:
            eng.device_free(p)
        for fl in fields:
            fl.destroy()
        eng.close()
