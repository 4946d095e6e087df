"""GPU tests of the compact dose-influence matrix: rtd_field_dose_influence_compact / _compact_info / _compact_device /
_apply_compact / _apply_t_compact and rtd_optimizer_create_compact (include/rtd.h "Compact dose-influence matrix").

The reference is tests/dij_compact_reference.py, the format and the two trees restated in numpy from the header's prose and fed the
CSC that rtd_field_dose_influence_copy returns: packed arrays and products are compared bit for bit (a NaN against a NaN: the payload
is the one thing a NaN + NaN leaves open). Against the plain products the bound follows from the format: per entry
|v^ - v| <= max(2^-11 |v|, 2^-25 s_j), plus tree_reference.tree_bound of both trees. The ray-weight cut-off is 0 throughout."""
import ctypes as C

import numpy as np
import pytest

import dij_compact_reference as DC
import optimizer_reference as OR
import tree_reference as TR
from gpu_plan_rigs import OptimizerRig, same
from gpu_support import FieldRig, bits, hetero_scene, options, rig_fixture, switches, worst_ratio
from raytracedicom_amd import abi, luts, rbe, scenarios

pytestmark = pytest.mark.gpu

F = np.float32
TREES = ((16, 1), (16, 2), (16, 4), (32, 1), (32, 2), (32, 4))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F).reshape(-1), np.ascontiguousarray(b, dtype=F).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


class CompactRig(FieldRig):
    """The single-field rig with the compact calls beside the plain ones."""

    def fetch(self, ptr, n, dtype):
        out = np.empty(int(n), dtype=dtype)
        if n:
            self.eng.to_host(out, ptr)
        return out

    def arrays(self, f, n_spots):
        """The packed arrays of the field's compact form as numpy arrays, and its info."""
        info, d = f.dose_influence_compact_info(), f.dose_influence_compact_device()
        a = {"scale": self.fetch(d.scale, n_spots, F), "csc_code": self.fetch(d.csc_code, d.nnz, np.uint16),
             "csc_base": self.fetch(d.csc_base, d.n_groups, np.int32), "row_ptr": self.fetch(d.row_ptr, d.n_rows + 1, np.int64),
             "row_code": self.fetch(d.row_code, d.row_entries, np.uint16), "row_col": self.fetch(d.row_col, d.row_entries, np.uint16),
             "csc_offset": self.fetch(d.csc_offset, d.nnz, np.uint16) if info["row_bits"] == 16 else None,
             "csc_rows": self.fetch(d.csc_rows, d.nnz, np.int32) if info["row_bits"] == 32 else None, "box": tuple(d.box)}
        assert (d.csc_offset is None) == (info["row_bits"] == 32) and (d.csc_rows is None) == (info["row_bits"] == 16), info
        assert d.nnz == info["nnz"] and d.row_entries == info["row_entries"], info
        return a, info

    def apply_c(self, f, w, into=None, init=True):
        vol = np.full(self.shape, np.nan, dtype=F) if into is None else np.ascontiguousarray(into, dtype=F)
        w = np.ascontiguousarray(w, dtype=F)
        dW = self.eng.device_alloc(w.nbytes)
        try:
            self.eng.to_device(dW, w)
            self.eng.to_device(self.dDose, vol)
            f.dose_influence_apply_compact(dW, self.dDose, init=init)
            out = np.empty(self.shape, dtype=F)
            self.eng.to_host(out, self.dDose)
        finally:
            self.eng.device_free(dW)
        return out

    def apply_t_c(self, f, g):
        return self._spot_call(f, f.dose_influence_apply_t_compact, g)


rig_of = rig_fixture(CompactRig)


class Restated:
    """The compact form of a copied CSC by the restatement, at the tree (G, E) and over the row box the engine reports."""

    def __init__(self, d, dims, box, G, E):
        self.d, self.dims, self.box, self.G, self.E = d, dims, box, G, E
        self.scale, _, self.codes = DC.quantize(d.indptr, d.data)
        self.base, self.off, self.row_bits = DC.pack_csc(d.indptr, d.indices)
        self.n_rows = int(box[3]) * int(box[4]) * int(box[5])
        self.rows = DC.box_rows(d.indices, dims, box)
        self.row_ptr, self.row_code, self.row_col, self.count = DC.pack_rows(d.indptr, self.rows, self.codes, self.n_rows, E)
        self.vox = DC.box_voxels(dims, box)

    def apply(self, w, into, init):
        sums, count = DC.apply_tree(self.d.indptr, self.rows, self.codes, self.scale, w, self.n_rows, self.G, self.E)
        out = np.array(into, dtype=F).reshape(-1).copy()
        with np.errstate(invalid="ignore", over="ignore"):
            if init:
                out[self.vox] = sums
            else:
                has = count > 0
                out[self.vox[has]] = out[self.vox[has]] + sums[has]
        return out

    def apply_t(self, g):
        return DC.apply_t_tree(self.d.indptr, self.d.indices, self.codes, self.scale, np.asarray(g, dtype=F).reshape(-1))


def check_packed(a, info, r, d):
    """Test 1: scales, codes, columns, bases, offsets and row_bits equal the restatement bit for bit."""
    assert (info["value_bits"], info["col_bits"], info["row_bits"]) == (16, 16, r.row_bits), info
    assert (info["lanes_per_row"], info["entries_per_lane"], info["nnz"], info["row_entries"]) == (r.G, r.E, d.nnz, r.row_code.size), info
    assert np.array_equal(bits(a["scale"]), bits(r.scale))
    assert np.array_equal(a["csc_code"], r.codes) and np.array_equal(a["csc_base"], r.base)
    if r.row_bits == 16:
        assert np.array_equal(a["csc_offset"], r.off)
    else:
        assert np.array_equal(a["csc_rows"], d.indices)
    assert np.array_equal(a["row_ptr"], r.row_ptr) and np.array_equal(a["row_code"], r.row_code) and np.array_equal(a["row_col"], r.row_col)


def vectors(rng, shape, n_vox_shape, live_col, live_vox):
    """(name, w, g) triples: one-hot, random, and a vector with a +inf and a zero at live places."""
    w_hot, g_hot = np.zeros(shape, dtype=F), np.zeros(n_vox_shape, dtype=F)
    w_hot.reshape(-1)[live_col] = 1.0
    g_hot.reshape(-1)[live_vox] = 1.0
    w_rand = (100.0 * rng.random(shape)).astype(F)
    g_rand = (rng.random(n_vox_shape) - 0.5).astype(F)
    w_inf, g_inf = w_rand.copy(), g_rand.copy()
    w_inf.reshape(-1)[live_col] = np.inf
    w_inf.reshape(-1)[(live_col + 1) % w_inf.size] = 0.0
    g_inf.reshape(-1)[live_vox] = np.inf
    g_inf.reshape(-1)[live_vox + 1] = 0.0
    return (("one-hot", w_hot, g_hot), ("random", w_rand, g_rand), ("inf and zero", w_inf, g_inf))


def check_products(rig, f, r, rng, names=("one-hot", "random", "inf and zero")):
    """Test 2: apply_compact (init 0 and 1) and apply_t_compact equal the restatement's trees bit for bit."""
    d = r.d
    lens = np.diff(d.indptr)
    live_col = int(np.argmax(lens))
    live_vox = int(d.indices[d.indptr[live_col] + lens[live_col] // 2])
    shape = f._beam.spotWeights.shape
    base = (rng.random(rig.shape) - 0.5).astype(F)
    for name, w, g in vectors(rng, shape, rig.shape, live_col, live_vox):
        if name not in names:
            continue
        for init in (True, False):
            into = np.full(rig.shape, np.nan, dtype=F) if init else base
            got = rig.apply_c(f, w, into=into, init=init)
            assert same_bits(got, r.apply(w, into, init)), (name, init, r.G, r.E)
        assert same_bits(rig.apply_t_c(f, g), r.apply_t(g)), (name, r.G, r.E)
        if name == "inf and zero":
            assert np.isnan(got).any() or np.isinf(got).any()


@pytest.fixture(scope="module")
def dense_case(engine, synth):
    """One 96^3 field of 75 spots 4 mm apart (rows of every length up to 75), its copied CSC, its compact form at the default tree and
    the restatement of it: computed once, read by several tests, changed by none."""
    scn = hetero_scene(synth, 96, [0.0], spots=5, pitch=4.0, layers=3)
    rig = CompactRig(engine, scn, options(0.0))
    f = rig.field(scn.beams[0])
    d = f.dose_influence()
    f.dose_influence_compact()
    a, info = rig.arrays(f, d.shape[1])
    r = Restated(d, rig.dims, a["box"], info["lanes_per_row"], info["entries_per_lane"])
    yield rig, f, d, a, info, r
    rig.close()


def test_packed_arrays_equal_the_restatement(dense_case):
    """Test 1 on the cubic rig, which reports 16-bit rows; the rig holds what test 2 needs (asserted on the CPU from the copied CSC)."""
    rig, f, d, a, info, r = dense_case
    G, E = info["lanes_per_row"], info["entries_per_lane"]
    assert (G, E) in TREES and info["row_bits"] == 16 and info["plain_released"] == 0
    has = set(np.unique(r.count).tolist())
    assert {0, 1, G * E - 1, G * E, G * E + 1} <= has, (G, E, sorted(has)[-5:])
    assert np.diff(d.indptr).max() > 2048                            # (a column of two chunks or more)
    check_packed(a, info, r, d)
    # the bytes: 4 B per entry on each side (pads and tables aside) against 16
    assert info["plain_bytes"] == 16 * d.nnz and info["released_bytes"] == 0
    assert 8 * d.nnz <= info["compact_bytes"] <= 8 * d.nnz + 4 * (r.row_code.size - d.nnz) + 4 * r.base.size + 8 * (r.n_rows + 1) + 8 * d.shape[1]


def test_products_equal_the_restated_trees(dense_case):
    """Test 2 at the tree the info reports."""
    rig, f, d, a, info, r = dense_case
    check_products(rig, f, r, np.random.default_rng(31))


def test_products_against_the_plain_ones(dense_case):
    """Test 3: |Dc w - D w| per voxel <= sum_j max(2^-11 |v|, 2^-25 s_j) |w_j| + the tree bounds of both trees; the transpose likewise."""
    rig, f, d, a, info, r = dense_case
    G, E = r.G, r.E
    rng = np.random.default_rng(41)
    w = (100.0 * rng.random(f._beam.spotWeights.shape)).astype(F)
    g = (rng.random(rig.shape) - 0.5).astype(F)
    col = np.repeat(np.arange(d.shape[1]), np.diff(d.indptr))
    eb = DC.entry_bound(d.data, r.scale, d.indptr)
    vhat = DC.dequantize(r.codes, r.scale, d.indptr)[1]
    absw, absg = np.abs(w.reshape(-1).astype(np.float64)), np.abs(g.reshape(-1).astype(np.float64))
    n_vox = d.shape[0]
    plain = rig.product(f, w).astype(np.float64)
    comp = rig.apply_c(f, w, into=np.zeros(rig.shape, dtype=F), init=True).reshape(-1).astype(np.float64)
    n_row = np.bincount(d.indices, minlength=n_vox)
    bound = (np.bincount(d.indices, weights=eb * absw[col], minlength=n_vox)
             + TR.tree_bound(DC.apply_depth(n_row, G, E), np.bincount(d.indices, weights=np.abs(vhat) * absw[col], minlength=n_vox))
             + TR.tree_bound(TR.apply_depth(n_row), np.bincount(d.indices, weights=np.abs(d.data.astype(np.float64)) * absw[col], minlength=n_vox)))
    err = np.abs(comp - plain)
    print("apply: worst |compact - plain| / bound = %.3g" % worst_ratio(err, bound))
    assert plain.max() > 0 and np.any(err > 0) and np.all(err <= bound), worst_ratio(err, bound)
    plain_t = rig.apply_t(f, g).reshape(-1).astype(np.float64)
    comp_t = rig.apply_t_c(f, g).reshape(-1).astype(np.float64)
    n_col = np.diff(d.indptr)
    n_sp = d.shape[1]
    bound_t = (np.bincount(col, weights=eb * absg[d.indices], minlength=n_sp)
               + TR.tree_bound(TR.apply_t_depth(n_col), np.bincount(col, weights=np.abs(vhat) * absg[d.indices], minlength=n_sp))
               + TR.tree_bound(TR.apply_t_depth(n_col), np.bincount(col, weights=np.abs(d.data.astype(np.float64)) * absg[d.indices], minlength=n_sp)))
    err_t = np.abs(comp_t - plain_t)
    print("apply_t: worst |compact - plain| / bound = %.3g" % worst_ratio(err_t, bound_t))
    assert np.abs(plain_t).max() > 0 and np.any(err_t > 0) and np.all(err_t <= bound_t), worst_ratio(err_t, bound_t)


@pytest.mark.parametrize("tree", [t for t in TREES], ids=lambda t: "G%d_E%d" % t)
def test_every_tree_of_the_family(rig_of, synth, tree):
    """Tests 1 and 2 at every (G, E) the build can be asked for, on a 64^3 field (random vectors; the default tree has the full set above)."""
    G, E = tree
    scn = hetero_scene(synth, 64, [30.0], spots=5, pitch=6.0, layers=2)
    rig = rig_of(scn, options(0.0))
    f = rig.field(scn.beams[0])
    d = f.dose_influence()
    with switches(RTD_DIJC_LANES=str(G), RTD_DIJC_PER=str(E)):
        f.dose_influence_compact()
    a, info = rig.arrays(f, d.shape[1])
    assert (info["lanes_per_row"], info["entries_per_lane"]) == (G, E)
    r = Restated(d, rig.dims, a["box"], G, E)
    assert r.count.max() > G and (E == 1 or np.any(r.count % E != 0))  # (rows longer than the lanes; rows that need pads)
    check_packed(a, info, r, d)
    check_products(rig, f, r, np.random.default_rng(7), names=("random", "inf and zero"))


def test_two_crossing_fields_accumulate(rig_of, synth):
    """Two crossing fields into one volume, init = 0 after init = 1: the restatement's bits, and voxels that both fields reach."""
    ct, _ = scenarios.hetero_phantom(64)
    scn = scenarios.hetero_ct(synth, n=64, spots=3, pitch=8.0, n_layers=2, angles=[0.0, 90.0], ct=ct, seed=5)
    rig = rig_of(scn, options(0.0))
    rng = np.random.default_rng(3)
    vol = np.full(rig.shape, np.nan, dtype=F)
    want = vol.reshape(-1).copy()
    reach = []
    for i, b in enumerate(scn.beams):
        f = rig.field(b)
        d = f.dose_influence()
        f.dose_influence_compact()
        a, info = rig.arrays(f, d.shape[1])
        r = Restated(d, rig.dims, a["box"], info["lanes_per_row"], info["entries_per_lane"])
        w = (100.0 * rng.random(b.spotWeights.shape)).astype(F)
        if i == 0:
            vol[:] = 0.0                                              # (field 0 accumulates into zeros over the whole volume)
            want[:] = 0.0
        vol = rig.apply_c(f, w, into=vol, init=False)
        want = r.apply(w, want, False)
        reach.append(np.bincount(d.indices, minlength=d.shape[0]) > 0)
    assert same_bits(vol, want) and np.count_nonzero(reach[0] & reach[1]) > 0 and np.nanmax(vol) > 0


def wide_slice_scene(synth):
    """A 64^3 CT with a dose grid of 512 x 256 x 8 voxels over it: a slice holds 131 072 voxels, so the 64-entry group that holds a
    column's last entries of one slice and its first of the next spans more than 65 535."""
    scn = hetero_scene(synth, 64, [0.0], spots=3, pitch=8.0, layers=1)
    dims = (512, 256, 8)
    s = np.array([dims[0] / 64.0, dims[1] / 64.0, dims[2] / 64.0])
    t = scn.beams[0].gantryToDoseIdx
    m = (s[:, None] * np.asarray(t.m, dtype=np.float64).reshape(3, 3)).astype(F)
    v = (s * np.asarray(t.v, dtype=np.float64).reshape(3) + (s - 1.0) / 2.0).astype(F)   # dose index i = s c + (s - 1) / 2 of CT index c
    scn.beams[0] = scn.beams[0].replace(gantryToDoseIdx=scenarios.Float3AffineTransform(m, v))
    return scn, dims


def test_wide_slices_keep_32_bit_rows(rig_of, synth):
    """Test 4: a dose grid whose slice holds more than 65 535 voxels reports row_bits == 32 and passes tests 1 and 2."""
    scn, dims = wide_slice_scene(synth)
    rig = rig_of(scn, options(0.0), dims)
    f = rig.field(scn.beams[0])
    d = f.dose_influence()
    assert d.nnz > 0
    f.dose_influence_compact()
    a, info = rig.arrays(f, d.shape[1])
    r = Restated(d, rig.dims, a["box"], info["lanes_per_row"], info["entries_per_lane"])
    assert r.row_bits == 32 and info["row_bits"] == 32
    check_packed(a, info, r, d)
    check_products(rig, f, r, np.random.default_rng(13), names=("random", "inf and zero"))
    assert info["compact_bytes"] >= 6 * d.nnz and info["plain_bytes"] == 16 * d.nnz


opt_rig_of = rig_fixture(OptimizerRig, "opt_rig_of")


def add_coupled_terms(rig):
    """One DVH and one EUD term beside the rig's four plain kinds."""
    rig.obj.add_dvh_term(abi.RTD_OBJ_MAX_DVH, 1, 2.0, 0.25 * rig.level, 0.2)
    rig.obj.add_eud_term(abi.RTD_OBJ_SQ_MAX_EUD, 1, 1.5, 0.2 * rig.level, 4.0)


def python_loop(rig, n_it, dD, dG):
    """The compact optimiser's iteration driven from Python with the public calls -> the reference optimiser after n_it steps."""
    eng = rig.eng
    offs = np.cumsum([0] + rig.sizes)
    w0 = np.concatenate([np.asarray(f._beam.spotWeights, dtype=F).reshape(-1) for f in rig.fields])
    ref = OR.ReferenceOptimizer(None, None, None, w0)
    dGrad = [rig.alloc(4 * n) for n in rig.sizes]
    for _ in range(n_it):
        eng.device_zero(dD, 4 * rig.nvox)
        for f, a, b in zip(rig.fields, offs, offs[1:]):
            dW = rig.alloc(4 * (b - a), zero=False)
            eng.to_device(dW, np.ascontiguousarray(ref.w[a:b], dtype=F))
            f.dose_influence_apply_compact(dW, dD, init=False)
        vals = rig.obj.eval(dD, dG)
        parts = []
        for f, n, dg in zip(rig.fields, rig.sizes, dGrad):
            f.dose_influence_apply_t_compact(dG, dg)
            part = np.empty(n, dtype=F)
            eng.to_host(part, dg)
            parts.append(part)
        ref.advance(float(vals[0]), np.concatenate(parts))
    return ref


def test_compact_optimizer_equals_a_python_loop(opt_rig_of, synth):
    """Test 5: ten iterations with the four plain term kinds, a DVH and an EUD term equal, bit for bit in weights, best weights, dose
    and history, a loop of apply_compact, rtd_objective_eval, apply_t_compact and the step rule of tests/optimizer_reference.py;
    run(10) equals run(5) twice; the two products captured into a graph and replayed give the direct calls' bits; the history differs
    from the plain optimiser's (other products) by little; set_let_objective and set_rbe refuse it."""
    import torch
    rig = opt_rig_of(hetero_scene(synth, 96, (0.0, 90.0)))
    eng = rig.eng
    add_coupled_terms(rig)
    with pytest.raises(rig.engine.RtdError) as ei:                     # no compact form yet
        eng.create_compact_optimizer(rig.fields, rig.obj)
    assert ei.value.status == abi.RTD_ERR_NOT_READY and "rtd_field_dose_influence_compact" in str(ei.value)
    for f in rig.fields:
        f.dose_influence_compact()
    n_it = 10
    opt = eng.create_compact_optimizer(rig.fields, rig.obj)
    rig.opts.append(opt)
    opt.run(n_it)
    rep, hist = opt.result()
    dD, dG = rig.alloc(4 * rig.nvox), rig.alloc(4 * rig.nvox)
    ref = python_loop(rig, n_it, dD, dG)
    want = np.array(ref.history, dtype=np.float64)
    print("device history:", " ".join("%.6g" % x for x in hist))
    print("python history:", " ".join("%.6g" % x for x in want))
    assert hist.size == n_it and np.array_equal(bits(hist), bits(want))
    got_w = np.concatenate([x.reshape(-1) for x in rig.weights(opt)])
    got_b = np.concatenate([x.reshape(-1) for x in rig.weights(opt, best=True)])
    assert np.array_equal(bits(got_w), bits(ref.w)) and np.array_equal(bits(got_b), bits(ref.w_best))
    assert np.array_equal(bits(rig.volume(opt.dose())), bits(rig.volume(dD))) and rig.volume(dD).max() > 0
    assert rep["f_best"] == want.min() and want.min() < want[0]
    # run(10) = run(5) twice
    halves = eng.create_compact_optimizer(rig.fields, rig.obj)
    rig.opts.append(halves)
    halves.run(5)
    halves.run(5)
    same(rig, opt, halves)
    # beside the plain optimiser: other bits, the same plan to the format's accuracy (reported, not bounded)
    plain = rig.optimizer()
    plain.run(n_it)
    _, hp = plain.result()
    print("plain history: ", " ".join("%.6g" % x for x in hp))
    assert not np.array_equal(bits(hp), bits(hist))
    with pytest.raises(rig.engine.RtdError) as ei:
        opt.set_let_objective(rig.obj)
    assert ei.value.status == abi.RTD_ERR_INVALID_ARG and "compact" in str(ei.value)
    model = eng.create_rbe(rig.dims, rbe.tissue("mcnamara", 0.5, 0.05))
    try:
        with pytest.raises(rig.engine.RtdError) as ei:
            opt.set_rbe(model)
        assert ei.value.status == abi.RTD_ERR_INVALID_ARG and "compact" in str(ei.value)
    finally:
        model.destroy()
    # launches only: the two products captured and replayed
    f = rig.fields[0]
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(5)
    w = (100.0 * torch.rand(rig.shapes[0], generator=gen)).to(dev)
    nx, ny, nz = rig.dims
    gvol = (torch.rand((nz, ny, nx), generator=gen) - 0.5).to(dev)
    ref_d = torch.full((nz, ny, nx), float("nan"), dtype=torch.float32, device=dev)
    ref_t = torch.full(tuple(rig.shapes[0]), float("nan"), dtype=torch.float32, device=dev)
    out_d, out_t = ref_d.clone(), ref_t.clone()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.sync()
    eng.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            f.dose_influence_apply_compact(w.data_ptr(), ref_d.data_ptr(), init=True)
            f.dose_influence_apply_t_compact(gvol.data_ptr(), ref_t.data_ptr())
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                f.dose_influence_apply_compact(w.data_ptr(), out_d.data_ptr(), init=True)
                f.dose_influence_apply_t_compact(gvol.data_ptr(), out_t.data_ptr())
            for _ in range(2):
                g.replay()
        torch.cuda.synchronize()
    finally:
        eng.set_stream(None)
    assert float(torch.nan_to_num(ref_d).max()) > 0 and float(ref_t.abs().max()) > 0
    assert torch.equal(ref_d.view(torch.int32), out_d.view(torch.int32)) and torch.equal(ref_t.view(torch.int32), out_t.view(torch.int32))


def refused(engine_mod, call, status=abi.RTD_ERR_NOT_READY, word="release_plain"):
    with pytest.raises(engine_mod.RtdError) as ei:
        call()
    assert ei.value.status == status and word in str(ei.value), str(ei.value)


def test_release_plain(engine, synth):
    """Test 6. Two identical runs, one with release_plain: the drop in used device memory equals released_bytes to within the
    allocator's granularity (2 MiB per freed buffer: device memory is handed out in fragments of at most that size); every consumer
    of the plain form answers RTD_ERR_NOT_READY with a message that names release_plain; the compact products and the compact
    optimiser give the bits they gave before; a fresh rtd_field_dose_influence restores everything and the compact optimiser created
    before it refuses to run."""
    import torch
    scn = hetero_scene(synth, 96, [0.0], spots=5, pitch=4.0, layers=3)
    b = scn.beams[0]
    rng = np.random.default_rng(19)
    w = (100.0 * rng.random(b.spotWeights.shape)).astype(F)
    g = (rng.random(scn.ct.shape) - 0.5).astype(F)
    used, keep = {}, {}
    for release in (False, True):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        rig = CompactRig(engine, scn, options(0.0))
        try:
            eng = rig.eng
            f = rig.field(b)
            d = f.dose_influence()
            f.dose_influence_compact()
            before = (rig.apply_c(f, w), rig.apply_t_c(f, g))          # (allocates the rig's g volume in both runs alike)
            obj = eng.create_objective(rig.dims)
            target = np.zeros(d.shape[0], dtype=bool)
            target[np.unique(d.indices)[::7]] = True
            obj.add_roi(target)
            obj.add_term(abi.RTD_OBJ_SQ_DEVIATION, 0, 1.0, float(d.matvec(b.spotWeights)[target].mean()))
            copt = eng.create_compact_optimizer([f], obj)
            copt.run(3)
            hist0 = copt.result()[1]
            plain_opt = eng.create_optimizer([f], obj)
            if release:
                f.dose_influence_compact(release_plain=True)
            eng.sync()
            info = f.dose_influence_compact_info()
            used[release] = free0 - torch.cuda.mem_get_info(0)[0]
            keep[release] = info
            if release:
                assert info["plain_released"] == 1 and info["released_bytes"] == info["plain_bytes"] == 16 * d.nnz, info
                E = engine
                L = engine.lib()
                p = [C.c_void_p() for _ in range(3)]
                n = C.c_size_t(0)
                dW = eng.device_alloc(w.nbytes)
                refused(E, lambda: f.dose_influence_device())
                refused(E, lambda: eng._check(L.rtd_field_dose_influence_copy(eng._h, f._h, p[0], p[1], p[2])))
                refused(E, lambda: f.dose_influence_apply(dW, rig.dDose, init=True))
                refused(E, lambda: f.dose_influence_apply_t(rig.dDose, dW))
                refused(E, lambda: f.dose_influence_apply_set(dW, rig.dDose, 1, init=True))
                refused(E, lambda: f.dose_influence_apply_t_set(rig.dDose, dW, 1))
                refused(E, lambda: f.dose_influence_prepare())
                eng.set_let_table(luts.synth_let(synth))
                refused(E, lambda: f.let_influence())
                refused(E, lambda: f.let_apply(dW, rig.dDose, init=True))
                refused(E, lambda: f.let_apply_t(rig.dDose, dW))
                refused(E, lambda: f.let_influence_device())
                refused(E, lambda: eng.create_optimizer([f], obj))
                refused(E, lambda: eng.create_lbfgs_optimizer([f], obj))
                refused(E, lambda: eng.create_robust_optimizer([[f]], obj, abi.RTD_ROBUST_EXPECTED))
                refused(E, lambda: eng.create_voxelwise_optimizer([[f]], obj))
                refused(E, lambda: eng.create_planset([f], obj, [[(abi.RTD_OBJ_SQ_DEVIATION, 0, 1.0, 1.0)]]))
                refused(E, lambda: plain_opt.run(1))                   # created before the release
                eng.device_free(dW)
                # the compact side goes on with the same bits
                after = (rig.apply_c(f, w), rig.apply_t_c(f, g))
                assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
                copt2 = eng.create_compact_optimizer([f], obj)
                copt2.run(3)
                assert np.array_equal(bits(copt2.result()[1]), bits(hist0))
                copt2.destroy()
                f.dose_influence_compact(release_plain=True)           # (a second call: nothing left to do)
                # a fresh matrix restores everything; the compact form went with the old one
                d2 = f.dose_influence()
                assert d2.nnz == d.nnz and np.array_equal(d2.data, d.data) and np.array_equal(d2.indices, d.indices)
                assert same_bits(rig.product(f, w), rig.apply(f, w, into=np.zeros(rig.shape, dtype=F)))
                refused(E, lambda: f.dose_influence_apply_compact(rig.dDose, rig.dDose), word="rtd_field_dose_influence_compact")
                refused(E, lambda: copt.run(1), word="computed again")
                plain_opt.run(1)                                       # (the plain optimiser notes nothing: it runs on the new matrix)
                f.dose_influence_compact()
                again = (rig.apply_c(f, w), rig.apply_t_c(f, g))
                assert same_bits(before[0], again[0]) and same_bits(before[1], again[1])
                refused(E, lambda: copt.run(1), word="computed again")
            copt.destroy()
            plain_opt.destroy()
            obj.destroy()
        finally:
            rig.close()
    drop = used[False] - used[True]
    want = keep[True]["released_bytes"]
    print("device memory in use: %d B kept, %d B released; drop %d B against released_bytes %d B" % (used[False], used[True], drop, want))
    assert keep[False]["released_bytes"] == 0 and keep[False]["plain_bytes"] == want
    assert abs(drop - want) <= 4 * (2 << 20), (drop, want)             # four buffers freed: CSC rows, values, companion columns, values


def test_refusals(engine, synth):
    """No matrix: NOT_READY. A remote field, a nuclear_corr field, a non-zero reserved word, release_plain above 1, a null pointer:
    INVALID_ARG. The field stays usable."""
    L = engine.lib()
    scn = hetero_scene(synth, 64, [0.0], spots=3, layers=1)
    b = scn.beams[0]
    eng = engine.Engine(0)
    try:
        eng.set_options(options(0.0))
        eng.set_luts(synth)
        eng.set_ct(scn.ct)
        f = eng.create_field(b, scn.dims)
        info, dev = abi.RtdDijCompactInfo(), abi.RtdDijCompactDevice()
        dVol, dSp = eng.device_alloc(4 * 64 ** 3), eng.device_alloc(4 * b.spotWeights.size)
        vol, sp = C.c_void_p(dVol), C.c_void_p(dSp)
        assert L.rtd_field_dose_influence_compact(eng._h, f._h, None) == abi.RTD_ERR_NOT_READY
        assert L.rtd_field_dose_influence_compact_info(eng._h, f._h, C.byref(info)) == abi.RTD_ERR_NOT_READY
        assert L.rtd_field_dose_influence_compact_device(eng._h, f._h, C.byref(dev)) == abi.RTD_ERR_NOT_READY
        assert L.rtd_field_dose_influence_apply_compact(eng._h, f._h, sp, vol, 1) == abi.RTD_ERR_NOT_READY
        assert L.rtd_field_dose_influence_apply_t_compact(eng._h, f._h, vol, sp) == abi.RTD_ERR_NOT_READY
        d = f.dose_influence()
        assert L.rtd_field_dose_influence_apply_compact(eng._h, f._h, sp, vol, 1) == abi.RTD_ERR_NOT_READY   # a matrix, no compact form
        o = abi.default_dij_compact_options()
        o.reserved[3] = 1
        assert L.rtd_field_dose_influence_compact(eng._h, f._h, C.byref(o)) == abi.RTD_ERR_INVALID_ARG
        o = abi.default_dij_compact_options()
        o.release_plain = 2
        assert L.rtd_field_dose_influence_compact(eng._h, f._h, C.byref(o)) == abi.RTD_ERR_INVALID_ARG
        with switches(RTD_DIJC_LANES="8"):
            assert L.rtd_field_dose_influence_compact(eng._h, f._h, None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_dose_influence_compact_info(eng._h, f._h, C.byref(info)) == abi.RTD_ERR_NOT_READY  # (the refusals built nothing)
        r = eng.create_field(b, scn.dims, remote=True)
        assert L.rtd_field_dose_influence_compact(eng._h, r._h, None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_dose_influence_apply_compact(eng._h, r._h, sp, vol, 1) == abi.RTD_ERR_INVALID_ARG
        r.destroy()
        assert L.rtd_field_dose_influence_compact(eng._h, f._h, None) == abi.RTD_OK        # NULL options: the defaults
        assert L.rtd_field_dose_influence_compact_info(eng._h, f._h, None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_dose_influence_compact_device(eng._h, f._h, None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_dose_influence_apply_compact(eng._h, f._h, None, vol, 1) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_dose_influence_apply_compact(eng._h, f._h, sp, None, 1) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_dose_influence_apply_t_compact(eng._h, f._h, None, sp) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_dose_influence_apply_t_compact(eng._h, f._h, vol, None) == abi.RTD_ERR_INVALID_ARG
        assert f.dose_influence_compact_info()["nnz"] == d.nnz
        f.destroy()
        eng.device_free(dVol)
        eng.device_free(dSp)
    finally:
        eng.close()
    eng = engine.Engine(0)
    try:
        eng.set_options(options(0.0, nuclear=1))
        eng.set_luts(luts.synth_luts(nuclear=True))
        eng.set_ct(scn.ct)
        f = eng.create_field(b, scn.dims)
        assert L.rtd_field_dose_influence_compact(eng._h, f._h, None) == abi.RTD_ERR_INVALID_ARG
        assert b"nuclear_corr" in L.rtd_last_error(eng._h)
        f.destroy()
    finally:
        eng.close()


def test_reproducible_on_a_second_engine(dense_case, engine, synth):
    """Test 7: the same inputs on a second engine give the same packed arrays and the same product bits."""
    rig, f, d, a, info, r = dense_case
    scn = hetero_scene(synth, 96, [0.0], spots=5, pitch=4.0, layers=3)
    rng = np.random.default_rng(53)
    w = (100.0 * rng.random(scn.beams[0].spotWeights.shape)).astype(F)
    g = (rng.random(rig.shape) - 0.5).astype(F)
    first = (rig.apply_c(f, w), rig.apply_t_c(f, g))
    other = CompactRig(engine, scn, options(0.0))
    try:
        f2 = other.field(scn.beams[0])
        d2 = f2.dose_influence()
        f2.dose_influence_compact()
        a2, info2 = other.arrays(f2, d2.shape[1])
        assert info2 == info
        for k in a:
            assert (a[k] is None and a2[k] is None) or np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(a2[k]).view(np.uint8)), k
        second = (other.apply_c(f2, w), other.apply_t_c(f2, g))
        assert same_bits(first[0], second[0]) and same_bits(first[1], second[1]) and np.nanmax(first[0]) > 0
    finally:
        other.close()
