"""GPU tests of the products with the resident dose-influence matrix: rtd_field_dose_influence_prepare / _apply / _apply_t / _device.

The host reference is DoseInfluence.matvec / rmatvec (float64) on the copied matrix. The accuracy bound is the standard one for a
float32 sum of n separately rounded float32 products in ANY order: |gpu - ref| <= gamma(n) * sum |a| |x| with
gamma(n) = (n + 1) u / (1 - (n + 1) u), u = 2^-24, n the number of entries of the row / column concerned and sum |a| |x| taken in
float64 on the host. It is derived, not measured; the fixed trees of the kernels do far better, and the tests print the worst
observed ratio. The ray-weight cut-off is 0 throughout (Dij needs it)."""
import ctypes as C

import numpy as np
import pytest

from gpu_support import (FieldRig, box_mask, col_bound, col_of_entry, gamma, hetero_scene, options, radii_above_16, rig_fixture, row_bound,
                         worst_ratio)
from raytracedicom_amd import abi, scenarios

pytestmark = pytest.mark.gpu

rig_of = rig_fixture(FieldRig)


def test_one_hot_products_are_exact(rig_of, synth):
    """apply(e_j, init=1) into NaNs is column j scattered into zeros inside the dose box, NaN outside it; apply_t(e_v) is row v; both
    bit for bit. Doubling the input doubles the output bit for bit."""
    scn = hetero_scene(synth, 96, [0.0], spots=(7, 3), pitch=50.0, layers=2)   # (the outermost spot columns lie 22 mm outside the CT: empty)
    b = scn.beams[0]
    rig = rig_of(scn, options(0.0))
    f = rig.field(b)
    d = f.dose_influence()
    _, info = f.finish()
    box = box_mask(rig, info).reshape(-1)
    assert box.any() and not box.all()
    lens = np.diff(d.indptr)
    L, ny, nx = b.spotWeights.shape
    empty = np.nonzero(lens == 0)[0]
    assert empty.size > 0 and lens.max() > 0
    live = np.nonzero(lens > 0)[0]
    sx = live % nx
    edge, interior = int(live[np.argmin(sx)]), int(live[np.argmin(np.abs(sx - nx // 2))])
    assert edge != interior
    for j in (edge, interior, int(empty[0])):
        e = np.zeros(d.shape[1], dtype=np.float32)
        e[j] = 1.0
        out = rig.apply(f, e.reshape(b.spotWeights.shape)).reshape(-1)
        want = np.full(d.shape[0], np.nan, dtype=np.float32)
        want[box] = 0.0
        rows, vals = d.column(j)
        assert np.all(box[rows])
        want[rows] = vals
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), j
    counts = np.bincount(d.indices, minlength=d.shape[0])
    v_many = int(np.argmax(counts))
    v_one = int(np.nonzero(counts == counts[counts > 0].min())[0][0])
    v_none = int(np.nonzero((counts == 0) & box)[0][0])
    assert counts[v_many] > 1 and counts[v_one] == 1
    col = col_of_entry(d)
    for v in (v_many, v_one, v_none):
        g = np.zeros(d.shape[0], dtype=np.float32)
        g[v] = 1.0
        out = rig.apply_t(f, g.reshape(rig.shape)).reshape(-1)
        want = np.zeros(d.shape[1], dtype=np.float32)
        hit = d.indices == v
        want[col[hit]] = d.data[hit]
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), v
    rng = np.random.default_rng(3)
    w = (1.0 + 99.0 * rng.random(b.spotWeights.shape)).astype(np.float32)      # products within [1e-20, 1e5]: no overflow, no subnormals
    a1, a2 = rig.product(f, w), rig.product(f, 2.0 * w)
    assert a1.max() > 0 and np.array_equal((2.0 * a1).view(np.uint32), a2.view(np.uint32))
    g = (np.where(rng.random(rig.shape) < 0.5, -1.0, 1.0) * (0.25 + 0.25 * rng.random(rig.shape))).astype(np.float32)
    t1, t2 = rig.apply_t(f, g), rig.apply_t(f, 2.0 * g)
    assert np.abs(t1).max() > 0 and np.array_equal((2.0 * t1).view(np.uint32), t2.view(np.uint32))
    mags = np.abs(d.data.astype(np.float64))
    assert mags.min() * 0.25 >= 2.0 ** -126 and mags.max() * 200.0 * d.shape[1] < 2.0 ** 127   # (the range the doubling claim holds for)


def test_against_float64(rig_of, synth):
    """Random w >= 0 and random signed g: every output element within gamma(n) * sum |a| |x| of the float64 host product."""
    scn = hetero_scene(synth, 96, [30.0])
    b = scn.beams[0]
    rig = rig_of(scn, options(0.0))
    f = rig.field(b)
    d = f.dose_influence()
    rng = np.random.default_rng(17)
    w = (100.0 * rng.random(b.spotWeights.shape)).astype(np.float32)
    got = rig.product(f, w).astype(np.float64)
    n, s = row_bound(d, w)
    err = np.abs(got - d.matvec(w))
    ratio_a = worst_ratio(err, gamma(n) * s)
    print("apply: worst |gpu - ref| / bound = %.3g, longest row %d" % (ratio_a, int(n.max())))
    assert np.all(err <= gamma(n) * s), ratio_a
    g = (rng.random(rig.shape) - 0.5).astype(np.float32)
    got_t = rig.apply_t(f, g).reshape(-1).astype(np.float64)
    nt, st = col_bound(d, g)
    err_t = np.abs(got_t - d.rmatvec(g))
    ratio_t = worst_ratio(err_t, gamma(nt) * st)
    print("apply_t: worst |gpu - ref| / bound = %.3g, longest column %d" % (ratio_t, int(nt.max())))
    assert nt.max() > 2048                                            # (columns of several chunks)
    assert np.all(err_t <= gamma(nt) * st), ratio_t


CASES = ["row_sweep", "radii_above_16", "water_uniform", "beam_along_x", "finite_source", "coarse_dose_grid"]


@pytest.mark.parametrize("case", CASES)
def test_apply_is_the_forward(rig_of, synth, case):
    """apply(w) = rtd_field_compute of a field at w, within 1e-5 of the dose maximum plus the float32 summation bound of the row."""
    dims = None
    if case == "row_sweep":
        scn = hetero_scene(synth, 96, [0.0])
    elif case == "radii_above_16":
        scn = radii_above_16(synth)
    elif case == "water_uniform":
        scn = scenarios.water_cube(synth, n=96, n_layers=3, spots=6, pitch=5.0)
    elif case == "beam_along_x":
        scn = hetero_scene(synth, 96, [90.0])
    elif case == "finite_source":
        scn = hetero_scene(synth, 96, [20.0], source_dist=(1800.0, 2100.0))
    else:
        scn = hetero_scene(synth, 96, [30.0])
        t = scn.beams[0].gantryToDoseIdx
        half = scenarios.Float3AffineTransform(0.5 * t.m, 0.5 * t.v - 0.25)     # dose voxel i covers CT voxels 2i, 2i + 1
        scn.beams[0] = scn.beams[0].replace(gantryToDoseIdx=half)
        dims = (48, 48, 48)
    b = scn.beams[0]
    rig = rig_of(scn, options(0.0), dims)
    f = rig.field(b)
    d = f.dose_influence()
    w = (b.spotWeights * (0.5 + np.random.default_rng(11).random(b.spotWeights.shape))).astype(np.float32)
    dw, info, _ = rig.compute(rig.field(b.replace(spotWeights=w)))
    ref = dw.reshape(-1).astype(np.float64)
    got = rig.product(f, w).astype(np.float64)
    n, s = row_bound(d, w)
    scale = float(ref.max())
    assert scale > 0
    err = np.abs(got - ref)
    assert np.all(err <= 1e-5 * scale + gamma(n) * s), float(np.max(err - gamma(n) * s)) / scale
    if case == "radii_above_16":
        assert info["max_radius"] > 16
    if case == "water_uniform":
        assert info["uniform_sigma"] == 1


@pytest.mark.parametrize("case", ["row_sweep", "finite_source"])
def test_apply_t_is_the_gradient(rig_of, synth, case):
    """apply_t(g) = rtd_field_spot_gradient(g) per spot, within 1e-5 * sum |Dij[:, j]| |g| plus the float32 summation bound."""
    scn = hetero_scene(synth, 96, [0.0]) if case == "row_sweep" else hetero_scene(synth, 96, [25.0], source_dist=(1900.0, 2200.0))
    b = scn.beams[0]
    rig = rig_of(scn, options(0.0))
    f = rig.field(b)
    d = f.dose_influence()
    g = (np.random.default_rng(6).random(rig.shape) - 0.3).astype(np.float32)
    grad = rig.grad(f, g).reshape(-1).astype(np.float64)
    got = rig.apply_t(f, g).reshape(-1).astype(np.float64)
    n, s = col_bound(d, g)
    assert (s > 0).sum() > 0
    err = np.abs(got - grad)
    assert np.all(err <= (1e-5 + gamma(n)) * s + 1e-30), float(np.max(err / np.maximum(s, 1e-300)))


def test_semantics(rig_of, synth):
    """init=0 adds s[v] to exactly the voxels that have entries; two fields add up in one volume; a new matrix (threshold 0.1) replaces
    the companion; set_spot_weights changes nothing."""
    ct, _ = scenarios.hetero_phantom(96)
    scn = scenarios.hetero_ct(synth, n=96, spots=5, pitch=8.0, n_layers=3, angles=[0.0, 90.0], ct=ct, seed=5)
    b1, b2 = scn.beams
    rig = rig_of(scn, options(0.0))
    f1, f2 = rig.field(b1), rig.field(b2)
    d1, d2 = f1.dose_influence(), f2.dose_influence()
    rng = np.random.default_rng(23)
    w1 = (100.0 * rng.random(b1.spotWeights.shape)).astype(np.float32)
    w2 = (100.0 * rng.random(b2.spotWeights.shape)).astype(np.float32)
    s1 = rig.product(f1, w1)
    base = (rng.random(rig.shape) - 0.5).astype(np.float32)
    out = rig.apply(f1, w1, into=base, init=False).reshape(-1)
    has = np.bincount(d1.indices, minlength=d1.shape[0]) > 0
    want = base.reshape(-1).copy()
    want[has] = (base.reshape(-1)[has] + s1[has]).astype(np.float32)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert np.all(s1[~has] == 0)
    # two fields into one volume
    both = rig.apply(f1, w1, into=np.zeros(rig.shape, dtype=np.float32), init=False)
    both = rig.apply(f2, w2, into=both, init=False).reshape(-1).astype(np.float64)
    n1, a1 = row_bound(d1, w1)
    n2, a2 = row_bound(d2, w2)
    err = np.abs(both - (d1.matvec(w1) + d2.matvec(w2)))
    assert np.all(err <= gamma(n1 + n2) * (a1 + a2)), worst_ratio(err, gamma(n1 + n2) * (a1 + a2))
    assert np.count_nonzero((n1 > 0) & (n2 > 0)) > 0                  # (the fields do overlap)
    # set_spot_weights leaves the matrix and the companion valid
    g = (rng.random(rig.shape) - 0.5).astype(np.float32)
    t1 = rig.apply_t(f1, g)
    dW = rig.eng.device_alloc(w1.nbytes)
    try:
        rig.eng.to_device(dW, w1)
        f1.set_spot_weights(dW)
        rig.eng.sync()
    finally:
        rig.eng.device_free(dW)
    assert np.array_equal(rig.product(f1, w1).view(np.uint32), s1.view(np.uint32))
    assert np.array_equal(rig.apply_t(f1, g).view(np.uint32), t1.view(np.uint32))
    # a new matrix replaces the companion
    dt = f1.dose_influence(0.1)
    assert 0 < dt.nnz < d1.nnz
    st = rig.product(f1, w1)
    nt, at = row_bound(dt, w1)
    assert np.all(np.abs(st.astype(np.float64) - dt.matvec(w1)) <= gamma(nt) * at)
    assert not np.array_equal(st, s1)
    tt = rig.apply_t(f1, g).reshape(-1).astype(np.float64)
    nc, ac = col_bound(dt, g)
    assert np.all(np.abs(tt - dt.rmatvec(g)) <= gamma(nc) * ac)
    assert f1.dose_influence_device()[3] == dt.nnz


def test_reproducible_and_without_side_effects(rig_of, synth):
    """Each product twice and on a second engine: identical bits, with and without an explicit prepare; the field's BEV dose, a
    following transfer and gradient and the copied CSC arrays are bit-identical to before."""
    scn = hetero_scene(synth, 96, [30.0], layers=2)
    b = scn.beams[0]
    rng = np.random.default_rng(2)
    w = (100.0 * rng.random(b.spotWeights.shape)).astype(np.float32)
    g = (rng.random(scn.ct.shape) - 0.5).astype(np.float32)
    results = []
    for explicit in (True, False):
        rig = rig_of(scn, options(0.0))
        f = rig.field(b)
        dose0, _, _ = rig.compute(f)
        d = f.dose_influence()
        bev0 = f.fetch("bev").copy()
        grad0 = rig.grad(f, g)
        if explicit:
            f.dose_influence_prepare()
            f.dose_influence_prepare()                                # (a no-op)
        a1, t1 = rig.product(f, w), rig.apply_t(f, g)
        a2, t2 = rig.product(f, w), rig.apply_t(f, g)
        assert np.array_equal(a1.view(np.uint32), a2.view(np.uint32)) and np.array_equal(t1.view(np.uint32), t2.view(np.uint32))
        results.append((a1, t1))
        assert np.array_equal(f.fetch("bev"), bev0)
        rig.eng.device_zero(rig.dDose, rig.nb)
        f.transfer(rig.dDose)
        rig.eng.sync()
        dose1 = np.empty(rig.shape, dtype=np.float32)
        rig.eng.to_host(dose1, rig.dDose)
        assert np.array_equal(dose1, dose0)
        assert np.array_equal(rig.grad(f, g), grad0)
        cp, ri, va, nnz = f.dose_influence_device()
        assert nnz == d.nnz and cp and ri and va
        indptr, indices, data = np.empty_like(d.indptr), np.empty_like(d.indices), np.empty_like(d.data)
        rig.eng.to_host(indptr, cp)
        rig.eng.to_host(indices, ri)
        rig.eng.to_host(data, va)
        assert np.array_equal(indptr, d.indptr) and np.array_equal(indices, d.indices) and np.array_equal(data, d.data)
    (a1, t1), (a2, t2) = results
    assert a1.max() > 0 and np.array_equal(a1.view(np.uint32), a2.view(np.uint32)) and np.array_equal(t1.view(np.uint32), t2.view(np.uint32))


def test_products_are_hipgraph_capturable(engine, synth):
    """After prepare, apply + apply_t only launch on the handle's stream: captured into a graph on a caller's stream and replayed, they
    give the bits of the direct calls."""
    import torch
    n = 96
    scn = hetero_scene(synth, n, [25.0], layers=2)
    b = scn.beams[0]
    dev = torch.device("cuda:0")
    eng = engine.Engine(0)
    eng.set_options(options(0.0))
    eng.set_luts(scn.luts)
    eng.set_ct(scn.ct)
    fld = eng.create_field(b, scn.dims)
    fld.dose_influence()
    fld.dose_influence_prepare()
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
        fld.dose_influence_apply(w.data_ptr(), ref_d.data_ptr(), init=True)
        fld.dose_influence_apply_t(gvol.data_ptr(), ref_t.data_ptr())
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            fld.dose_influence_apply(w.data_ptr(), out_d.data_ptr(), init=True)
            fld.dose_influence_apply_t(gvol.data_ptr(), out_t.data_ptr())
        for _ in range(3):
            g.replay()
    torch.cuda.synchronize()
    assert float(torch.nan_to_num(ref_d).max()) > 0 and float(ref_t.abs().max()) > 0
    assert torch.equal(ref_d.view(torch.int32), out_d.view(torch.int32)) and torch.equal(ref_t.view(torch.int32), out_t.view(torch.int32))
    eng.set_stream(None)
    fld.destroy()
    eng.close()


def _descent(matvec, rmatvec, target, w, steps):
    """Projected gradient descent with exact line search on 1/2 |A w - target|^2 (vector updates in float64 on the host; the
    products see float32 inputs). Returns the objective after every step, the start first."""
    def residual(wv):
        r = matvec(wv.astype(np.float32)).astype(np.float64) - target
        return r, 0.5 * float(np.dot(r, r))
    r, fv = residual(w)
    hist = [fv]
    for _ in range(steps):
        step = -rmatvec(r.astype(np.float32)).astype(np.float64)
        step[(w <= 0.0) & (step < 0.0)] = 0.0                        # bound-active spots stay at 0
        ap = matvec(step.astype(np.float32)).astype(np.float64)
        t = -float(np.dot(r, ap)) / float(np.dot(ap, ap))
        neg = step < 0.0
        if neg.any():
            t = min(t, float(np.min(w[neg] / -step[neg])))           # stay feasible
        w = np.maximum(w + t * step, 0.0)
        r, fv = residual(w)
        hist.append(fv)
    return hist


def test_projected_gradient_descent_on_the_device(rig_of, synth):
    """The loop the products exist for: thirty steps with apply / apply_t; the objective never increases and ends at no more than
    half its start. The same steps with the float64 host products run beside it; the difference is reported, not bounded."""
    scn = hetero_scene(synth, 96, [0.0], spots=5, pitch=8.0, layers=3)
    b = scn.beams[0]
    rig = rig_of(scn, options(0.0))
    f = rig.field(b)
    d = f.dose_influence()
    f.dose_influence_prepare()
    shape = b.spotWeights.shape
    w_true = (40.0 + 120.0 * np.random.default_rng(21).random(shape)).astype(np.float32)
    target = d.matvec(w_true)
    w0 = np.full(d.shape[1], float(w_true.mean()))
    gpu = _descent(lambda w: rig.product(f, w.reshape(shape)), lambda g: rig.apply_t(f, g.reshape(rig.shape)).reshape(-1), target, w0.copy(), 30)
    host = _descent(lambda w: d.matvec(w), lambda g: d.rmatvec(g), target, w0.copy(), 30)
    rel = abs(gpu[-1] - host[-1]) / host[-1]
    msg = "objective %.6g -> %.6g on the device, %.6g with the host products: relative difference %.3g" % (gpu[0], gpu[-1], host[-1], rel)
    print(msg)
    assert all(b2 <= a2 for a2, b2 in zip(gpu, gpu[1:])), (msg, gpu)
    assert gpu[-1] <= 0.5 * gpu[0], msg


def test_errors_and_an_empty_matrix(engine, synth):
    """NOT_READY before any matrix; INVALID_ARG for each null pointer and for a remote field; the field stays usable; an all-empty
    matrix gives zeros / no change."""
    L = engine.lib()
    scn = hetero_scene(synth, 64, [0.0], spots=3, layers=1)
    b = scn.beams[0]
    eng = engine.Engine(0)
    try:
        eng.set_options(options(0.0))
        eng.set_luts(synth)
        eng.set_ct(scn.ct)
        f = eng.create_field(b, scn.dims)
        nvox = 64 ** 3
        dVol, dSp = eng.device_alloc(4 * nvox), eng.device_alloc(4 * b.spotWeights.size)
        vol, sp = C.c_void_p(dVol), C.c_void_p(dSp)
        eng.device_zero(dVol, 4 * nvox)
        eng.device_zero(dSp, 4 * b.spotWeights.size)
        p1, p2, p3, nnz = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        assert L.rtd_field_dose_influence_prepare(eng._h, f._h) == abi.RTD_ERR_NOT_READY
        assert L.rtd_field_dose_influence_apply(eng._h, f._h, sp, vol, 1) == abi.RTD_ERR_NOT_READY
        assert L.rtd_field_dose_influence_apply_t(eng._h, f._h, vol, sp) == abi.RTD_ERR_NOT_READY
        assert L.rtd_field_dose_influence_device(eng._h, f._h, C.byref(p1), C.byref(p2), C.byref(p3), C.byref(nnz)) == abi.RTD_ERR_NOT_READY
        d = f.dose_influence()                                        # usable after the refusals
        assert d.nnz > 0
        assert L.rtd_field_dose_influence_apply(eng._h, f._h, None, vol, 1) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_dose_influence_apply(eng._h, f._h, sp, None, 0) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_dose_influence_apply_t(eng._h, f._h, None, sp) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_dose_influence_apply_t(eng._h, f._h, vol, None) == abi.RTD_ERR_INVALID_ARG
        for k in range(4):
            args = [C.byref(p1), C.byref(p2), C.byref(p3), C.byref(nnz)]
            args[k] = None
            assert L.rtd_field_dose_influence_device(eng._h, f._h, *args) == abi.RTD_ERR_INVALID_ARG
        r = eng.create_field(b, scn.dims, remote=True)
        assert L.rtd_field_dose_influence_prepare(eng._h, r._h) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_dose_influence_apply(eng._h, r._h, sp, vol, 1) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_dose_influence_apply_t(eng._h, r._h, vol, sp) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_dose_influence_device(eng._h, r._h, C.byref(p1), C.byref(p2), C.byref(p3), C.byref(nnz)) == abi.RTD_ERR_INVALID_ARG
        r.destroy()
        w = np.ones(b.spotWeights.shape, dtype=np.float32)            # still usable: Dij 1 against the host product
        eng.to_device(dSp, w)
        f.dose_influence_apply(dSp, dVol, init=False)
        out = np.empty(nvox, dtype=np.float32)
        eng.to_host(out, dVol)
        n, s = row_bound(d, w)
        assert out.max() > 0 and np.all(np.abs(out.astype(np.float64) - d.matvec(w)) <= gamma(n) * s)
        f.destroy()
        # every spot 70 mm outside the CT: no ray meets the phantom, the matrix has no entries
        miss = scenarios.make_field(synth, 64, 4.0, (-128.0, -128.0, -106.0), 0.0, 2, 400.0, 1, 3)
        fm = eng.create_field(miss, scn.dims)
        dm = fm.dose_influence()
        assert dm.nnz == 0
        fm.dose_influence_prepare()
        for init in (False, True):
            base = np.random.default_rng(1).random(nvox).astype(np.float32)
            eng.to_device(dVol, base)
            eng.to_device(dSp, np.ones(4, dtype=np.float32))
            fm.dose_influence_apply(dSp, dVol, init=init)
            eng.to_host(out, dVol)
            _, info = fm.finish()
            lo, hi = info["dose_box_min"], info["dose_box_max"]
            want = base.reshape(64, 64, 64).copy()
            if init:                                                  # the dose box (it may be empty) is written with zeros
                want[max(lo[2], 0):hi[2] + 1, max(lo[1], 0):hi[1] + 1, max(lo[0], 0):hi[0] + 1] = 0.0
            assert np.array_equal(out.view(np.uint32), want.reshape(-1).view(np.uint32)), init
        eng.to_device(dSp, np.full(4, np.nan, dtype=np.float32))
        fm.dose_influence_apply_t(dVol, dSp)
        gt = np.empty(4, dtype=np.float32)
        eng.to_host(gt, dSp)
        assert np.array_equal(gt.view(np.uint32), np.zeros(4, dtype=np.uint32))
        assert fm.dose_influence_device()[3] == 0
        fm.destroy()
        eng.device_free(dVol)
        eng.device_free(dSp)
    finally:
        eng.close()
