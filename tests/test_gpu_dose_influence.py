"""GPU tests of the dose-influence matrix (rtd_field_dose_influence / _copy) and of rtd_field_set_spot_weights.

Dij is checked against the engine's two other paths: Dij w = D(w) (the forward) and Dij^T g = rtd_field_spot_gradient(g) (the
transposed path). Dot products and sums are float64 on the host; tolerances are relative to sum |a| |b| of the pair compared. The
ray-weight cut-off is 0 unless stated otherwise (Dij needs it)."""
import ctypes as C

import numpy as np
import pytest

from gpu_support import FieldRig, hetero_scene, options, radii_above_16, rig_fixture
from raytracedicom_amd import abi, scenarios

pytestmark = pytest.mark.gpu

rig_of = rig_fixture(FieldRig)


def _check_csc(d):
    assert d.indptr[0] == 0 and np.all(np.diff(d.indptr) >= 0) and d.indptr[-1] == d.indices.size == d.data.size
    for j in range(d.shape[1]):
        rows, vals = d.column(j)
        assert np.all(np.diff(rows) > 0), j                           # strictly ascending: no voxel twice
        assert np.all(vals != 0)
    assert d.indices.size == 0 or (d.indices.min() >= 0 and d.indices.max() < d.shape[0])


def _linearity(rig, beam, seed, tol=1e-5):
    f = rig.field(beam)
    d = f.dose_influence()
    _check_csc(d)
    w = (beam.spotWeights * (0.5 + np.random.default_rng(seed).random(beam.spotWeights.shape))).astype(np.float32)
    dw, info, _ = rig.compute(rig.field(beam.replace(spotWeights=w)))
    a = d.matvec(w)
    b = dw.reshape(-1).astype(np.float64)
    scale = float(np.abs(b).max())
    assert scale > 0
    assert float(np.abs(a - b).max()) <= tol * scale, (float(np.abs(a - b).max()), scale)
    return f, d, info


def test_columns_are_single_spot_doses(rig_of, synth):
    """Column j at threshold 0 is the dose of a fresh field with one-hot weights e_j: edge spots and interior spots, at least two of
    them in one batch, within 1e-6 of the column maximum (the other spots of a batch add exact zeros)."""
    scn = hetero_scene(synth, 96, [20.0], spots=(4, 3), pitch=50.0, layers=2)    # (spots far apart: their grown footprints can share a batch)
    b = scn.beams[0]
    rig = rig_of(scn, options(0.0))
    f = rig.field(b)
    d = f.dose_influence()
    batch = f.fetch("dij_batch")
    L, ny, nx = b.spotWeights.shape
    picks = [(0, 0, 0), (0, 0, nx - 1), (1, ny - 1, 0), (1, ny - 1, nx - 1), (0, 1, 1), (1, 1, 2)]
    shared = [int(j) for j in np.nonzero(batch == batch[0])[0][:2]]
    assert len(shared) == 2, batch                                    # two spots of one batch
    picks += [np.unravel_index(j, (L, ny, nx)) for j in shared]
    js = [(l * ny + y) * nx + x for (l, y, x) in picks]
    assert min(int(batch[j]) for j in js) >= 0
    for j, p in zip(js, picks):
        e = np.zeros(b.spotWeights.shape, dtype=np.float32)
        e[p] = 1.0
        dense = rig.dose(b.replace(spotWeights=e)).reshape(-1)
        col = np.zeros(d.shape[0], dtype=np.float32)
        rows, vals = d.column(j)
        col[rows] = vals
        assert dense.max() > 0, p
        # (not bit for bit: the superposition's summation grouping follows the extents of the rays that carry dose, which differ
        #  between a batch and a one-spot field)
        assert float(np.abs(col - dense).max()) <= 1e-6 * float(dense.max()), (p, float(np.abs(col - dense).max()), float(dense.max()))
        assert np.array_equal(col != 0, dense != 0) or np.count_nonzero((col != 0) != (dense != 0)) <= 1e-3 * np.count_nonzero(dense), p


CASES = ["row_sweep", "radii_above_16", "water_uniform", "beam_along_x", "finite_source", "coarse_dose_grid"]


@pytest.mark.parametrize("case", CASES)
def test_linearity(rig_of, synth, case):
    """Dij w = D(w) for random w, on every superposition / transfer path and on a half-resolution dose grid."""
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
        # dose voxel i covers CT voxels 2i, 2i + 1: index = 0.5 * ct index - 0.25
        half = scenarios.Float3AffineTransform(0.5 * t.m, 0.5 * t.v - 0.25)
        scn.beams[0] = scn.beams[0].replace(gantryToDoseIdx=half)
        dims = (48, 48, 48)
    rig = rig_of(scn, options(0.0), dims)
    _, _, info = _linearity(rig, scn.beams[0], seed=11)
    if case == "radii_above_16":
        assert info["max_radius"] > 16
    if case == "water_uniform":
        assert info["uniform_sigma"] == 1


@pytest.mark.parametrize("case", ["row_sweep", "finite_source"])
def test_transpose_is_the_gradient(rig_of, synth, case):
    """Dij^T g = rtd_field_spot_gradient(g) per spot, relative to sum |Dij[:, j]| |g|."""
    scn = hetero_scene(synth, 96, [0.0]) if case == "row_sweep" else hetero_scene(synth, 96, [25.0], source_dist=(1900.0, 2200.0))
    b = scn.beams[0]
    rig = rig_of(scn, options(0.0))
    f = rig.field(b)
    d = f.dose_influence()
    g = (np.random.default_rng(6).random(rig.shape) - 0.3).astype(np.float32)
    grad = rig.grad(f, g).reshape(-1).astype(np.float64)
    a = d.rmatvec(g)
    scale = np.zeros(d.shape[1])
    np.add.at(scale, np.repeat(np.arange(d.shape[1]), np.diff(d.indptr)), np.abs(d.data.astype(np.float64) * g.reshape(-1)[d.indices]))
    live = scale > 0
    assert live.sum() > 0
    assert np.all(np.abs(a - grad) <= 1e-5 * scale + 1e-30), float(np.max(np.abs(a - grad) - 1e-5 * scale))


def test_against_the_cpu_oracle(rig_of, synth, orc):
    """C1 (water 128^3, one layer): Dij w = the oracle's dose at cut-off 0."""
    scn = scenarios.water_cube(synth, n=128, n_layers=1)
    opt = options(0.0)
    rig = rig_of(scn, opt)
    d = rig.field(scn.beams[0]).dose_influence()
    ref = orc.compute(scn, options=opt).reshape(-1).astype(np.float64)
    a = d.matvec(scn.beams[0].spotWeights)
    assert float(np.abs(a - ref).max()) <= 1e-4 * float(ref.max())


def test_dense_spots_force_many_batches(rig_of, synth):
    """A 2 mm spot pitch: the grown footprints overlap, so the spots need many batches; every column is a proper set of voxels, and
    the columns sum to the forward at w = 1."""
    scn = hetero_scene(synth, 96, [10.0], spots=9, pitch=2.0, layers=2)
    b = scn.beams[0]
    rig = rig_of(scn, options(0.0))
    f = rig.field(b)
    d = f.dose_influence()
    batch = f.fetch("dij_batch")
    assert batch.max() + 1 > 1
    _check_csc(d)
    ones = np.ones(b.spotWeights.shape, dtype=np.float32)
    d1 = rig.dose(b.replace(spotWeights=ones)).reshape(-1).astype(np.float64)
    a = d.matvec(ones)
    assert float(np.abs(a - d1).max()) <= 1e-5 * float(d1.max())


def test_threshold(rig_of, synth):
    """Kept entries are >= t * column max; what t drops from the t = 0 matrix is below it; nnz is monotone in t."""
    scn = hetero_scene(synth, 96, [0.0])
    rig = rig_of(scn, options(0.0))
    f = rig.field(scn.beams[0])
    d0 = f.dose_influence(0.0)
    last = d0.nnz
    for t in (0.001, 0.01, 0.1, 0.5):
        dt = f.dose_influence(t)
        _check_csc(dt)
        assert dt.nnz <= last
        last = dt.nnz
        for j in range(d0.shape[1]):
            r0, v0 = d0.column(j)
            if v0.size == 0:
                continue
            thr = np.float32(t) * v0.max()
            rt, vt = dt.column(j)
            assert np.all(vt >= thr)
            assert np.array_equal(rt, r0[v0 >= thr]) and np.array_equal(vt, v0[v0 >= thr])
    assert last < d0.nnz


def test_reproducible_and_without_side_effects(rig_of, synth):
    """Two calls give identical arrays; the field's BEV dose, a following transfer and gradient are bit-identical to before."""
    scn = hetero_scene(synth, 96, [30.0], layers=2)
    b = scn.beams[0]
    rig = rig_of(scn, options(0.0))
    f = rig.field(b)
    dose0, _, _ = rig.compute(f)
    bev0 = f.fetch("bev").copy()
    g = (np.random.default_rng(2).random(rig.shape) - 0.5).astype(np.float32)
    grad0 = rig.grad(f, g)
    d1 = f.dose_influence(0.0)
    d2 = f.dose_influence(0.0)
    for a, c in [(d1.indptr, d2.indptr), (d1.indices, d2.indices), (d1.data, d2.data)]:
        assert np.array_equal(a, c)
    assert np.array_equal(f.fetch("bev"), bev0)
    rig.eng.device_zero(rig.dDose, rig.nb)
    f.transfer(rig.dDose)
    rig.eng.sync()
    dose1 = np.empty(rig.shape, dtype=np.float32)
    rig.eng.to_host(dose1, rig.dDose)
    assert np.array_equal(dose1, dose0)
    assert np.array_equal(rig.grad(f, g), grad0)


def test_without_a_prior_compute(rig_of, synth):
    """A field never computed: the call runs the forward itself, and the field then transfers its own dose."""
    scn = hetero_scene(synth, 96, [0.0], layers=2)
    b = scn.beams[0]
    rig = rig_of(scn, options(0.0))
    ref = rig.dose(b)
    f = rig.field(b)
    d = f.dose_influence()
    assert d.nnz > 0
    rig.eng.device_zero(rig.dDose, rig.nb)
    f.transfer(rig.dDose)
    rig.eng.sync()
    out = np.empty(rig.shape, dtype=np.float32)
    rig.eng.to_host(out, rig.dDose)
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("cutoff", [0.0, 1.0])
def test_set_spot_weights(rig_of, synth, cutoff):
    """After set_spot_weights a compute equals a fresh field with those weights bit for bit, and so does its gradient. Under cut-off 1
    the new weights change the live set (spots below the cut-off): the hints of the last compute must not survive."""
    scn = hetero_scene(synth, 96, [15.0], layers=2)
    b = scn.beams[0]
    rig = rig_of(scn, options(cutoff))
    f = rig.field(b)
    rig.compute(f)
    rig.compute(f)                                                    # (a finished compute: the field holds its hints)
    w = (b.spotWeights * np.random.default_rng(9).random(b.spotWeights.shape)).astype(np.float32)
    w[:, :2, :] = 0.5                                                 # below the cut-off of 1: those rays die
    dW = rig.eng.device_alloc(w.nbytes)
    try:
        rig.eng.to_device(dW, w)
        f.set_spot_weights(dW)
    finally:
        rig.eng.sync()
        rig.eng.device_free(dW)
    got, _, _ = rig.compute(f)
    b2 = b.replace(spotWeights=w)
    f2 = rig.field(b2)
    ref, _, _ = rig.compute(f2)
    assert np.array_equal(got, ref)
    assert not np.array_equal(got, rig.dose(b))
    g = (np.random.default_rng(4).random(rig.shape) - 0.3).astype(np.float32)
    assert np.array_equal(rig.grad(f, g), rig.grad(f2, g))


def test_engine_form(engine, synth):
    """Engine.dose_influence: one DoseInfluence per beam, each equal to the field call."""
    scn = hetero_scene(synth, 64, [0.0], spots=3, layers=1)
    eng = engine.Engine(0)
    try:
        eng.set_options(options(0.0))
        eng.set_luts(synth)
        eng.set_ct(scn.ct)
        ds = eng.dose_influence(scn.beams + scn.beams, scn.dims)
        assert len(ds) == 2 and ds[0].nnz > 0
        assert np.array_equal(ds[0].indptr, ds[1].indptr) and np.array_equal(ds[0].data, ds[1].data)
        assert ds[0].shape == (64 ** 3, 9)
    finally:
        eng.close()


def test_errors(engine, synth):
    """Each refusal returns its status and leaves the field usable: cut-off != 0, nuclear_corr, a remote field, null pointers, a
    threshold outside [0, 1); copy before any result is NOT_READY."""
    L = engine.lib()
    scn = hetero_scene(synth, 64, [0.0], spots=3, layers=1)
    b = scn.beams[0]
    dims = scn.dims
    eng = engine.Engine(0)
    try:
        eng.set_luts(synth)
        eng.set_ct(scn.ct)
        eng.set_options(options(1.0))
        f1 = eng.create_field(b, dims)
        with pytest.raises(engine.RtdError) as e:
            f1.dose_influence()
        assert e.value.status == abi.RTD_ERR_INVALID_ARG and "ray_weight_cutoff" in str(e.value)
        f1.destroy()
        eng.set_options(options(0.0))
        f = eng.create_field(b, dims)
        nnz = C.c_size_t(0)
        i64 = np.zeros(16, dtype=np.int64)
        assert L.rtd_field_dose_influence_copy(eng._h, f._h, i64.ctypes.data_as(C.c_void_p), None, None) == abi.RTD_ERR_NOT_READY
        for t in (-0.1, 1.0, float("nan")):
            assert L.rtd_field_dose_influence(eng._h, f._h, C.c_float(t), C.byref(nnz)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_dose_influence(eng._h, f._h, C.c_float(0.0), None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_set_spot_weights(eng._h, f._h, None) == abi.RTD_ERR_INVALID_ARG
        r = eng.create_field(b, dims, remote=True)
        assert L.rtd_field_dose_influence(eng._h, r._h, C.c_float(0.0), C.byref(nnz)) == abi.RTD_ERR_INVALID_ARG
        dW = eng.device_alloc(64)
        assert L.rtd_field_set_spot_weights(eng._h, r._h, C.c_void_p(dW)) == abi.RTD_ERR_INVALID_ARG
        eng.device_free(dW)
        r.destroy()
        d = f.dose_influence()                                        # the field is still usable
        assert d.nnz > 0
        assert L.rtd_field_dose_influence_copy(eng._h, f._h, None, None, None) == abi.RTD_ERR_INVALID_ARG
        f.destroy()
    finally:
        eng.close()
    from raytracedicom_amd import luts
    nl = luts.synth_luts(nuclear=True)
    scn = scenarios.water_cube(nl, n=64, n_layers=1, spots=5, pitch=6.0)
    o = options(0.0)
    o.nuclear_corr = 1                                                # RTD_NUC_SOUKUP
    eng = engine.Engine(0)
    try:
        eng.set_options(o)
        eng.set_luts(nl)
        eng.set_ct(scn.ct)
        f = eng.create_field(scn.beams[0], scn.dims)
        with pytest.raises(engine.RtdError) as e:
            f.dose_influence()
        assert e.value.status == abi.RTD_ERR_INVALID_ARG
        f.destroy()
    finally:
        eng.close()
