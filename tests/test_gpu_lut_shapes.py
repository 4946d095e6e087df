"""GPU tests on look-up tables of other shapes than the default one (tests/lut_shapes.py): the builds of k_fill that read the layer's
cumulative-IDD rows from global memory, the tracer's fallbacks to the plain sampling kernel, tables of unequal lengths and non-unit
scale factors, and the paths that read the same tables by their sizes (spot gradient, dose-influence matrix, LET).

Which build a launch chose is read from rtd_field_fetch "launch_builds" ([0] tracer kernel 0 plain / 1 along-beam / 2 diagonal,
[1] the fill's rows staged in LDS, [2] the fill's mode 0 walked / 1 sigma replayed, dose walked / 2 both replayed, [3] NUCLEAR_CORR)
and asserted per case; no test works it out from the table sizes. The checks and tolerances are those of the files the default
shape is tested in: gpu_support.compare_field / compare_nuclear_field (tests/test_gpu_parity.py), stage_identities / end_to_end
(test_gpu_gradient.py), dead_work_support (test_gpu_fill_dead_skip.py), test_gpu_dose_influence.py, and the float32 restatements of
let_reference.py (test_gpu_let.py).

The scene is lut_shapes.scene: the 64^3 heterogeneous phantom, 5 x 5 spots, 3 layers, 512 steps, 64 x 56 rays."""
import numpy as np
import pytest

import let_reference as R
import lut_shapes as LS
from dead_work_support import compute, reference, same, set_weights
from gpu_support import (FieldRig, bits, box_mask, compare_field, compare_nuclear_field, end_to_end, hetero_scene, options, rig_fixture,
                         stage_identities, switches)
from raytracedicom_amd import abi, luts, scenarios

pytestmark = pytest.mark.gpu

rig_of = rig_fixture(FieldRig)

F = np.float32
PLAIN, ALONG, DIAGONAL = 0, 1, 2


def builds(f):
    return [int(v) for v in f.fetch("launch_builds")]


def worst_rel(dose, ref):
    """The largest relative difference above 1e-3 of the reference's maximum (what rel_close bounds by 1e-4)."""
    big = ref > 1e-3 * ref.max()
    return float((np.abs(dose.astype(np.float64) - ref)[big] / ref[big]).max())


# ---- forward parity: the fill's rows in LDS and in global memory -----------------------------------------------------------------

@pytest.mark.parametrize("name,rows_in_lds", [("rows_last_in_lds", 1), ("rows_first_global", 0), ("rows_global", 0), ("rows_2049", 1)])
def test_fill_rows_against_the_oracle(orc, engine, name, rows_in_lds):
    """Every intermediate of a walked field against the oracle; rows_first_global and rows_global through k_fill<false, false>."""
    es = LS.table(name)
    scn = LS.scene(es)
    got = []
    dose, ref, _, info = compare_field(orc, engine, scn, scn.beams[0], inspect=lambda f: got.append(builds(f)))
    print("%s: %d B of rows and step table, launch_builds %s, ray_dims %s, max_radius %d, worst relative difference %.3g" % (
        name, LS.fill_lds_bytes(es), got[0], info["ray_dims"], info["max_radius"], worst_rel(dose, ref)))
    assert got[0][1:] == [rows_in_lds, 0, 0], got


def test_nuclear_fill_with_rows_in_global_memory(orc, engine):
    """k_fill<false, true> with the halo. The halo reaches the dose only from a beam that starts inside the patient (entry step 0),
    so this case runs on the 64^3 water cube of tests/test_gpu_nuclear.py, not on the module's scene."""
    es = LS.table("rows_global_nuclear")
    scn = scenarios.water_cube(es, n=64, n_layers=3, spots=7, pitch=6.0)
    opt = abi.default_options()
    opt.nuclear_corr = abi.RTD_NUC_SOUKUP
    got = []
    dose, ref, info = compare_nuclear_field(orc, engine, scn, opt, inspect=lambda f: got.append(builds(f)))
    base = np.zeros_like(scn.ct)
    orc.run_field(scn, scn.beams[0], base, keep_layers=False).close()
    print("rows_global, NUCLEAR_CORR: launch_builds %s, entry step %d, worst relative difference %.3g, dose sum %.6g against %.6g without" % (
        got[0], info["beam_first_inside"], worst_rel(dose, ref), float(ref.sum()), float(base.sum())))
    assert got[0][1:] == [0, 0, 1], got
    assert info["beam_first_inside"] == 0 and 0.9 * base.sum() < ref.sum() < base.sum()


# ---- the tracer: LDS limits of the along-beam and diagonal kernels, unequal tables, scale factors -------------------------------

TRACER = [("hu_6048", 0, PLAIN), ("hu_6048", 1, ALONG), ("hu_6048", 2, DIAGONAL),
          ("hu_6049", 0, PLAIN), ("hu_6049", 1, PLAIN), ("hu_6049", 2, DIAGONAL),        # mode 1: the tables leave the tile no room
          ("hu_12672", 0, PLAIN), ("hu_12672", 1, PLAIN), ("hu_12672", 2, DIAGONAL),
          ("hu_12673", 0, PLAIN), ("hu_12673", 1, PLAIN), ("hu_12673", 2, PLAIN),        # mode 2 likewise
          ("mixed", 0, PLAIN), ("mixed", 1, ALONG), ("mixed", 2, DIAGONAL)]


@pytest.mark.parametrize("name,mode,kernel", TRACER)
def test_tracer_kernels_against_the_oracle(orc, engine, name, mode, kernel):
    """The field at 15 degrees under RTD_TRACE_MODE 0, 1 and 2 (each kernel is valid at every angle; the ray grid is 64 wide, a
    multiple of the diagonal kernel's 32): tracer outputs bit for bit, everything behind them at the parity tolerances."""
    es = LS.table(name)
    scn = LS.scene(es)
    got = []
    with switches(RTD_TRACE_MODE=str(mode), RTD_TRACE_DIAG_B=None):
        dose, ref, _, info = compare_field(orc, engine, scn, scn.beams[0], inspect=lambda f: got.append(builds(f)))
    print("%s, RTD_TRACE_MODE=%d: %d staged entries (%d B), launch_builds %s, worst relative difference %.3g" % (
        name, mode, LS.trace_lut_entries(es), 4 * LS.trace_lut_entries(es), got[0], worst_rel(dose, ref)))
    assert info["ray_dims"][0] % 32 == 0
    assert got[0][0] == kernel and got[0][1:] == [1, 0, 0], got


# ---- replay: the sigma record and the dose record over rows in global memory ------------------------------------------------------

CUTOFF = 1.0


def _left_dead(w):
    """The three left spot columns below the cut-off (tests/test_gpu_fill_dead_skip.py)."""
    w = w.copy()
    w[:, :, :3] = 0.0
    return w


@pytest.mark.parametrize("name,env,rows_in_lds,modes", [
    ("rows_global", {}, 0, (0, 2, 2)), ("rows_first_global", {}, 0, (0, 2, 2)),
    ("rows_global", {"RTD_NO_DOSE_REPLAY": "1"}, 0, (0, 1, 1)), ("rows_first_global", {"RTD_NO_DOSE_REPLAY": "1"}, 0, (0, 1, 1)),
    ("rows_last_in_lds", {"RTD_NO_DOSE_REPLAY": "1"}, 1, (0, 1, 1))])
def test_replayed_fills_are_the_walked_ones(rig_of, name, env, rows_in_lds, modes):
    """One field computed three times (walked, recorded and replayed, replayed), then the weight sequence of
    test_gpu_fill_dead_skip.py (spot columns below the cut-off and back, all zero and back): every compute bit-equal, over everything
    a compute writes, to the first compute of a fresh field with the same weights that traces and walks. Under RTD_NO_DOSE_REPLAY the
    field keeps no dose record: sigma replayed, dose walked from the rows, k_fill<false, false, kFillReplay> for rows in global
    memory."""
    scn = LS.scene(LS.table(name))
    beam = scn.beams[0]
    rig = rig_of(scn, options(CUTOFF))
    full = beam.spotWeights.astype(np.float32)
    weights = {"part": _left_dead(full), "full": full, "none": np.zeros_like(full)}
    refs = {k: reference(rig, beam.replace(spotWeights=w)) for k, w in weights.items()}
    f = rig.field(beam.replace(spotWeights=weights["part"]), **env)
    seen = []
    for _ in range(3):
        same(compute(rig, f), refs["part"])
        seen.append(builds(f))
    for key in ("full", "part", "part", "full", "part", "none", "none", "part", "full"):
        set_weights(rig, f, weights[key])
        out = compute(rig, f)
        seen.append(builds(f))
        assert out["sigma_reused"] == 2 and out["trace_reused"] == 1
        same(out, refs[key])
    print("%s %s: launch_builds of the computes %s" % (name, env, seen))
    assert refs["full"]["dose"].max() > 0 and refs["none"]["dose"].max() == 0 and not np.array_equal(refs["full"]["dose"], refs["part"]["dose"])
    assert tuple(b[2] for b in seen[:3]) == modes and all(b[2] == modes[2] for b in seen[3:]), seen
    # (a replayed dose step looks nothing up: with the dose record no rows are staged wherever they would fit)
    assert seen[0][1] == rows_in_lds and all(b[1] == (rows_in_lds if modes[2] == 1 else 0) for b in seen[1:]), seen
    assert all(b[3] == 0 for b in seen), seen


# ---- the spot gradient ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,rows_in_lds", [("rows_global", 0), ("mixed", 1)])
def test_gradient_identities(rig_of, name, rows_in_lds):
    """The stage identities and the end-to-end identity of tests/test_gpu_gradient.py at 0 degrees with a finite source."""
    scn = LS.scene(LS.table(name), angle=0.0, source_dist=(2000.0, 2300.0))
    rng = np.random.default_rng(1)
    b = scn.beams[0].replace(spotWeights=20.0 + 80.0 * rng.random(scn.beams[0].spotWeights.shape))
    g = rng.random(scn.ct.shape).astype(np.float32)
    rig = rig_of(scn, options(0.0))
    f, _, grad, _ = stage_identities(rig, b, g, 1e-5)
    got = builds(f)
    assert np.abs(grad).max() > 0
    g2 = (np.random.default_rng(3).random(scn.ct.shape) - 0.3).astype(np.float32)
    info = end_to_end(rig, scn.beams[0], g2, seed=4)
    got2 = builds(rig.fields[-1])
    print("%s: launch_builds %s and %s, max_radius %d" % (name, got, got2, info["max_radius"]))
    assert got[1:] == [rows_in_lds, 0, 0] and got2[1:] == [rows_in_lds, 0, 0], (got, got2)


# ---- the dose-influence matrix ----------------------------------------------------------------------------------------------------

def test_dose_influence_columns_with_rows_in_global_memory(rig_of):
    """tests/test_gpu_dose_influence.py::test_columns_are_single_spot_doses on rows_global: column j at threshold 0 is the dose of a
    fresh field with one-hot weights. The spots are 50 mm apart (4 x 3 of them, 2 layers, on the 64^3 phantom), not the module's
    scene: their grown footprints have to be far enough apart to share a batch."""
    scn = hetero_scene(LS.table("rows_global"), 64, [20.0], spots=(4, 3), pitch=50.0, layers=2)
    b = scn.beams[0]
    rig = rig_of(scn, options(0.0))
    f = rig.field(b)
    d = f.dose_influence()
    got = builds(f)
    batch = f.fetch("dij_batch")
    L, ny, nx = b.spotWeights.shape
    picks = [(0, 0, 0), (0, 0, nx - 1), (1, ny - 1, 0), (1, ny - 1, nx - 1), (0, 1, 1), (1, 1, 2)]
    shared = [int(j) for j in np.nonzero(batch == batch[0])[0][:2]]
    assert len(shared) == 2, batch                                    # two spots of one batch
    picks += [np.unravel_index(j, (L, ny, nx)) for j in shared]
    js = [(l * ny + y) * nx + x for (l, y, x) in picks]
    assert min(int(batch[j]) for j in js) >= 0
    worst = 0.0
    for j, p in zip(js, picks):
        e = np.zeros(b.spotWeights.shape, dtype=np.float32)
        e[p] = 1.0
        dense = rig.dose(b.replace(spotWeights=e)).reshape(-1)
        col = np.zeros(d.shape[0], dtype=np.float32)
        rows, vals = d.column(j)
        col[rows] = vals
        assert dense.max() > 0, p
        worst = max(worst, float(np.abs(col - dense).max()) / float(dense.max()))
        assert float(np.abs(col - dense).max()) <= 1e-6 * float(dense.max()), (p, float(np.abs(col - dense).max()), float(dense.max()))
        assert np.array_equal(col != 0, dense != 0) or np.count_nonzero((col != 0) != (dense != 0)) <= 1e-3 * np.count_nonzero(dense), p
    print("rows_global, Dij columns: launch_builds after the matrix %s, %d batches, worst |column - dose| / max %.3g" % (got, int(batch.max()) + 1, worst))
    assert got[1] == 0 and got[3] == 0, got


def test_dose_influence_linearity_and_the_computes_around_it(rig_of):
    """Dij w = D(w) for a random w (test_gpu_dose_influence.py::_linearity), then the field's own computes around the matrix equal
    their reference bit for bit (test_gpu_fill_dead_skip.py::test_dose_influence_between_computes): the batches go through the
    replaying fill with weights of their own."""
    scn = LS.scene(LS.table("rows_global"))
    b = scn.beams[0]
    rig = rig_of(scn, options(0.0))
    f = rig.field(b)
    ref = reference(rig, b)
    seen = []
    for _ in range(3):
        same(compute(rig, f), ref)
        seen.append(builds(f))
    d = f.dose_influence()
    seen.append(builds(f))
    assert d.indptr[0] == 0 and np.all(np.diff(d.indptr) >= 0) and d.indptr[-1] == d.indices.size == d.data.size and d.nnz > 0
    for j in range(d.shape[1]):
        rows, vals = d.column(j)
        assert np.all(np.diff(rows) > 0) and np.all(vals != 0), j
    w = (b.spotWeights * (0.5 + np.random.default_rng(11).random(b.spotWeights.shape))).astype(np.float32)
    dw = rig.dose(b.replace(spotWeights=w)).reshape(-1).astype(np.float64)
    a = d.matvec(w)
    scale = float(np.abs(dw).max())
    assert scale > 0 and float(np.abs(a - dw).max()) <= 1e-5 * scale, (float(np.abs(a - dw).max()), scale)
    for _ in range(2):
        same(compute(rig, f), ref)
        seen.append(builds(f))
    part = _left_dead(b.spotWeights.astype(np.float32))
    set_weights(rig, f, part)
    same(compute(rig, f), reference(rig, b.replace(spotWeights=part)))
    seen.append(builds(f))
    print("rows_global, Dij: |Dij w - D(w)| / max %.3g; launch_builds of three computes, the matrix, three computes: %s" % (
        float(np.abs(a - dw).max()) / scale, seen))
    assert seen[0][1:] == [0, 0, 0] and all(s[1] == 0 and s[3] == 0 for s in seen), seen
    assert all(s[2] in (1, 2) for s in seen[1:]), seen


# ---- LET --------------------------------------------------------------------------------------------------------------------------

SENTINEL = F(-12345.5)


def test_let_depth_and_matrix_values_are_the_restatement(rig_of):
    """tests/test_gpu_let.py::test_water_depth_is_the_restatement and ::test_matrix_values_are_the_restatement on rows_global with
    luts.synth_let of that table ([40][8192]): the water depth bit for bit inside the dose box and the sentinel outside, the CSC LET
    values float32(D * L) of the restatement bit for bit, a one-hot w through let_apply reproducing its column."""
    es = LS.table("rows_global")
    scn = LS.scene(es)
    beam = scn.beams[0]
    rig = rig_of(scn, options(0.0))
    eng, f = rig.eng, rig.field(beam)
    table = luts.synth_let(es)
    assert table.shape == (es.nEnergies, es.nEnergySamples) == (40, 8192)
    eng.set_let_table(table)
    d = f.dose_influence()
    f.let_influence()
    _, info = f.finish()
    got_builds = builds(f)
    W, H, L = info["ray_dims"]
    S = beam.tracerSteps
    wepl = f.fetch("wepl").reshape(S, H, W).copy()
    plan = f.fetch("layer_plan").reshape(L, 8).copy()
    tr = R.Transfer(beam, info)
    nx, ny, nz = rig.dims
    # the water depth
    eng.to_device(rig.dDose, np.full(rig.shape, SENTINEL, dtype=F))
    f.water_depth(rig.dDose)
    got = np.empty(rig.shape, dtype=F)
    eng.to_host(got, rig.dDose)
    lo, hi = info["dose_box_min"], info["dose_box_max"]
    box = box_mask(rig, info)
    assert box.any() and not box.all()
    want = np.full(rig.shape, SENTINEL, dtype=F)
    want[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = R.box_depth(tr, wepl, lo, hi)
    diff = bits(got) != bits(want)
    assert not diff.any(), "%d of %d voxels differ (%d of them inside the box); first: got %r, want %r" % (
        int(diff.sum()), diff.size, int((diff & box).sum()), got[diff][:1], want[diff][:1])
    assert np.isfinite(got[box]).all() and got[box].min() >= 0 and got[box].max() > 10.0
    # the matrix values
    va, nnz = f.let_influence_device()
    assert nnz == d.nnz and va
    vals = np.empty(nnz, dtype=F)
    eng.to_host(vals, va)
    rows = np.unique(d.indices)
    depth = np.full(d.shape[0], np.nan, dtype=F)
    depth[rows] = R.water_depth(tr, wepl, rows % nx, (rows // nx) % ny, rows // (nx * ny))
    per = int(np.prod(beam.spotWeights.shape[1:]))
    restated = R.let_values(d.data, d.indices, d.indptr, per, plan, table, depth)
    diff = bits(vals) != bits(restated)
    assert not diff.any(), "%d of %d entries differ; first: got %r, want %r (D %r)" % (int(diff.sum()), diff.size, vals[diff][:1], restated[diff][:1], d.data[diff][:1])
    assert vals.max() > 0 and not np.array_equal(vals, d.data)
    flat_box = box.reshape(-1)
    lens = np.diff(d.indptr)
    for layer in range(d.shape[1] // per):
        j = layer * per + int(np.argmax(lens[layer * per:(layer + 1) * per]))   # the layer's longest column
        assert lens[j] > 0
        e = np.zeros(d.shape[1], dtype=F)
        e[j] = 1.0
        dW = eng.device_alloc(e.nbytes)
        try:
            eng.to_device(dW, e)
            eng.to_device(rig.dDose, np.full(rig.shape, np.nan, dtype=F))
            f.let_apply(dW, rig.dDose, init=True)
            out = np.empty(rig.shape, dtype=F)
            eng.to_host(out, rig.dDose)
        finally:
            eng.device_free(dW)
        expect = np.full(d.shape[0], np.nan, dtype=F)
        expect[flat_box] = 0.0
        col_rows = d.indices[d.indptr[j]:d.indptr[j + 1]]
        assert np.all(flat_box[col_rows])
        expect[col_rows] = restated[d.indptr[j]:d.indptr[j + 1]]
        assert np.array_equal(bits(out.reshape(-1)), bits(expect)), j
    print("rows_global, LET: launch_builds %s, %d matrix entries, depth up to %.4g mm, LET values up to %.4g" % (
        got_builds, nnz, float(got[box].max()), float(vals.max())))
    assert got_builds[1] == 0 and got_builds[3] == 0, got_builds


# ---- tables beyond a block's LDS -------------------------------------------------------------------------------------------------

def test_tables_beyond_a_blocks_lds_are_refused(engine, synth):
    """The two staged HU tables of a 16-bit CT range (2 x 65 536 entries, 512 KiB) exceed the 160 KiB of LDS a block can have: no
    tracer kernel could be launched for them. rtd_set_luts refuses them with a message that names the limit, at 40 961 entries as
    well, and takes 40 960; no launch is involved in any of these calls. The handle keeps its tables and stays usable."""
    scn = scenarios.water_cube(synth, n=32, n_layers=1, spots=3)
    small = luts.synth_luts(n_energies=8, n_samples=64, n_hu=65536)

    def tables(n_density, n_sp):
        return luts.EnergyStruct(small.energiesPerU, small.peakDepths, small.scaleFacts, small.ciddMatrix, 1.0, small.densityVector[:n_density],
                                 1.0, small.spVector[:n_sp], 1000.0, small.rRlVector)
    dose = [np.zeros_like(scn.ct), np.zeros_like(scn.ct)]
    with engine.Engine(0) as eng:
        eng.set_luts(synth)
        eng.set_ct(scn.ct)
        eng.compute(scn.beams, dose[0])
        for nd, ns in ((65536, 65536), (20481, 20480), (1, 40960)):
            with pytest.raises(engine.RtdError) as e:
                eng.set_luts(tables(nd, ns))
            print("%d + %d entries: status %d, %s" % (nd, ns, e.value.status, e.value))
            assert e.value.status == abi.RTD_ERR_INVALID_ARG and "160 KiB" in str(e.value) and "40960" in str(e.value) and str(nd + ns) in str(e.value)
        eng.compute(scn.beams, dose[1])                               # the handle still holds the tables it had
        np.testing.assert_array_equal(dose[1], dose[0])
        eng.set_luts(tables(20480, 20480))                            # the largest tables taken (set, not computed with)
        eng.set_luts(synth)
        dose[1][:] = 0
        eng.compute(scn.beams, dose[1])
        np.testing.assert_array_equal(dose[1], dose[0])
    assert dose[0].max() > 0
