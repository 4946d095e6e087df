"""GPU tests of the derived ROIs (rtd_roi_margin, rtd_roi_combine, rtd_roi_from_mask; include/rtd.h) through the
C ABI: the voxel list and the info are compared for EQUALITY with the numpy restatement (tests/roi_ops_reference.py), which
test_roi_ops_reference.py pins by answers known exactly. The rule is integers and comparisons of float32 values, so there is no
tolerance anywhere in this file.

The kernels' tiles (rtd_roi_ops.hpp): k_roi_margin_xy takes 64 columns by 32 rows (kMarginRows) of one source slice, the source rows 64
at a time (kMarginChunk); k_roi_margin_z takes 64 columns by 4 rows by 16 slices (kMarginSlices); k_roi_from_mask 2048 columns of a row.
Small windows go through the brute force of the restatement, large ones through its three one-axis passes (equal, by the CPU test)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import roi_ops_child as child
import roi_ops_reference as rr
import roi_reference as R
import target_reference as T
import target_scenes as TS
from conftest import ROOT
from raytracedicom_amd import abi

pytestmark = pytest.mark.gpu

f32 = np.float32
ROWS, CHUNK, SLICES = 32, 64, 16           # kMarginRows, kMarginChunk, kMarginSlices
ISO = (1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def eng(engine):
    e = engine.Engine(0)
    yield e
    e.close()


def want_margin(a, sp, mg, contract=False):
    t = rr.tables(sp, mg, swap_sides=contract)
    window = len(t[0]) * len(t[1]) * len(t[2])
    return rr.margin(a, sp, mg, contract, method=rr.expand_brute if window * a.size <= 4e7 else rr.expand_separable)


def same(roi, want):
    got = roi.voxels()
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, rr.voxels(want))
    assert roi.info == rr.info(want), (roi.info, rr.info(want))
    dev, n = roi.device()
    assert n == got.size and (dev != 0 or n == 0)


def check_margin(eng, a, sp, mg, contract=False, src=None):
    """The device's margin of mask `a` against the restatement; the source's list is the same before and after. Returns the result mask."""
    own = src is None
    if own:
        src = child.upload(eng, a)
    before = src.voxels()
    np.testing.assert_array_equal(before, rr.voxels(a))
    out = src.contract(mg, sp) if contract else src.expand(mg, sp)
    want = want_margin(np.asarray(a, dtype=bool), sp, mg, contract)
    same(out, want)
    np.testing.assert_array_equal(src.voxels(), before)
    out.close()
    if own:
        src.close()
    return want


def random_mask(dims, density, seed):
    nx, ny, nz = dims
    return np.random.default_rng(seed).random((nz, ny, nx)) < density


def planted(dims, seed=7):
    """A box that touches the last column, row and slice, a few specks, and a voxel in the first corner."""
    nx, ny, nz = dims
    a = random_mask(dims, 0.003, seed)
    a[nz // 2:, ny // 2:, max(0, nx - 3):] = True
    a[0, 0, 0] = True
    return a


# ---- the smallest shapes that can still go wrong ----
@pytest.mark.parametrize("contract", (False, True), ids=("expand", "contract"))
@pytest.mark.parametrize("dims", [(31, 9, 5), (32, 9, 5), (33, 9, 5), (64, 9, 5), (65, 9, 5), (50, 1, 4), (1, 50, 3), (40, 30, 1), (2100, 3, 2), (70, 37, 9)],
                         ids=lambda d: "%dx%dx%d" % d)
def test_grid_shapes(eng, dims, contract):
    """nx around the word and the tile of 64 columns with the structure on the last column; a single row, column and slice; a row longer
    than one piece of k_roi_from_mask and many column tiles; 70 x 37 x 9 with partial tiles on every axis."""
    a = planted(dims)
    if contract:
        a = ~random_mask(dims, 0.004, 11)                              # nearly full: the contraction eats around every hole
        a[:, :, 0] = True
        a[dims[2] // 2, dims[1] // 2, dims[0] // 2] = False
    want = check_margin(eng, a, (1.0, 1.0, 1.5), (2.0, 3.0, 2.5, 1.0, 1.5, 3.0), contract)
    assert 0 < want.sum() < want.size or min(dims) == 1


def test_halo_from_the_neighbour_tile(eng):
    """ny = ROWS + 1 + both tables and nz = SLICES + 1 + both tables: the last tile's window comes from the tile before it; two blobs
    on either side of the tile borders."""
    L = 3
    dims = (66, ROWS + 1 + 2 * L, SLICES + 1 + 2 * L)
    a = np.zeros((dims[2], dims[1], dims[0]), dtype=bool)
    a[SLICES - 1, ROWS - 1, 63] = a[SLICES, ROWS, 64] = a[SLICES + L, ROWS + L, 2] = a[0, 0, 65] = True
    for contract in (False, True):
        check_margin(eng, ~a if contract else a, ISO, float(L), contract)


# ---- margins ----
MARGINS = {
    "equal": (ISO, 3.0),
    "six": (ISO, (1.0, 4.0, 2.0, 0.0, 3.0, 5.0)),
    "zero-side": (ISO, (0.0, 3.0, 3.0, 3.0, 3.0, 3.0)),
    "zero-axis": (ISO, (3.0, 3.0, 0.0, 0.0, 3.0, 3.0)),
    "zero-z": (ISO, (4.0, 4.0, 4.0, 4.0, 0.0, 0.0)),
    "below-one-spacing": ((1.0, 2.5, 3.0), (0.9, 0.9, 2.4, 2.4, 2.9, 2.9)),
    "exact-5-in": (ISO, 5.0),
    "exact-1.2-6-out": ((f32(1.2), f32(1.2), f32(1.2)), 6.0),
    "anisotropic": ((0.9765625, 0.9765625, 2.5), 5.0),
    "anisotropic-six": ((0.9765625, 0.9765625, 2.5), (7.0, 3.0, 7.0, 3.0, 7.0, 5.0)),
}


@pytest.mark.parametrize("contract", (False, True), ids=("expand", "contract"))
@pytest.mark.parametrize("name", sorted(MARGINS))
def test_margins(eng, name, contract):
    sp, mg = MARGINS[name]
    dims = (70, 37, 19)
    a = planted(dims, seed=3)
    a[5:12, 8:25, 20:50] = True
    if contract:
        a = ~a
        a[:, :, :2] = True
    want = check_margin(eng, a, sp, mg, contract)
    if name == "below-one-spacing":
        assert (want == a).all()                                       # the tables hold only d = 0


def test_all_zero_margins_return_a_copy(eng):
    a = planted((45, 20, 7))
    for contract in (False, True):
        assert (check_margin(eng, a, ISO, 0.0, contract) == a).all()


def test_exact_boundaries_on_a_single_voxel(eng):
    a = np.zeros((13, 13, 13), dtype=bool)
    a[6, 6, 6] = True
    w = check_margin(eng, a, ISO, 5.0)
    assert w.sum() == 515 and w[6, 6, 11] and w[6, 10, 9] and not w[6, 10, 10]
    w = check_margin(eng, a, (f32(1.2),) * 3, 6.0)
    assert w[6, 6, 10] and not w[6, 6, 11] and not w[6, 6, 1]           # d = 5 is out: float32(1.2) lies above 1.2


def test_tables_longer_than_the_grid_and_than_the_tiles(eng):
    """Tables of 40 (y: more than ROWS, a window of more than one CHUNK), 20 (z: more than SLICES) and 70 (x: more than two words) on a
    grid that is shorter than the x and z tables."""
    a = np.zeros((12, 90, 50), dtype=bool)
    a[3, 44, 10] = a[11, 2, 49] = a[6, 40:43, 30:33] = True
    mg = (70.0, 70.0, 40.0, 40.0, 20.0, 20.0)
    assert [rr.reach(t) for t in rr.tables(ISO, mg)] == [(70, 70), (40, 40), (20, 20)] and 40 > ROWS and ROWS + 80 > CHUNK and 20 > SLICES
    w = check_margin(eng, a, ISO, mg)
    assert 0 < w.sum() < w.size
    check_margin(eng, ~a, ISO, mg, contract=True)
    # a z table of 20 (more than SLICES) on three groups of slices: a walk of k_roi_margin_z starts in the group before the one next to it
    c = np.zeros((2 * SLICES + 8, 5, 40), dtype=bool)
    c[0, 2, 3] = c[2 * SLICES + 7, 1, 30] = c[SLICES + 2, 4, 17] = True
    mz = (2.0, 2.0, 1.0, 1.0, 20.0, 20.0)
    assert rr.reach(rr.tables(ISO, mz)[2]) == (20, 20) and c.shape[0] > 2 * SLICES and 20 > SLICES
    w = check_margin(eng, c, ISO, mz)
    assert w[20, 2, 3] and not w[21, 2, 3] and w[2 * SLICES + 7 - 20, 1, 30] and not w[2 * SLICES + 6 - 20, 1, 30]
    check_margin(eng, c, ISO, (2.0, 2.0, 1.0, 1.0, 20.0, 0.0))         # one-sided: only the walk down the column reaches
    check_margin(eng, ~c, ISO, mz, contract=True)
    # the longest table there is, on a row of its own
    b = np.zeros((1, 1, 300), dtype=bool)
    b[0, 0, 150] = True
    w = check_margin(eng, b, ISO, (127.0, 90.0, 0.0, 0.0, 0.0, 0.0))
    assert np.flatnonzero(w[0, 0]).tolist() == list(range(150 - 127, 150 + 91))


# ---- content ----
def test_a_voxel_in_every_corner(eng):
    a = np.zeros((11, 21, 37), dtype=bool)
    for z in (0, 10):
        for y in (0, 20):
            for x in (0, 36):
                a[z, y, x] = True
    w = check_margin(eng, a, (1.0, 1.0, 2.0), 4.0)
    assert w.sum() == 8 * w[:6, :11, :19].sum() > 8
    check_margin(eng, ~a, (1.0, 1.0, 2.0), 4.0, contract=True)


def test_blobs_merge_shell_closes_bridge_is_cut(eng):
    nz, ny, nx = 15, 40, 70
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    two = ((x - 20) ** 2 + (y - 20) ** 2 + (z - 7) ** 2 <= 36) | ((x - 38) ** 2 + (y - 20) ** 2 + (z - 7) ** 2 <= 36)
    assert not two[7, 20, 29]
    w = check_margin(eng, two, ISO, 3.0)
    assert w[7, 20, 27:32].all()                                       # the gap between the blobs is closed
    r2 = (x - 35) ** 2 + (y - 20) ** 2 + (z - 7) ** 2
    shell = (r2 <= 49) & (r2 >= 9)
    assert not shell[7, 20, 35]
    w = check_margin(eng, shell, ISO, 3.0)
    assert w[7, 20, 35] and w[5:10, 18:23, 33:38].all()                # the hole is closed
    bridge = np.zeros((nz, ny, nx), dtype=bool)
    bridge[3:12, 5:35, 5:25] = bridge[3:12, 5:35, 45:65] = True
    bridge[6:9, 19:22, 25:45] = True
    w = check_margin(eng, bridge, ISO, 2.0, contract=True)
    assert w[7, 20, 10] and w[7, 20, 55] and not w[:, :, 25:45].any()   # the bridge is cut, the two bodies stay


def test_contraction_that_empties_the_structure(eng):
    a = np.zeros((9, 20, 40), dtype=bool)
    a[3:6, 5:9, 10:15] = True
    src = child.upload(eng, a)
    out = src.contract(3.0, ISO)
    assert out.info == {"n_voxels": 0, "box_lo": [0, 0, 0], "box_hi": [0, 0, 0], "n_planes": 0, "n_slices_covered": 0}
    assert out.voxels().size == 0 and out.device()[1] == 0
    d = eng.device_alloc(a.size)
    eng.to_device(d, np.full(a.size, 7, dtype=np.uint8))
    out.fill_mask(d)
    back = np.empty(a.size, dtype=np.uint8)
    eng.to_host(back, d)
    eng.device_free(d)
    assert not back.any()
    again = out.expand(3.0, ISO)                                       # an empty ROI is an input like any other
    same(again, np.zeros_like(a))
    for r in (again, out, src):
        r.close()


def test_empty_and_full_sources(eng):
    empty, full = np.zeros((6, 12, 40), dtype=bool), np.ones((6, 12, 40), dtype=bool)
    for a in (empty, full):
        for contract in (False, True):
            w = check_margin(eng, a, ISO, (2.0, 1.0, 3.0, 0.0, 1.0, 1.0), contract)
            assert (w == a).all()


@pytest.mark.parametrize("density", (0.004, 0.5))
def test_random_masks(eng, density):
    a = random_mask((70, 37, 9), density, 5)
    check_margin(eng, a, (1.0, 1.3, 2.0), (3.0, 2.0, 4.1, 0.0, 5.0, 2.0))
    check_margin(eng, ~a if density < 0.1 else a, (1.0, 1.3, 2.0), (3.0, 2.0, 4.1, 0.0, 5.0, 2.0), contract=True)


# ---- contract ----
def test_contract_does_not_erode_at_the_faces(eng):
    full = np.ones((10, 12, 40), dtype=bool)
    for axis in range(3):
        for side in (0, 1):
            a = full.copy()
            cut = [slice(None)] * 3
            cut[axis] = slice(6, None) if side == 0 else slice(0, 3)   # the structure touches one face of this axis only
            a[tuple(cut)] = False
            w = check_margin(eng, a, ISO, 2.0, contract=True)
            keep = [slice(None)] * 3
            keep[axis] = slice(0, 4) if side == 0 else slice(5, None)
            want = np.zeros_like(a)
            want[tuple(keep)] = True
            assert (w == want).all(), (axis, side)


def test_six_sided_margins_act_on_the_opposite_sides(eng):
    a = np.zeros((20, 20, 40), dtype=bool)
    a[5:15, 4:16, 10:30] = True
    mg = (1.0, 3.0, 0.0, 2.0, 4.0, 1.0)
    grown = check_margin(eng, a, ISO, mg)
    z, y, x = np.nonzero(grown)
    assert (x.min(), x.max(), y.min(), y.max(), z.min(), z.max()) == (10 - 1, 29 + 3, 4 - 0, 15 + 2, 5 - 4, 14 + 1)
    shrunk = check_margin(eng, a, ISO, mg, contract=True)
    z, y, x = np.nonzero(shrunk)
    assert (x.min(), x.max(), y.min(), y.max(), z.min(), z.max()) == (10 + 1, 29 - 3, 4 + 0, 15 - 2, 5 + 4, 14 - 1)


# ---- combine ----
def ball(dims, c, r):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= r * r


OPS = (("union", rr.OR), ("intersect", rr.AND), ("subtract", rr.ANDNOT), ("xor", rr.XOR))


@pytest.mark.parametrize("pair", ("overlapping", "disjoint", "nested", "equal", "other-slices", "one-empty"))
def test_combine(eng, pair):
    dims = (70, 37, 19)
    a = ball(dims, (30, 18, 9), 8)
    b = {"overlapping": ball(dims, (37, 20, 11), 7), "disjoint": ball(dims, (60, 30, 15), 4), "nested": ball(dims, (31, 18, 9), 3), "equal": a,
         "other-slices": ball(dims, (30, 18, 16), 2) | ball(dims, (66, 3, 1), 1), "one-empty": np.zeros_like(a)}[pair]
    ra, rb = child.upload(eng, a), child.upload(eng, b)
    va, vb = ra.voxels(), rb.voxels()
    for name, op in OPS:
        for p, q, ma, mb in ((ra, rb, a, b), (rb, ra, b, a)):
            out = getattr(p, name)(q)
            same(out, rr.combine(ma, mb, op))
            out.close()
    np.testing.assert_array_equal(ra.voxels(), va)
    np.testing.assert_array_equal(rb.voxels(), vb)
    ra.close()
    rb.close()


# ---- from mask ----
def test_from_mask_byte_values_and_long_rows(eng):
    rng = np.random.default_rng(9)
    for dims in ((2100, 3, 2), (70, 37, 9), (1, 1, 1), (4097, 2, 1)):
        m = rng.integers(0, 256, size=(dims[2], dims[1], dims[0]), dtype=np.uint8)
        m[rng.random(m.shape) < 0.6] = 0
        m[-1, -1, -1] = 128
        roi = child.upload(eng, m)
        same(roi, rr.from_mask(m))
        roi.close()


def test_from_mask_of_a_torch_tensor(eng):
    import torch
    m = (np.random.default_rng(2).random((5, 11, 45)) < 0.3).astype(np.uint8) * 3
    t = torch.from_numpy(m).to("cuda:0")
    torch.cuda.synchronize()
    roi = eng.roi_from_mask(t)
    assert roi.dims == (45, 11, 5)
    same(roi, m != 0)
    roi.close()
    flat = eng.roi_from_mask(t.reshape(-1), dims=(45, 11, 5))           # explicit dims for another shape of the same bytes
    same(flat, m != 0)
    flat.close()
    with pytest.raises(ValueError):
        eng.roi_from_mask(t, dims=(45, 11, 4))
    with pytest.raises(ValueError):
        eng.roi_from_mask(t.cpu())


def ellipsoid_contours(dims, centre, semi, n_points=40):
    """An ellipsoid in voxel coordinates as closed contours on the grid's slices."""
    out = []
    t = np.linspace(0.0, 2.0 * np.pi, n_points, endpoint=False)
    for k in range(dims[2]):
        s2 = 1.0 - ((k - centre[2]) / semi[2]) ** 2
        if s2 > 0.05:
            s = math.sqrt(s2)
            out.append(np.stack([centre[0] + semi[0] * s * np.cos(t), centre[1] + semi[1] * s * np.sin(t), np.full_like(t, float(k))], axis=1).astype(np.float32))
    return out


def test_from_mask_of_fill_mask_gives_the_list_back(eng):
    dims = (70, 37, 9)
    roi = eng.rasterize_roi(dims, R.IDENTITY, ellipsoid_contours(dims, (33.3, 17.2, 4.1), (20.0, 11.0, 3.5)), 1.0)
    assert roi.info["n_voxels"] > 500 and roi.info["n_planes"] > 0
    d = eng.device_alloc(70 * 37 * 9)
    roi.fill_mask(d)
    back = eng.roi_from_mask(d, dims)
    eng.device_free(d)
    np.testing.assert_array_equal(back.voxels(), roi.voxels())
    assert back.info["n_planes"] == 0 and back.info["n_slices_covered"] == 0
    assert {k: back.info[k] for k in ("n_voxels", "box_lo", "box_hi")} == {k: roi.info[k] for k in ("n_voxels", "box_lo", "box_hi")}
    # a rasterised ROI (slots on the contoured slices only) is a source like any other
    a = np.zeros(9 * 37 * 70, dtype=bool)
    a[roi.voxels()] = True
    a = a.reshape(9, 37, 70)
    for contract in (False, True):
        check_margin(eng, a, (1.0, 1.0, 2.5), (3.0, 2.0, 3.0, 3.0, 5.0, 2.5), contract, src=roi)
    both = roi.union(back)
    same(both, a)
    for r in (both, back, roi):
        r.close()


# ---- chaining and use ----
def test_ring_and_chains(eng):
    dims = (70, 37, 19)
    a = ball(dims, (30, 18, 9), 6)
    b = ball(dims, (36, 18, 9), 4)
    sp = (1.0, 1.0, 1.5)
    ra, rb = child.upload(eng, a), child.upload(eng, b)
    ring = ra.ring(2.0, 5.0, sp)
    want = rr.ring(a, 2.0, 5.0, sp)
    assert want.sum() > 0 and not (want & a).any()
    same(ring, want)
    sub = ra.subtract(rb)
    grown = sub.expand((2.0, 0.0, 3.0, 1.0, 1.5, 1.5), sp)              # expand of subtract of a from_mask
    same(grown, rr.margin(rr.combine(a, b, rr.ANDNOT), sp, (2.0, 0.0, 3.0, 1.0, 1.5, 1.5)))
    # the ring's list is what an objective takes
    n = 70 * 37 * 19
    obj = eng.create_objective(dims)
    obj.add_term(abi.RTD_OBJ_SQ_DEVIATION, obj.add_roi(ring.voxels()), 1.0, 2.0)
    d_dose, d_g = eng.device_alloc(4 * n), eng.device_alloc(4 * n)
    eng.to_device(d_dose, np.full(n, 1.5, dtype=np.float32))
    eng.device_zero(d_g, 4 * n)
    values = obj.eval(d_dose, d_g)
    g = np.empty(n, dtype=np.float32)
    eng.to_host(g, d_g)
    assert values[0] > 0 and math.isfinite(values[0])
    assert ((g != 0) == want.reshape(-1)).all()
    obj.destroy()
    for p in (d_dose, d_g):
        eng.device_free(p)
    for r in (grown, sub, ring, ra, rb):
        r.close()


def test_expanded_target_selects_a_superset_of_the_spots(engine, synth):
    scn = TS.scene(synth, "A")
    beam, dims = scn.beams[0], scn.dose_dims
    nvox = int(np.prod(dims))
    with engine.Engine(0) as eng:
        eng.set_options(TS.options())
        eng.set_luts(scn.luts)
        eng.set_ct(scn.ct)
        d_dose, d_mask = eng.device_alloc(4 * nvox), eng.device_alloc(nvox)
        eng.device_zero(d_dose, 4 * nvox)
        field = eng.create_field(beam, dims)
        field.compute(d_dose)
        _, info = field.finish()
        g = T.geometry_of(info, beam)
        wepl = field.fetch("wepl").reshape(g.S, g.H, g.W)
        peaks = field.fetch("layer_plan").reshape(-1, 8)[:, 2].copy()
        centre = TS.central_point(scn, g, wepl, peaks)
        sp, origin = np.asarray(scn.dose_spacing, dtype=np.float64), np.asarray(scn.dose_origin, dtype=np.float64)
        c_idx = (np.asarray(centre) - origin) / sp
        semi = np.asarray(TS.SEMI_AXES) / sp * 0.6                      # a small target: room for the margin to add spots
        roi = eng.rasterize_roi(dims, R.IDENTITY, ellipsoid_contours(dims, c_idx, semi), 1.0)
        assert roi.info["n_voxels"] > 50
        grown = roi.expand(5.0, scn.dose_spacing)
        a = np.zeros(nvox, dtype=bool)
        a[roi.voxels()] = True
        same(grown, want_margin(a.reshape(dims[2], dims[1], dims[0]), scn.dose_spacing, 5.0))
        selected = []
        for r in (roi, grown):
            r.fill_mask(d_mask)
            assert field.project_target(d_mask)["n_samples"] > 0
            selected.append(field.select_spots())
        assert grown.info["n_voxels"] > roi.info["n_voxels"]
        assert selected[0].sum() >= 1 and (selected[1] >= selected[0]).all()
        for r in (grown, roi):
            r.close()
        field.destroy()
        eng.device_free(d_dose)
        eng.device_free(d_mask)


# ---- the second implementation ----
def test_naive_kernel_gives_the_same_lists(eng, tmp_path):
    """RTD_ROI_MARGIN_NAIVE (read when a handle is created) in a child process, the separable kernels here, on 200 x 180 x 60 with a
    12-voxel table; both equal the restatement's three one-axis passes."""
    out = str(tmp_path / "naive.npz")
    env = dict(os.environ, RTD_ROI_MARGIN_NAIVE="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "roi_ops_child.py"), out], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "RTD_ROI_MARGIN_NAIVE" not in os.environ
    naive = np.load(out)
    here = child.run(eng)
    a = child.mid_mask()
    for name, margins, contract in child.CASES:
        want = rr.voxels(rr.margin(a, child.SPACING, margins, contract, method=rr.expand_separable))
        assert 1000 < want.size < a.size and want.size != a.sum()
        np.testing.assert_array_equal(here[name], want, err_msg=name)
        np.testing.assert_array_equal(naive[name], want, err_msg=name + " (naive)")


# ---- determinism and refusals ----
def test_a_second_engine_gives_the_same_bits(engine, eng):
    a = planted((70, 37, 9), seed=21)
    args = ((1.0, 1.0, 2.0), (3.0, 2.0, 4.0, 1.0, 2.0, 4.0))
    lists = []
    for e in (eng, engine.Engine(0), eng):
        src = child.upload(e, a)
        r1, r2 = src.expand(*reversed(args)), src.contract(*reversed(args))
        x = r1.xor(r2)
        lists.append((r1.voxels(), r2.voxels(), x.voxels()))
        for r in (x, r2, r1, src):
            r.close()
        if e is not eng:
            e.close()
    for other in lists[1:]:
        for p, q in zip(lists[0], other):
            np.testing.assert_array_equal(p, q)


def test_refusals_leave_the_handle_usable(engine, eng):
    L = engine.lib()
    a = planted((40, 20, 6))
    src = child.upload(eng, a)
    other = child.upload(eng, np.ones((6, 20, 41), dtype=bool))
    before = src.voxels()
    sp3, mg6 = (C.c_float * 3)(1, 1, 1), (C.c_float * 6)(2, 2, 2, 2, 2, 2)
    good = abi.uint3((40, 20, 6))
    d = eng.device_alloc(40 * 20 * 6)
    eng.device_zero(d, 40 * 20 * 6)

    def margin(src_h=src._h, sp=sp3, mg=mg6, contract=0, with_out=True):
        out = C.c_void_p(1)
        return L.rtd_roi_margin(eng._h, src_h, sp, mg, contract, C.byref(out) if with_out else None), out.value

    def combine(a_h=src._h, b_h=src._h, op=abi.RTD_ROI_OR, with_out=True):
        out = C.c_void_p(1)
        return L.rtd_roi_combine(eng._h, a_h, b_h, op, C.byref(out) if with_out else None), out.value

    def from_mask(dims=good, ptr=d, with_out=True):
        out = C.c_void_p(1)
        return L.rtd_roi_from_mask(eng._h, dims, C.c_void_p(ptr) if ptr else None, C.byref(out) if with_out else None), out.value

    def f3(*v):
        return (C.c_float * 3)(*v)

    def f6(*v):
        return (C.c_float * 6)(*v)

    without_out = [lambda: margin(with_out=False), lambda: combine(with_out=False), lambda: from_mask(with_out=False)]
    bad = [lambda: margin(src_h=None), lambda: margin(sp=None), lambda: margin(mg=None),
           lambda: margin(sp=f3(0, 1, 1)), lambda: margin(sp=f3(1, -1, 1)), lambda: margin(sp=f3(1, 1, math.inf)), lambda: margin(sp=f3(math.nan, 1, 1)),
           lambda: margin(mg=f6(2, 2, -1, 2, 2, 2)), lambda: margin(mg=f6(2, 2, 2, math.nan, 2, 2)), lambda: margin(mg=f6(2, 2, 2, 2, 2, math.inf)),
           lambda: margin(mg=f6(0, 128, 0, 0, 0, 0)), lambda: margin(contract=2), lambda: margin(contract=-1),
           lambda: combine(a_h=None), lambda: combine(b_h=None), lambda: combine(op=4), lambda: combine(op=-1),
           lambda: combine(b_h=other._h),
           lambda: from_mask(dims=None), lambda: from_mask(ptr=None), lambda: from_mask(dims=abi.uint3((40, 0, 6))),
           lambda: from_mask(dims=abi.uint3((2048, 2048, 512)))]
    grown = rr.info(rr.margin(a, ISO, 2.0))
    assert grown["n_voxels"] > int(a.sum()) > 0
    good_calls = ((lambda: src.expand(2.0, ISO), grown), (lambda: src.union(src), rr.info(a)), (lambda: eng.roi_from_mask(d, (40, 20, 6)), rr.info(np.zeros_like(a))))
    for i, call in enumerate(bad + without_out):
        st, out = call()
        # *out = NULL where there is an out; the seed 1 stays where none was passed
        assert st == abi.RTD_ERR_INVALID_ARG and out == (None if i < len(bad) else 1), (i, st, out)
        assert L.rtd_last_error(eng._h), i
        # a good call on the same handle, its info against the restatement
        good_call, want_info = good_calls[i % 3]
        r = good_call()
        assert r.info == want_info, (i, r.info, want_info)
        r.close()
    st, out = margin(mg=f6(127, 0, 0, 0, 0, 0))
    assert st == abi.RTD_OK and out
    L.rtd_roi_destroy(eng._h, C.c_void_p(out))
    same(src, a)
    np.testing.assert_array_equal(src.voxels(), before)
    eng.device_free(d)
    src.close()
    other.close()
