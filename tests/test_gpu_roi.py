"""GPU tests of the contour rasterisation (rtd_roi_*, include/rtd.h) through the C ABI: the voxel list is compared for EQUALITY with the
numpy restatement (tests/roi_reference.py), which test_roi_reference.py pins by answers known exactly. The rule is comparisons of float64
values and integer counting, so there is no tolerance anywhere in this file.

k_roi_scan takes the edges of a plane 256 at a time (kRoiBlock), in blocks of 32 rows (kRoiRows) by 2048 columns (kRoiSegBits)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import roi_reference as R
import rtstruct_fixture as sfx
from conftest import ROOT
from raytracedicom_amd import abi, scenarios

pytestmark = pytest.mark.gpu

EDGES_PER_PASS = 256      # kRoiBlock of rtd_roi.hpp
M, V = R.IDENTITY


@pytest.fixture
def eng(engine):
    e = engine.Engine(0)
    yield e
    e.close()


def both(eng, dims, m, v, contours, thickness):
    """Rasterises on the device and by the restatement; asserts the lists and the info equal; returns (roi, voxels)."""
    ref, info = R.rasterize(dims, m, v, contours, thickness)
    roi = eng.rasterize_roi(dims, (m, v), contours, thickness)
    got = roi.voxels()
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, ref)
    assert roi.info == info
    return roi, got


def blob(cx, cy, r, z, n=24):
    return R.circle(cx, cy, r, n, z, ry=0.8 * r)


# ---- the smallest shapes that can still go wrong ----
@pytest.mark.parametrize("dims", [(70, 37, 9), (33, 20, 3), (32, 20, 3), (64, 5, 2), (65, 40, 2), (50, 1, 4), (1, 50, 2), (2100, 3, 1)],
                         ids=lambda d: "%dx%dx%d" % d)
def test_grid_shapes(eng, dims):
    """70 x 37 x 9: nx no multiple of 32 or 64, a partial last word, a partial last group of rows. nx = 33 and 32: the difference mask
    needs bit nx in a second word. A single row, a single column, and a row longer than one block's 2048 columns."""
    nx, ny, nz = dims
    contours = []
    for k in range(nz):
        # reaches past the right and the upper edge of the grid, so that the last column, word and row are inside
        contours.append(R.polygon([(0.3 * nx, -2.0), (nx + 3.0, -1.0), (nx + 1.5, 0.6 * ny + 0.4), (0.55 * nx, ny + 2.0), (-1.5, 0.7 * ny), (0.2 * nx, 0.3 * ny)], k))
        if nx > 8 and ny > 8:
            contours.append(blob(0.5 * nx, 0.45 * ny, 0.12 * min(nx, ny), k, n=9))                  # a hole
    roi, vox = both(eng, dims, M, V, contours, 1.0)
    assert vox.size > 0 and roi.info["box_hi"][0] == nx - 1
    roi.close()


# ---- content ----
def test_circle_with_more_edges_than_one_pass(eng):
    n = 5000
    assert n > 19 * EDGES_PER_PASS
    roi, vox = both(eng, (90, 77, 1), M, V, [R.circle(44.3, 38.6, 33.7, n, 0.0)], 1.0)
    assert abs(vox.size - math.pi * 33.7 ** 2) < 0.02 * math.pi * 33.7 ** 2
    roi.close()


def test_triangle(eng):
    roi, vox = both(eng, (40, 30, 2), M, V, [R.polygon([(3.2, 2.1), (35.7, 9.4), (11.9, 27.3)], 1.0)], 1.0)
    assert vox.size > 0 and roi.info["box_lo"][2] == 1
    roi.close()


def test_hole_and_disjoint_contours_on_one_plane(eng):
    contours = [R.circle(30.2, 30.1, 22.0, 60, 2.0), R.circle(31.0, 29.0, 9.5, 31, 2.0), R.rect(60.5, 75.5, 5.5, 50.5, 2.0), blob(67.0, 60.0, 5.0, 2.0)]
    roi, vox = both(eng, (80, 70, 4), M, V, contours, 1.0)
    mask = np.zeros(80 * 70 * 4, dtype=bool)
    mask[vox] = True
    mask = mask.reshape(4, 70, 80)
    assert not mask[2, 29, 31] and mask[2, 30, 12] and mask[2, 20, 65] and not mask[2, 30, 56] and not mask[1].any()
    roi.close()


@pytest.mark.parametrize("side", ["left", "right", "below", "above"])
def test_partly_and_wholly_outside(eng, side):
    nx, ny = 45, 38
    dx, dy = {"left": (-1, 0), "right": (1, 0), "below": (0, -1), "above": (0, 1)}[side]
    cx, cy = 0.5 * nx + dx * 0.5 * nx, 0.5 * ny + dy * 0.5 * ny
    roi, vox = both(eng, (nx, ny, 1), M, V, [blob(cx, cy, 12.3, 0.0)], 1.0)                       # partly: negative xc, xc > nx
    assert 0 < vox.size < 0.6 * math.pi * 12.3 * 0.8 * 12.3
    roi.close()
    roi, vox = both(eng, (nx, ny, 1), M, V, [blob(cx + dx * 40.0, cy + dy * 40.0, 12.3, 0.0)], 1.0)   # wholly
    assert vox.size == 0 and roi.info["n_voxels"] == 0 and roi.info["n_slices_covered"] == 1
    p, n = roi.device()
    assert n == 0
    roi.close()
    roi, vox = both(eng, (nx, ny, 1), M, V, [R.rect(-1e6, 1e6, -1e6, 1e6, 0.0)], 1.0)              # the grid wholly inside
    assert vox.size == nx * ny
    roi.close()


def test_planted_boundary_cases(eng):
    for name, contours, (nx, ny) in R.boundary_cases(z=1.0):
        roi, vox = both(eng, (nx, ny, 3), M, V, contours, 1.0)
        assert vox.size > 0, name
        roi.close()


def test_rotated_world_to_idx(eng):
    """An in-plane rotation by 0.3 rad with anisotropic voxels (0.9 x 1.3 x 2.5 mm) and an origin: contours drawn in index space are
    taken to mm by the inverse, rounded to float32, and come back through float32 matrix entries."""
    c, s = math.cos(0.3), math.sin(0.3)
    rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    to_mm = rot @ np.diag([0.9, 1.3, 2.5])
    origin = np.array([-31.5, 12.25, -40.0])
    m = np.linalg.inv(to_mm).astype(np.float32)
    v = (-np.linalg.inv(to_mm) @ origin).astype(np.float32)
    contours = []
    for k in range(1, 6):
        idx = blob(33.0 + k, 21.5, 14.0 + k, float(k), n=40).astype(np.float64)
        contours.append((idx @ to_mm.T + origin).astype(np.float32))
    roi, vox = both(eng, (70, 48, 7), m, v, contours, 2.5)
    assert roi.info["n_planes"] == 5 and roi.info["n_slices_covered"] == 5 and vox.size > 2000
    roi.close()


@pytest.mark.parametrize("thickness,covered", [(2.5, 14), (1.0, 6), (0.4, 1)])
def test_planes_every_two_and_a_half_slices(eng, thickness, covered):
    """Planes at 0.75 + 2.5 p against integer slices (slice 2 is a tie between two planes at thickness 2.5); thinner slabs leave
    slices between the planes uncovered: at thickness 1.0 the slices 1, 3, 6, 8, 11 (0.25 from a plane) and 12, at 0.4 slice 12 alone."""
    planes = [0.75 + 2.5 * p for p in range(5)] + [12.0]
    contours = [blob(20.0 + p, 18.0, 6.0 + 1.5 * p, z) for p, z in enumerate(planes)]
    roi, vox = both(eng, (48, 40, 14), M, V, contours, thickness)
    assert roi.info["n_planes"] == 6 and roi.info["n_slices_covered"] == covered
    roi.close()


@pytest.mark.parametrize("seed", range(5))
def test_random_star_polygons(eng, seed):
    """200 star-shaped polygons, one per plane, a quarter of their vertices snapped onto rows."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = 61, 45, 200
    contours = [R.star(rng, rng.uniform(10, 50), rng.uniform(8, 37), 2.0, rng.uniform(6.0, 30.0), int(rng.integers(3, 40)), float(k)) for k in range(nz)]
    roi, vox = both(eng, (nx, ny, nz), M, V, contours, 1.0)
    assert vox.size > 10000 and roi.info["n_planes"] == nz
    roi.close()


# ---- the other entry points ----
def _content():
    return (70, 37, 9), [blob(30.0, 18.0, 14.0, float(k)) for k in (1, 2, 3, 6)] + [R.rect(50.5, 75.0, 3.5, 30.5, 6.0)]


def test_fill_mask_and_device_list(eng):
    import torch
    dims, contours = _content()
    roi, vox = both(eng, dims, M, V, contours, 1.0)
    nvox = int(np.prod(dims))
    t = torch.full((nvox,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    roi.fill_mask(t)
    eng.sync()
    exp = np.zeros(nvox, dtype=np.uint8)
    exp[vox] = 1
    np.testing.assert_array_equal(t.cpu().numpy(), exp)
    p, n = roi.device()
    assert n == vox.size and p
    dev = np.empty(n, dtype=np.int32)
    eng.to_host(dev, p)
    np.testing.assert_array_equal(dev, vox)
    # an ROI none of whose planes reaches a slice still writes the whole volume
    far = eng.rasterize_roi(dims, (M, V), [blob(30.0, 18.0, 14.0, 40.0)], 1.0)
    assert far.info["n_voxels"] == 0 and far.info["n_slices_covered"] == 0
    t.fill_(7)
    torch.cuda.synchronize()
    far.fill_mask(t)
    eng.sync()
    assert int(t.max()) == 0
    far.close()
    roi.close()


def test_a_second_engine_gives_the_same_bits(engine, eng):
    dims, contours = _content()
    a = eng.rasterize_roi(dims, (M, V), contours, 1.0)
    with engine.Engine(0) as other:
        b = other.rasterize_roi(dims, (M, V), contours, 1.0)
        vb, ib = b.voxels(), b.info
        b.close()
    again = eng.rasterize_roi(dims, (M, V), contours, 1.0)
    assert a.voxels().tobytes() == vb.tobytes() == again.voxels().tobytes() and a.info == ib
    a.close()
    again.close()


def test_refusals_leave_the_handle_usable(engine, eng):
    dims, contours = _content()
    L = engine.lib()

    def refused(call):
        with pytest.raises(engine.RtdError) as ei:
            call()
        assert ei.value.status == abi.RTD_ERR_INVALID_ARG
        roi, _ = both(eng, dims, M, V, contours, 1.0)                 # everything is still usable
        roi.close()

    good = blob(30.0, 18.0, 14.0, 2.0)
    refused(lambda: eng.rasterize_roi((70, 0, 9), (M, V), contours, 1.0))
    refused(lambda: eng.rasterize_roi((2048, 2048, 512), (M, V), contours, 1.0))                  # 2^31 voxels
    refused(lambda: eng.rasterize_roi(dims, (M, V), [], 1.0))
    refused(lambda: eng.rasterize_roi(dims, (M, V), [good, good[:2]], 1.0))
    for bad in (0.0, -1.0, math.nan, math.inf):
        refused(lambda: eng.rasterize_roi(dims, (M, V), contours, bad))
    nan_pt = good.copy()
    nan_pt[5, 1] = np.nan
    refused(lambda: eng.rasterize_roi(dims, (M, V), [good, nan_pt], 1.0))
    inf_pt = good.copy()
    inf_pt[0, 0] = np.inf
    refused(lambda: eng.rasterize_roi(dims, (M, V), [inf_pt], 1.0))
    m_bad = M.copy()
    m_bad[1, 2] = np.nan
    refused(lambda: eng.rasterize_roi(dims, (m_bad, V), contours, 1.0))
    v_bad = V.copy()
    v_bad[2] = np.inf
    refused(lambda: eng.rasterize_roi(dims, (M, v_bad), contours, 1.0))
    tilted = good.copy()
    tilted[7, 2] += 0.01
    refused(lambda: eng.rasterize_roi(dims, (M, V), [tilted], 1.0))
    # through the C ABI: null pointers and offsets that do not ascend
    g = abi.RtdRoiGrid()
    for i in range(3):
        g.dims[i] = dims[i]
    g.world_to_idx = abi.make_affine(M, V)
    g.plane_thickness_mm = 1.0
    pts = np.ascontiguousarray(np.concatenate([good, good]))
    offs = np.array([0, len(good), 2 * len(good)], dtype=np.uint32)
    s = abi.RtdContourSet()
    s.points, s.offsets, s.n_contours = abi.fptr(pts), offs.ctypes.data_as(C.POINTER(C.c_uint32)), 2
    h = C.c_void_p()
    refused(lambda: eng._check(L.rtd_roi_rasterize(eng._h, None, C.byref(s), C.byref(h))))
    refused(lambda: eng._check(L.rtd_roi_rasterize(eng._h, C.byref(g), None, C.byref(h))))
    refused(lambda: eng._check(L.rtd_roi_rasterize(eng._h, C.byref(g), C.byref(s), None)))
    s.points = None
    refused(lambda: eng._check(L.rtd_roi_rasterize(eng._h, C.byref(g), C.byref(s), C.byref(h))))
    s.points = abi.fptr(pts)
    offs[:] = [len(good), 0, 2 * len(good)]
    refused(lambda: eng._check(L.rtd_roi_rasterize(eng._h, C.byref(g), C.byref(s), C.byref(h))))
    offs[:] = [0, len(good), 2 * len(good)]
    eng._check(L.rtd_roi_rasterize(eng._h, C.byref(g), C.byref(s), C.byref(h)))                   # the same arguments, in order, are accepted
    info = abi.RtdRoiInfo()
    refused(lambda: eng._check(L.rtd_roi_get_info(eng._h, h, None)))
    eng._check(L.rtd_roi_get_info(eng._h, h, C.byref(info)))
    assert info.n_voxels == 0                                         # the same contour twice cancels: XOR
    big = eng.rasterize_roi(dims, (M, V), contours, 1.0)
    small = np.empty(big.info["n_voxels"] - 1, dtype=np.int32)
    refused(lambda: eng._check(L.rtd_roi_voxels(eng._h, big._h, small.ctypes.data_as(C.POINTER(C.c_int32)), small.size)))
    refused(lambda: eng._check(L.rtd_roi_fill_mask(eng._h, big._h, None)))
    big.close()
    eng._check(L.rtd_roi_destroy(eng._h, h))


def test_the_list_goes_into_an_objective(eng):
    dims, contours = _content()
    roi, vox = both(eng, dims, M, V, contours, 1.0)
    nvox = int(np.prod(dims))
    obj = eng.create_objective(dims)
    rid = obj.add_roi(roi.voxels())
    obj.add_term(abi.RTD_OBJ_SQ_DEVIATION, rid, 1.0, 2.0)
    dose = np.random.default_rng(3).random(nvox).astype(np.float32) * 4.0
    d_dose, d_g = eng.device_alloc(4 * nvox), eng.device_alloc(4 * nvox)
    eng.to_device(d_dose, dose)
    eng.device_zero(d_g, 4 * nvox)
    vals = obj.eval(d_dose, d_g)
    exp = float(np.mean((dose[vox].astype(np.float64) - 2.0) ** 2))
    assert math.isfinite(vals[0]) and abs(vals[0] - exp) <= 1e-12 * exp
    empty = eng.rasterize_roi(dims, (M, V), [blob(30.0, 18.0, 14.0, 40.0)], 1.0)
    with pytest.raises(Exception):
        obj.add_roi(empty.voxels())                                   # add_roi goes on refusing the empty list
    empty.close()
    obj.destroy()
    eng.device_free(d_dose)
    eng.device_free(d_g)
    roi.close()


# ---- end to end: RTSTRUCT file -> reader -> rasterise -> objective -> optimiser ----
def test_structure_set_to_optimiser(engine, synth, tmp_path):
    n = 96
    ct, _ = scenarios.hetero_phantom(n)
    scn = scenarios.hetero_ct(synth, n=n, spots=5, pitch=8.0, n_layers=3, angles=[0.0], ct=ct, source_dist=(math.inf, math.inf), seed=5)
    dims = tuple(scn.dims)
    nvox = int(np.prod(dims))
    opts = abi.default_options()
    opts.ray_weight_cutoff = 0.0
    with engine.Engine(0) as eng:
        eng.set_options(opts)
        eng.set_luts(scn.luts)
        eng.set_ct(scn.ct)
        field = eng.create_field(scn.beams[0], dims)
        dij = field.dose_influence()
        w = np.asarray(scn.beams[0].spotWeights, dtype=np.float32)
        dose = dij.matvec(w).reshape(dims[2], dims[1], dims[0])
        hot = np.argwhere(dose > 0.5 * dose.max())                    # (k, j, i)
        k_lo, k_hi = int(hot[:, 0].min()), int(hot[:, 0].max())
        cj, ci = float(hot[:, 1].mean()), float(hot[:, 2].mean())
        # the structure set, in mm of a patient system whose voxels are those of the grid: 2.5 mm voxels, origin (-120, -118.5, -60)
        sp, origin = 2.5, np.array([-120.0, -118.5, -60.0])
        def mm(poly):
            return (np.asarray(poly, dtype=np.float64) * sp + origin).astype(np.float32)
        target = dict(number=1, name="CTV", contours=[dict(points=mm(R.circle(ci, cj, 6.0, 40, float(k)))) for k in range(k_lo, k_hi + 1)])
        oar = dict(number=2, name="OAR ring", contours=[c for k in range(k_lo, k_hi + 1)
                                                       for c in (dict(points=mm(R.circle(ci, cj, 16.0, 48, float(k)))), dict(points=mm(R.circle(ci, cj, 9.0, 32, float(k)))))]
                   + [dict(type="POINT", points=np.zeros((1, 3)))])
        path = str(tmp_path / "rs.dcm")
        sfx.write_rtstruct(path, [target, oar], syntax=sfx.IMPLICIT, undefined_length=False)
        exe = str(tmp_path / "test_rtd_rtstruct")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_rtd_rtstruct.cpp"), "-o", exe])
        out = tmp_path / "out"
        out.mkdir()
        subprocess.check_call([exe, path, str(out)])
        names = [ln.rstrip("\n").split("\t")[3] for ln in open(str(out / "rois.txt"))]
        assert names == ["CTV", "OAR ring"]
        world_to_idx = (np.eye(3, dtype=np.float32) / np.float32(sp), (-origin / sp).astype(np.float32))
        rois = []
        for r in range(2):
            pts = np.fromfile(str(out / ("roi_%d_points.bin" % r)), dtype=np.float32).reshape(-1, 3)
            offs = np.fromfile(str(out / ("roi_%d_offsets.bin" % r)), dtype=np.uint32)
            contours = [pts[a:b] for a, b in zip(offs[:-1], offs[1:])]
            roi = eng.rasterize_roi(dims, world_to_idx, contours, sp)
            ref, _ = R.rasterize(dims, world_to_idx[0], world_to_idx[1], contours, sp)
            np.testing.assert_array_equal(roi.voxels(), ref)
            rois.append(roi)
        assert rois[0].info["n_voxels"] > 100 and rois[1].info["n_voxels"] > 100
        assert np.intersect1d(rois[0].voxels(), rois[1].voxels()).size == 0
        obj = eng.create_objective(dims)
        level = float(dose.reshape(-1)[rois[0].voxels()].mean())
        t_id, o_id = obj.add_roi(rois[0].voxels()), obj.add_roi(rois[1].voxels())
        obj.add_term(abi.RTD_OBJ_SQ_DEVIATION, t_id, 1.0, level)
        obj.add_term(abi.RTD_OBJ_SQ_OVERDOSE, o_id, 1.0, 0.3 * level)
        opt = eng.create_optimizer([field], obj)
        start = np.full(w.shape, 0.5 * float(w.mean()), dtype=np.float32)
        d_w = eng.device_alloc(start.nbytes)
        eng.to_device(d_w, start)
        opt.set_weights(0, d_w)
        opt.run(10)
        rep, hist = opt.result()
        assert hist.size == 10 and np.all(np.isfinite(hist)) and math.isfinite(rep["f_best"])
        assert rep["f_best"] < hist[0]
        opt.destroy()
        obj.destroy()
        eng.device_free(d_w)
        for roi in rois:
            roi.close()
        field.destroy()
