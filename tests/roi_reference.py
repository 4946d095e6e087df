"""numpy restatement of the contour rasterisation of include/rtd.h (section "RT Structure Set contours -> ROI voxel lists"): the
transform, the planarity check, the planes, the slice assignment and ONE inside test per voxel centre, written from the definition (no
scanline bookkeeping). float64 throughout; numpy rounds every operation and contracts nothing, as the engine's build does.

rasterize(dims, m, v, contours, thickness) -> (voxels int32 ascending, info dict). ValueError where the engine returns INVALID_ARG."""
import numpy as np

PLANE_TOL = 1e-3


def transform(m, v, pts):
    """(u, v, kc) float64 of float32 points (n, 3): ((m0 x + m1 y) + m2 z) + v0, and rows 1 and 2 likewise."""
    m = np.asarray(m, dtype=np.float32).reshape(9).astype(np.float64)
    v = np.asarray(v, dtype=np.float32).reshape(3).astype(np.float64)
    p = np.asarray(pts, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return tuple(((m[3 * r] * x + m[3 * r + 1] * y) + m[3 * r + 2] * z) + v[r] for r in range(3))


def planes_of(m, v, contours):
    """[(kc_p, [(u, v) of every contour of the plane])], ascending in kc_p."""
    items = []
    for c in contours:
        c = np.asarray(c, dtype=np.float32).reshape(-1, 3)
        if len(c) < 3:
            raise ValueError("a contour needs at least 3 points")
        if not np.all(np.isfinite(c)):
            raise ValueError("a coordinate is not finite")
        u, w, kc = transform(m, v, c)
        if np.any(np.abs(kc - kc[0]) > PLANE_TOL):
            raise ValueError("a contour is not planar in the grid's k")
        items.append((float(kc[0]), u, w))
    if not items:
        raise ValueError("no contours")
    order = sorted(range(len(items)), key=lambda i: items[i][0])      # (sorted is stable)
    planes = []
    for i in order:
        kc, u, w = items[i]
        if not planes or kc - planes[-1][0] > PLANE_TOL:
            planes.append((kc, []))
        planes[-1][1].append((u, w))
    return planes


def slab_of(m, thickness):
    m = np.asarray(m, dtype=np.float32).reshape(9).astype(np.float64)
    return float(np.float64(np.float32(thickness)) * np.sqrt((m[6] * m[6] + m[7] * m[7]) + m[8] * m[8]))


def assign_slices(plane_kc, nz, slab):
    """Per slice k the index of its plane or -1: the nearest plane, a tie to the lower coordinate, only within slab / 2."""
    kc = np.asarray(plane_kc, dtype=np.float64)
    out = np.full(nz, -1, dtype=np.int64)
    for k in range(nz):
        d = np.abs(np.float64(k) - kc)
        p = int(np.argmin(d))                                         # (the first minimum: the planes ascend)
        if d[p] <= slab / 2:
            out[k] = p
    return out


def edges_of(polys):
    """(au, av, bu, bv) of all edges of all contours of one plane; the last point closes to the first."""
    au = np.concatenate([u for u, _ in polys])
    av = np.concatenate([w for _, w in polys])
    bu = np.concatenate([np.roll(u, -1) for u, _ in polys])
    bv = np.concatenate([np.roll(w, -1) for _, w in polys])
    return au, av, bu, bv


def inside_plane(polys, nx, ny):
    """bool [ny][nx]: voxel (i, j) is flipped by every edge that crosses row j with double(i) < xc; inside iff flipped an odd number of times."""
    au, av, bu, bv = edges_of(polys)
    i = np.arange(nx, dtype=np.float64)
    out = np.zeros((ny, nx), dtype=bool)
    for j in range(ny):
        dj = np.float64(j)
        cross = (av <= dj) != (bv <= dj)
        if not cross.any():
            continue
        a_u, a_v, b_u, b_v = au[cross], av[cross], bu[cross], bv[cross]
        t = (dj - a_v) / (b_v - a_v)
        xc = a_u + t * (b_u - a_u)
        flips = (i[None, :] < xc[:, None]).sum(axis=0)
        out[j] = (flips & 1).astype(bool)
    return out


def rasterize(dims, m, v, contours, thickness):
    nx, ny, nz = (int(d) for d in dims)
    if min(nx, ny, nz) < 1 or nx * ny * nz > 2 ** 31 - 1:
        raise ValueError("a zero dimension or more than 2^31 - 1 voxels")
    if not (np.all(np.isfinite(np.asarray(m, dtype=np.float32))) and np.all(np.isfinite(np.asarray(v, dtype=np.float32)))):
        raise ValueError("a matrix entry is not finite")
    th = np.float32(thickness)
    if not (th > 0 and np.isfinite(th)):
        raise ValueError("plane_thickness_mm must be positive and finite")
    planes = planes_of(m, v, contours)
    take = assign_slices([p[0] for p in planes], nz, slab_of(m, thickness))
    masks = {}
    vol = np.zeros((nz, ny, nx), dtype=bool)
    for k in range(nz):
        p = int(take[k])
        if p < 0:
            continue
        if p not in masks:
            masks[p] = inside_plane(planes[p][1], nx, ny)
        vol[k] = masks[p]
    vox = np.flatnonzero(vol).astype(np.int32)
    info = {"n_voxels": int(vox.size), "box_lo": [0, 0, 0], "box_hi": [0, 0, 0], "n_planes": len(planes), "n_slices_covered": int((take >= 0).sum())}
    if vox.size:
        kk, jj, ii = np.nonzero(vol)
        info["box_lo"] = [int(ii.min()), int(jj.min()), int(kk.min())]
        info["box_hi"] = [int(ii.max()), int(jj.max()), int(kk.max())]
    return vox, info


# ---- shapes the tests share ----
IDENTITY = (np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32))


def polygon(uv, z):
    """(n, 3) float32 points of a polygon given in (x, y) at height z (under the identity transform x = u, y = v, z = k)."""
    uv = np.asarray(uv, dtype=np.float64)
    return np.concatenate([uv, np.full((len(uv), 1), z)], axis=1).astype(np.float32)


def rect(x0, x1, y0, y1, z):
    return polygon([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], z)


def circle(cx, cy, r, n, z, ry=None):
    a = 2.0 * np.pi * np.arange(n) / n
    return polygon(np.stack([cx + r * np.cos(a), cy + (r if ry is None else ry) * np.sin(a)], axis=1), z)


def star(rng, cx, cy, r_lo, r_hi, n, z, snap=0.25):
    """A star-shaped polygon (radii random per vertex); a fraction `snap` of the vertices is moved onto the nearest row."""
    a = np.sort(rng.uniform(0.0, 2.0 * np.pi, n))
    r = rng.uniform(r_lo, r_hi, n)
    uv = np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1)
    on_row = rng.random(n) < snap
    uv[on_row, 1] = np.round(uv[on_row, 1])
    return polygon(uv, z)


def boundary_cases(z=0.0):
    """The planted boundary cases, as (name, contours, dims (nx, ny), expected inside set of (i, j) or None):
    vertices exactly on rows, a horizontal edge on a row, a crossing exactly at a voxel centre."""
    cases = []
    # a diamond with all four vertices on voxel centres: rows 2..5 (av <= j decides: the bottom vertex row is in, the top one is out)
    cases.append(("diamond_on_centres", [polygon([(4, 2), (7, 5), (4, 8), (1, 5)], z)], (10, 10)))
    # a rectangle whose horizontal edges lie exactly on rows 2 and 6 and whose vertical edges lie exactly on columns 3 and 8
    cases.append(("rect_on_rows_and_columns", [rect(3, 8, 2, 6, z)], (12, 9)))
    # a triangle whose slanted edge crosses row 4 exactly at the voxel centre i = 5 (dyadic: exact in float64)
    cases.append(("crossing_on_centre", [polygon([(1, 0), (9, 8), (1, 8)], z)], (12, 10)))
    # a vertex that touches a row from above and one from below without crossing it
    cases.append(("touching_vertices", [polygon([(1, 1.5), (3, 3), (5, 1.5), (7, 3), (9, 1.5), (9, 6), (5, 3), (1, 6)], z)], (11, 8)))
    return cases
