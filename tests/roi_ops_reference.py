"""The numpy restatement of rtd_roi_margin, rtd_roi_combine and rtd_roi_from_mask (include/rtd.h): the cost
tables, the margin by brute force over the table window (shifted boolean arrays, the additions in float32 in the stated order), the
same margin by three one-axis min-plus passes in float32 (the evaluation the kernels rest on), the four boolean ops and the mask
rule. Masks are [Z][Y][X] boolean arrays. A plain module (no tests)."""
import numpy as np

f32 = np.float32
TABLE_MAX = 127
OR, AND, ANDNOT, XOR = 0, 1, 2, 3


class Refused(ValueError):
    """What the C ABI answers with RTD_ERR_INVALID_ARG."""


def six(margin_mm):
    """A scalar, 3 values (one per axis, both sides) or (-x, +x, -y, +y, -z, +z) -> 6 float32."""
    m = np.atleast_1d(np.asarray(margin_mm, dtype=f32)).reshape(-1)
    if m.size == 1:
        m = np.repeat(m, 6)
    elif m.size == 3:
        m = np.repeat(m, 2)
    assert m.size == 6
    return m


def tables(spacing_mm, margin_mm, swap_sides=False):
    """One dict d -> float32 cost per axis (x, y, z). c[0] = 0; on the side with margin m > 0: q = (double(d) * double(s)) / double(m),
    c = float(q * q), held while c <= 1.0f; a side with m == 0 holds only d = 0. c[+d] uses the + margin. swap_sides: the two sides of
    every axis change places (the tables of the expansion of the complement that a contraction is)."""
    sp = np.asarray(spacing_mm, dtype=f32)
    mg = six(margin_mm)
    if sp.shape != (3,) or not (np.isfinite(sp).all() and (sp > 0).all()):
        raise Refused("a spacing is not positive and finite")
    if not (np.isfinite(mg).all() and (mg >= 0).all()):
        raise Refused("a margin is negative or not finite")
    out = []
    for a in range(3):
        s = float(sp[a])
        t = {0: f32(0)}
        for side, sign in ((0, -1), (1, 1)):
            m = float(mg[2 * a + ((1 - side) if swap_sides else side)])
            d = 1
            while m > 0:
                q = (float(d) * s) / m
                c = f32(q * q)
                if not c <= f32(1):
                    break
                if d > TABLE_MAX:
                    raise Refused("a table side holds more than 127 entries")
                t[sign * d] = c
                d += 1
        out.append(t)
    return out


def reach(t):
    """(the farthest d on the - side, on the + side) of one table."""
    return -min(t), max(t)


def shift(a, d, axis, fill):
    """out[p] = a[p - d] along axis, `fill` where p - d leaves the grid."""
    out = np.full_like(a, fill)
    n = a.shape[axis]
    if abs(d) >= n:
        return out
    src, dst = [slice(None)] * 3, [slice(None)] * 3
    if d >= 0:
        src[axis], dst[axis] = slice(0, n - d), slice(d, n)
    else:
        src[axis], dst[axis] = slice(-d, n), slice(0, n + d)
    out[tuple(dst)] = a[tuple(src)]
    return out


def expand_brute(a, t):
    """The definition: p is in iff some q in a has fl(fl(cx[dx] + cy[dy]) + cz[dz]) <= 1 for d = p - q inside the tables."""
    a = np.asarray(a, dtype=bool)
    out = np.zeros_like(a)
    for dx, cx in t[0].items():
        ax = shift(a, dx, 2, False)
        for dy, cy in t[1].items():
            s = f32(cx + cy)
            if not s <= f32(1):
                continue
            axy = None
            for dz, cz in t[2].items():
                if f32(s + cz) <= f32(1):
                    if axy is None:
                        axy = shift(ax, dy, 1, False)
                    out |= shift(axy, dz, 0, False)
    return out


def expand_separable(a, t):
    """min_dz fl(min_dy fl(min_dx cx + cy) + cz) <= 1: three one-axis min-plus passes in float32."""
    a = np.asarray(a, dtype=bool)
    inf = f32(np.inf)
    g = np.where(a, f32(0), inf).astype(f32)
    for axis, tab in ((2, t[0]), (1, t[1]), (0, t[2])):
        best = np.full(a.shape, inf, dtype=f32)
        for d, c in tab.items():
            best = np.minimum(best, (shift(g, d, axis, inf) + c).astype(f32))
        g = best
    return g <= f32(1)


def margin(a, spacing_mm, margin_mm, contract=False, method=expand_brute):
    """rtd_roi_margin. A contraction is the complement within the grid of the expansion of the complement within the grid under the
    tables with the two sides of every axis swapped: voxels outside the grid count as inside the structure."""
    a = np.asarray(a, dtype=bool)
    t = tables(spacing_mm, margin_mm, swap_sides=bool(contract))
    return ~method(~a, t) if contract else method(a, t)


def contract_by_definition(a, spacing_mm, margin_mm):
    """The contraction as include/rtd.h words it first: p in A, and no grid voxel q outside A with the cost of d = q - p <= 1 under the
    tables as given (not swapped). Voxel by voxel: for small masks."""
    a = np.asarray(a, dtype=bool)
    t = tables(spacing_mm, margin_mm)
    nz, ny, nx = a.shape
    out = a.copy()
    for z, y, x in zip(*np.nonzero(a)):
        for dx, cx in t[0].items():
            for dy, cy in t[1].items():
                s = f32(cx + cy)
                for dz, cz in t[2].items():
                    qx, qy, qz = x + dx, y + dy, z + dz
                    if f32(s + cz) <= f32(1) and 0 <= qx < nx and 0 <= qy < ny and 0 <= qz < nz and not a[qz, qy, qx]:
                        out[z, y, x] = False
    return out


def combine(a, b, op):
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    if a.shape != b.shape:
        raise Refused("the two ROIs have different dims")
    if op == OR:
        return a | b
    if op == AND:
        return a & b
    if op == ANDNOT:
        return a & ~b
    if op == XOR:
        return a ^ b
    raise Refused("unknown op")


def from_mask(mask):
    """The voxels whose byte is non-zero."""
    return np.asarray(mask) != 0


def ring(a, inner_mm, outer_mm, spacing_mm, method=expand_brute):
    return combine(margin(a, spacing_mm, outer_mm, method=method), margin(a, spacing_mm, inner_mm, method=method), ANDNOT)


def voxels(a):
    """The strictly ascending linear indices (k ny + j) nx + i of a [Z][Y][X] mask, int32."""
    return np.flatnonzero(np.asarray(a, dtype=bool).reshape(-1)).astype(np.int32)


def info(a):
    """What rtd_roi_get_info reports for a derived ROI: the count, the inclusive box in (i, j, k) (all zero when empty), no planes."""
    a = np.asarray(a, dtype=bool)
    z, y, x = np.nonzero(a)
    if not z.size:
        return {"n_voxels": 0, "box_lo": [0, 0, 0], "box_hi": [0, 0, 0], "n_planes": 0, "n_slices_covered": 0}
    return {"n_voxels": int(z.size), "box_lo": [int(x.min()), int(y.min()), int(z.min())], "box_hi": [int(x.max()), int(y.max()), int(z.max())],
            "n_planes": 0, "n_slices_covered": 0}
