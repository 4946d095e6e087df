"""The compact form of a dose-influence matrix and the trees of its two products (include/rtd.h "Compact dose-influence matrix",
DESIGN.md section 28), restated in numpy from that prose. A test helper, not product code: the format is fixed by the matrix and a
few constants, so every packed array and every bit of `Dij w` and `Dij^T g` can be predicted.

The matrix is CSC (indptr int64 [n_spots + 1], indices int32 voxel numbers ascending within a column, data float32).

VALUES. m_j = max |v| of column j; frexp(m_j) = (f, e_j), f in [0.5, 1); s_j = 2^(e_j - 15); code = binary16(v * 2^(15 - e_j)), round to
nearest even; an empty or all-zero column: s_j = 1, codes 0. v^ = float(code) * s_j is exact in float32 and
|v^ - v| <= max(2^-11 |v|, 2^-25 s_j): binary16 has 11 significant bits (half an ulp is 2^-11 relative) down to its normal range, and
below it a fixed spacing of 2^-24 (half of it 2^-25), both in units of s_j.
Refused: a value that is not finite, a column with 0 < m_j < 2^-100, more than 65 536 columns.
CSC SIDE. Chunks of CHUNK entries per column, groups of GROUP entries per chunk; a group's base is its first entry's voxel, an entry's
offset its voxel minus the base; base[32 c + g] for group g of chunk c (chunks numbered through the columns), 0 where a chunk is short.
row_bits = 32 if any offset exceeds 65 535.
COMPANION SIDE. Rows are given per entry (`rows`, numbers in [0, n_rows)); within a row the columns ascend. Rows padded to a multiple of
E; pointer r = start (a multiple of E) + the row's pads (E > 1), pointer n_rows = all entries; pads have code 0 and column 0.
FORWARD TREE. ws = fl(w * s); lane t of G adds fl(float(code) * ws[col]) of the row's entries (k G + t) E + e, e = 0 .. E - 1, then
k = 0, 1, ..., from +0; butterfly at G / 2 .. 1. TRANSPOSED. tree_reference.apply_t_tree on float(code), then fl(s_j * sum)."""
import numpy as np

import tree_reference as tr

CHUNK, GROUP = 2048, 64
GROUPS_PER_CHUNK = CHUNK // GROUP
MAX_SPOTS = 65536
TINY = 2.0 ** -100


def _csc(indptr, indices, data):
    return tr._csc(indptr, indices, data)


def refusal(indptr, data, n_spots=None):
    """None, or why the build refuses the matrix."""
    indptr = np.asarray(indptr, dtype=np.int64)
    data = np.asarray(data, dtype=np.float32)
    n = indptr.size - 1 if n_spots is None else int(n_spots)
    if n > MAX_SPOTS:
        return "spots"
    if not np.all(np.isfinite(data)):
        return "not finite"
    m = column_max(indptr, data)
    if np.any((m > 0) & (m < TINY)):
        return "tiny"
    return None


def column_max(indptr, data):
    indptr = np.asarray(indptr, dtype=np.int64)
    a = np.abs(np.asarray(data, dtype=np.float32))
    m = np.zeros(indptr.size - 1, dtype=np.float32)
    cols = np.flatnonzero(np.diff(indptr))
    if cols.size:
        m[cols] = np.maximum.reduceat(a, indptr[cols])
    return m


def quantize(indptr, data):
    """(scale float32 [n_spots], exponent int [n_spots], codes uint16 [nnz])."""
    indptr = np.asarray(indptr, dtype=np.int64)
    data = np.asarray(data, dtype=np.float32)
    m = column_max(indptr, data)
    _, e = np.frexp(m.astype(np.float64))
    e = np.where(m > 0, e, 15).astype(np.int64)                        # s = 1 for an empty or all-zero column
    scale = np.ldexp(1.0, e - 15).astype(np.float32)
    col = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    scaled = np.ldexp(data.astype(np.float64), 15 - e[col])            # a product by a power of two: exact in float64
    codes = scaled.astype(np.float16).view(np.uint16)
    return scale, e, codes


def dequantize(codes, scale, indptr):
    """v^ per entry in float32, and the same product in float64 (they must agree: the product is exact)."""
    col = np.repeat(np.arange(np.asarray(indptr).size - 1), np.diff(indptr))
    c32 = np.asarray(codes, dtype=np.uint16).view(np.float16).astype(np.float32)
    return c32 * scale[col], c32.astype(np.float64) * scale[col].astype(np.float64)


def entry_bound(data, scale, indptr):
    """max(2^-11 |v|, 2^-25 s_j) per entry, float64."""
    col = np.repeat(np.arange(np.asarray(indptr).size - 1), np.diff(indptr))
    return np.maximum(2.0 ** -11 * np.abs(np.asarray(data, dtype=np.float64)), 2.0 ** -25 * scale[col].astype(np.float64))


def chunks(indptr):
    """(chunk start, chunk length, chunk column, first chunk per column [n_spots + 1])."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n_chunks = -(-np.diff(indptr) // CHUNK)
    first = np.concatenate([[0], np.cumsum(n_chunks)]).astype(np.int64)
    ccol = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), n_chunks)
    cstart = indptr[ccol] + (np.arange(ccol.size, dtype=np.int64) - first[ccol]) * CHUNK
    clen = np.minimum(cstart + CHUNK, indptr[ccol + 1]) - cstart
    return cstart, clen, ccol, first


def pack_csc(indptr, indices):
    """(base int32 [32 * n_chunks], offset uint16 [nnz] (cut to 16 bits), row_bits)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    cstart, clen, _, _ = chunks(indptr)
    base = np.zeros(GROUPS_PER_CHUNK * cstart.size, dtype=np.int32)
    first_of_entry = np.zeros(indices.size, dtype=np.int64)
    for c in range(cstart.size):
        for g in range(-(-int(clen[c]) // GROUP)):
            a = int(cstart[c]) + g * GROUP
            b = min(a + GROUP, int(cstart[c] + clen[c]))
            base[GROUPS_PER_CHUNK * c + g] = indices[a]
            first_of_entry[a:b] = indices[a]
    off = indices - first_of_entry
    row_bits = 32 if off.size and off.max() > 65535 else 16
    return base, (off & 0xFFFF).astype(np.uint16), row_bits


def box_rows(indices, dims, box):
    """The companion's row number of every entry: the voxel's place in the row box (x0, y0, z0, bw, bh, bd), x fastest."""
    v = np.asarray(indices, dtype=np.int64)
    nx, ny = int(dims[0]), int(dims[1])
    x, y, z = v % nx, (v // nx) % ny, v // (nx * ny)
    x0, y0, z0, bw, bh, bd = (int(t) for t in box)
    assert v.size == 0 or (x.min() >= x0 and x.max() < x0 + bw and y.min() >= y0 and y.max() < y0 + bh and z.min() >= z0 and z.max() < z0 + bd)
    return ((z - z0) * bh + (y - y0)) * bw + (x - x0)


def box_voxels(dims, box):
    """The voxel number of every row of the box."""
    nx, ny = int(dims[0]), int(dims[1])
    x0, y0, z0, bw, bh, bd = (int(t) for t in box)
    r = np.arange(bw * bh * bd, dtype=np.int64)
    return ((z0 + r // (bw * bh)) * ny + y0 + (r // bw) % bh) * nx + x0 + r % bw


def pack_rows(indptr, rows, codes, n_rows, E):
    """(row_ptr int64 [n_rows + 1] with the pad counts in the low bits, row_code uint16, row_col uint16, count per row)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    col = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
    order = np.argsort(rows, kind="stable")                            # within a row the CSC order: ascending column
    count = np.bincount(rows, minlength=n_rows).astype(np.int64)
    padded = -(-count // E) * E
    start = np.concatenate([[0], np.cumsum(padded)]).astype(np.int64)
    plain_start = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    row_code = np.zeros(int(start[-1]), dtype=np.uint16)
    row_col = np.zeros(int(start[-1]), dtype=np.uint16)
    r_sorted = rows[order]
    at = start[r_sorted] + (np.arange(rows.size, dtype=np.int64) - plain_start[r_sorted])
    row_code[at] = np.asarray(codes, dtype=np.uint16)[order]
    row_col[at] = col[order].astype(np.uint16)
    row_ptr = start.copy()
    row_ptr[:-1] += padded - count
    return row_ptr, row_code, row_col, count


def _lane_sums(prod, start, length, G, E):
    """Lane t's sequential float32 sum of the segment's entries (k G + t) E + e -> [segments, G]."""
    start, length = np.asarray(start, dtype=np.int64), np.asarray(length, dtype=np.int64)
    acc = np.zeros((start.size, G), dtype=np.float32)
    t = np.arange(G, dtype=np.int64)
    trips = int(-(-length.max() // (G * E))) if length.size else 0
    live = np.arange(start.size)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(trips):
            live = live[length[live] > k * G * E]
            for e in range(E):
                pos = (k * G + t[None, :]) * E + e
                have = pos < length[live][:, None]
                at = np.where(have, start[live][:, None] + pos, 0)
                acc[live] = acc[live] + np.where(have, prod[at], np.float32(0.0))
    return acc


def apply_tree(indptr, rows, codes, scale, w, n_rows, G, E):
    """Dij w with the compact form -> (float32 [n_rows], entries per row)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        ws = np.asarray(w, dtype=np.float32).reshape(-1) * scale
        col = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
        order = np.argsort(rows, kind="stable")
        c32 = np.asarray(codes, dtype=np.uint16).view(np.float16).astype(np.float32)
        prod = (c32 * ws[col])[order]
    count = np.bincount(rows, minlength=n_rows).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
    out = np.zeros(n_rows, dtype=np.float32)
    live = np.flatnonzero(count)
    if live.size:
        with np.errstate(invalid="ignore", over="ignore"):
            out[live] = tr._butterfly(_lane_sums(prod, start[live], count[live], G, E))
    return out, count


def apply_t_tree(indptr, indices, codes, scale, g):
    """Dij^T g with the compact form -> float32 [n_spots]."""
    c32 = np.asarray(codes, dtype=np.uint16).view(np.float16).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return scale * tr.apply_t_tree(indptr, indices, c32, g, chunk=CHUNK)


def apply_depth(row_len, G, E):
    """The longest chain of additions of the forward tree for rows of row_len entries."""
    n = np.asarray(row_len, dtype=np.int64)
    return -(-n // (G * E)) * E + int(np.log2(G))
