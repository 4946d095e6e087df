"""The summation trees of the two products with the resident dose-influence matrix (the header comment of
rtd_dij_apply.hpp), restated in numpy float32 from that prose. A test helper, not product code: the trees are fixed by the matrix and
two constants, so the bits of `Dij w` and `Dij^T g` can be predicted, and a product that dropped an entry, a lane or a chunk of a
long column differs from the prediction however small the dropped part is.

Both take the matrix as CSC (indptr int64 [n_spots + 1], indices int32 row numbers ascending within a column, data float32). Every
product is rounded to float32 before it is added; every sum starts from +0.0 (so a row or column without entries gives +0.0, and
padding a lane with +0.0 addends changes no bit: a sum that started from +0.0 is never -0.0).

The tree-depth bound. A float32 sum whose every addend passes through at most d additions, of products that were themselves rounded
once, differs from the exact sum by at most (d + 1) u * sum |a| |x|, u = 2^-24: each addend meets at most d + 1 roundings, and the
first-order bound holds without a higher-order term (Jeannerod and Rump, "Improved error bounds for inner products in floating-point
arithmetic", SIAM J. Matrix Anal. Appl. 34, 2013: n u for a dot product in any order of evaluation; the depth of the tree stands for
n when the additions are not all in sequence). The longest path:
  apply    a lane adds ceil(n / G) entries in sequence, then log2(G) = 4 butterfly levels:              d = ceil(n / 16) + 4;
  apply_t  a lane adds at most 32 entries of a chunk, 6 butterfly levels, then a lane adds ceil(chunks / 64) chunk sums, 6 more
           levels:                                                                                     d = 32 + 6 + ceil(chunks / 64) + 6.
For a column of 200 000 entries (98 chunks) that is d = 46 against the order-free gamma(n) with n = 200 000: 4000 times tighter."""
import numpy as np

U = 2.0 ** -24


def _butterfly(v):
    """v [rows, lanes] float32: every lane adds the lane at distance lanes / 2, ..., 1 (xor); lane 0's sum per row."""
    lanes = v.shape[1]
    idx = np.arange(lanes)
    m = lanes // 2
    while m >= 1:
        v = v + v[:, idx ^ m]
        m //= 2
    return v[:, 0]


def _strided_lane_sums(prod, start, length, lanes):
    """For every segment s (prod[start[s] : start[s] + length[s]], float32): lane t's sequential float32 sum of the segment's entries
    t, t + lanes, ... from +0.0 -> [segments, lanes] float32."""
    start, length = np.asarray(start, dtype=np.int64), np.asarray(length, dtype=np.int64)
    acc = np.zeros((start.size, lanes), dtype=np.float32)
    t = np.arange(lanes, dtype=np.int64)
    trips = int(-(-length.max() // lanes)) if length.size else 0
    live = np.arange(start.size)
    for k in range(trips):
        live = live[length[live] > k * lanes]                          # segments that still have entries in this trip
        pos = k * lanes + t[None, :]                                   # [1, lanes]
        have = pos < length[live][:, None]
        at = np.where(have, start[live][:, None] + pos, 0)
        acc[live] = acc[live] + np.where(have, prod[at], np.float32(0.0))
    return acc


def _csc(indptr, indices, data):
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    data = np.asarray(data, dtype=np.float32)
    assert indptr.ndim == 1 and indptr[0] == 0 and indptr[-1] == indices.size == data.size
    return indptr, indices, data


def apply_tree(indptr, indices, data, w, G=16, n_rows=None):
    """Dij w in the tree of `apply` -> float32 [n_rows] (n_rows: default the largest row number + 1): per voxel the entries in
    ascending column order, lane t of G adds the entries t, t + G, ..., the G lane sums in a butterfly at distances G / 2 ... 1."""
    indptr, indices, data = _csc(indptr, indices, data)
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    assert w.size == indptr.size - 1 and G >= 1 and G & (G - 1) == 0
    n_rows = int(indices.max()) + 1 if n_rows is None and indices.size else int(n_rows or 0)
    col = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
    order = np.argsort(indices, kind="stable")                         # by row; within a row the CSC order, which is ascending column
    prod = (data * w[col])[order]                                      # float32 * float32, rounded to float32
    count = np.bincount(indices, minlength=n_rows)
    start = np.concatenate([[0], np.cumsum(count)[:-1]]) if n_rows else np.zeros(0, dtype=np.int64)
    rows = np.flatnonzero(count)
    out = np.zeros(n_rows, dtype=np.float32)
    if rows.size:
        out[rows] = _butterfly(_strided_lane_sums(prod, start[rows], count[rows], G))
    return out


def apply_t_tree(indptr, indices, data, g, chunk=2048):
    """Dij^T g in the tree of `apply_t` -> float32 [n_spots]: per column chunks of `chunk` consecutive entries; in a chunk lane t of 64
    adds the entries t, t + 64, ..., butterfly at 32 ... 1; lane t then adds the column's chunk sums t, t + 64, ..., butterfly again."""
    indptr, indices, data = _csc(indptr, indices, data)
    g = np.asarray(g, dtype=np.float32).reshape(-1)
    n_spots = indptr.size - 1
    prod = data * g[indices]
    lens = np.diff(indptr)
    n_chunks = -(-lens // chunk)
    first = np.concatenate([[0], np.cumsum(n_chunks)])
    ccol = np.repeat(np.arange(n_spots, dtype=np.int64), n_chunks)
    cnum = np.arange(ccol.size, dtype=np.int64) - first[ccol]          # the chunk's number within its column
    cstart = indptr[ccol] + cnum * chunk
    clen = np.minimum(cstart + chunk, indptr[ccol + 1]) - cstart
    partial = _butterfly(_strided_lane_sums(prod, cstart, clen, 64)) if ccol.size else np.zeros(0, dtype=np.float32)
    out = np.zeros(n_spots, dtype=np.float32)
    cols = np.flatnonzero(n_chunks)
    if cols.size:
        out[cols] = _butterfly(_strided_lane_sums(partial, first[cols], n_chunks[cols], 64))
    return out


def tree_bound(depth, scale):
    """(d + 1) u * scale, scale = sum |a| |x| in float64."""
    return (np.asarray(depth, dtype=np.float64) + 1.0) * U * np.asarray(scale, dtype=np.float64)


def apply_depth(row_len, G=16):
    """d of `apply` for rows of row_len entries."""
    n = np.asarray(row_len, dtype=np.int64)
    return -(-n // G) + int(np.log2(G))


def apply_t_depth(col_len, chunk=2048):
    """d of `apply_t` for columns of col_len entries."""
    n = np.asarray(col_len, dtype=np.int64)
    chunks = -(-n // chunk)
    return 32 + 6 + -(-chunks // 64) + 6
