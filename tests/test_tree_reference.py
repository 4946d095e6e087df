"""CPU tests of tests/tree_reference.py alone, on random CSC matrices: the restated trees stay within the tree-depth bound of a float64
product, give exactly the plain product for one-hot inputs, and equal a scalar loop written from the same prose."""
import numpy as np
import pytest

import tree_reference as T


def _random_csc(rng, n_rows, col_lens, signed=True):
    """Columns of the given lengths, rows ascending within a column, values spread over six decades."""
    indptr = np.concatenate([[0], np.cumsum(col_lens)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(n_rows, int(n), replace=False)) for n in col_lens] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    data = (10.0 ** rng.uniform(-9.0, -3.0, indices.size)).astype(np.float32)
    if signed:
        data *= np.where(rng.random(indices.size) < 0.5, np.float32(-1.0), np.float32(1.0))
    return indptr, indices, data


def _float64(indptr, indices, data, w, g, n_rows):
    col = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    a = data.astype(np.float64)
    pw, pg = a * w.astype(np.float64)[col], a * g.astype(np.float64)[indices]
    fwd = np.bincount(indices, weights=pw, minlength=n_rows)
    fwd_abs = np.bincount(indices, weights=np.abs(pw), minlength=n_rows)
    adj = np.bincount(col, weights=pg, minlength=indptr.size - 1)
    adj_abs = np.bincount(col, weights=np.abs(pg), minlength=indptr.size - 1)
    return fwd, fwd_abs, adj, adj_abs


# (rows, column lengths): short rows and columns; rows of several trips of 16 lanes (300 columns over 400 rows); a column of more
# than 64 chunks (64 * 2048 = 131 072 entries) whose chunk count is no multiple of 64 and whose last chunk is partial, next to
# columns of one partial chunk, exactly one chunk, one chunk and one entry, and none.
SHAPES = {
    "small": (97, [0, 1, 5, 16, 17, 33, 64, 65, 97, 0, 3]),
    "long_rows": (400, [200 + 7 * (j % 23) for j in range(300)]),
    "long_column": (150001, [140001, 100, 2048, 2049, 0, 70000, 4097]),
}


@pytest.fixture(scope="module", params=sorted(SHAPES))
def case(request):
    n_rows, lens = SHAPES[request.param]
    rng = np.random.default_rng(sorted(SHAPES).index(request.param) + 40)
    indptr, indices, data = _random_csc(rng, n_rows, lens)
    w = (100.0 * rng.random(len(lens))).astype(np.float32)
    g = (rng.random(n_rows) - 0.5).astype(np.float32)
    return request.param, n_rows, indptr, indices, data, w, g


def test_shapes_cross_the_thresholds():
    n_rows, lens = SHAPES["long_column"]
    chunks = -(-np.array(lens) // 2048)
    assert chunks.max() > 64 and chunks.max() % 64 != 0 and max(lens) % 2048 != 0 and max(lens) % 64 != 0
    n_rows, lens = SHAPES["long_rows"]
    assert min(lens) * len(lens) / n_rows > 128                       # the mean row is longer than two trips of a 64-lane sort


def test_within_the_tree_depth_bound_of_float64(case):
    name, n_rows, indptr, indices, data, w, g = case
    fwd, fwd_abs, adj, adj_abs = _float64(indptr, indices, data, w, g, n_rows)
    got = T.apply_tree(indptr, indices, data, w, n_rows=n_rows)
    assert got.dtype == np.float32 and got.shape == (n_rows,)
    bound = T.tree_bound(T.apply_depth(np.bincount(indices, minlength=n_rows)), fwd_abs)
    err = np.abs(got.astype(np.float64) - fwd)
    assert np.all(err <= bound), float(np.max(err[bound > 0] / bound[bound > 0]))
    got_t = T.apply_t_tree(indptr, indices, data, g)
    assert got_t.dtype == np.float32 and got_t.shape == (indptr.size - 1,)
    bound_t = T.tree_bound(T.apply_t_depth(np.diff(indptr)), adj_abs)
    err_t = np.abs(got_t.astype(np.float64) - adj)
    assert np.all(err_t <= bound_t), float(np.max(err_t[bound_t > 0] / bound_t[bound_t > 0]))
    assert np.abs(got).max() > 0 and np.abs(got_t).max() > 0
    # rows and columns without entries are +0.0
    assert not np.signbit(got[np.bincount(indices, minlength=n_rows) == 0]).any() and np.all(got[np.bincount(indices, minlength=n_rows) == 0] == 0)
    assert np.all(got_t[np.diff(indptr) == 0].view(np.uint32) == 0)


def test_depths():
    assert list(T.apply_depth([1, 16, 17, 129])) == [5, 5, 6, 13]
    assert list(T.apply_t_depth([1, 2048, 2049, 64 * 2048, 64 * 2048 + 1, 200000])) == [45, 45, 45, 45, 46, 46]
    # the point of it: for a column of 200 000 entries the bound is some 4000 times below the order-free gamma(n)
    n = 200000
    gamma = (n + 1) * T.U / (1 - (n + 1) * T.U)
    assert 4000 < gamma / float(T.tree_bound(T.apply_t_depth(n), 1.0)) < 4500


def test_one_hot_inputs_give_the_plain_product(case):
    name, n_rows, indptr, indices, data, w, g = case
    lens = np.diff(indptr)
    for j in {int(np.argmax(lens)), int(np.argmin(lens)), len(lens) - 1}:
        e = np.zeros(len(lens), dtype=np.float32)
        e[j] = 1.0
        want = np.zeros(n_rows, dtype=np.float32)
        want[indices[indptr[j]:indptr[j + 1]]] = data[indptr[j]:indptr[j + 1]]
        got = T.apply_tree(indptr, indices, data, e, n_rows=n_rows)
        assert np.array_equal(got.view(np.uint32), (want + np.float32(0.0)).view(np.uint32)), j   # (a sum from +0.0: -0 cannot occur)
    counts = np.bincount(indices, minlength=n_rows)
    col = np.repeat(np.arange(len(lens)), lens)
    for v in {int(np.argmax(counts)), int(np.flatnonzero(counts == counts[counts > 0].min())[0]), int(indices[-1])}:
        e = np.zeros(n_rows, dtype=np.float32)
        e[v] = 1.0
        want = np.zeros(len(lens), dtype=np.float32)
        hit = indices == v
        want[col[hit]] = data[hit]
        got = T.apply_t_tree(indptr, indices, data, e)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), v


def _wave(v):
    v = list(v)
    m = len(v) // 2
    while m >= 1:
        v = [np.float32(v[i] + v[i ^ m]) for i in range(len(v))]
        m //= 2
    return v[0]


def test_against_a_scalar_loop():
    """The vectorised helper against the prose once more, one float32 operation at a time (the two small shapes)."""
    for name in ("small", "long_rows"):
        n_rows, lens = SHAPES[name]
        lens = lens[:40]
        rng = np.random.default_rng(77)
        indptr, indices, data = _random_csc(rng, n_rows, lens)
        w = (100.0 * rng.random(len(lens))).astype(np.float32)
        g = (rng.random(n_rows) - 0.5).astype(np.float32)
        rows = [[] for _ in range(n_rows)]
        for j in range(len(lens)):                                    # ascending j: every row's list is in ascending column order
            for e in range(indptr[j], indptr[j + 1]):
                rows[indices[e]].append(np.float32(data[e] * w[j]))
        want = np.zeros(n_rows, dtype=np.float32)
        for r, ps in enumerate(rows):
            lanes = [np.float32(0.0)] * 16
            for i, p in enumerate(ps):
                lanes[i % 16] = np.float32(lanes[i % 16] + p)
            want[r] = _wave(lanes)
        assert np.array_equal(T.apply_tree(indptr, indices, data, w, n_rows=n_rows).view(np.uint32), want.view(np.uint32)), name
        chunk = 64 if name == "small" else 128                        # (several chunks per column at these lengths)
        want_t = np.zeros(len(lens), dtype=np.float32)
        for j in range(len(lens)):
            sums = []
            for a in range(indptr[j], indptr[j + 1], chunk):
                lanes = [np.float32(0.0)] * 64
                for i, e in enumerate(range(a, min(a + chunk, indptr[j + 1]))):
                    lanes[i % 64] = np.float32(lanes[i % 64] + np.float32(data[e] * g[indices[e]]))
                sums.append(_wave(lanes))
            lanes = [np.float32(0.0)] * 64
            for i, s in enumerate(sums):
                lanes[i % 64] = np.float32(lanes[i % 64] + s)
            want_t[j] = _wave(lanes)
        assert np.array_equal(T.apply_t_tree(indptr, indices, data, g, chunk=chunk).view(np.uint32), want_t.view(np.uint32)), name


def test_dropped_entries_are_seen():
    """What the order-free bound cannot see: 512 entries (a quarter of a chunk) missing from a column of 140 001 pass gamma(n)
    against float64 and fail both the bit comparison and the tree-depth bound."""
    n_rows, lens = SHAPES["long_column"]
    rng = np.random.default_rng(5)
    indptr, indices, data = _random_csc(rng, n_rows, lens, signed=False)
    g = rng.random(n_rows).astype(np.float32)
    full = T.apply_t_tree(indptr, indices, data, g)
    cut = data.copy()
    cut[10 * 2048:10 * 2048 + 512] = 0.0                               # the first quarter of column 0's eleventh chunk contributes nothing
    short = T.apply_t_tree(indptr, indices, cut, g)
    _, _, adj, adj_abs = _float64(indptr, indices, data, np.zeros(len(lens), dtype=np.float32), g, n_rows)
    n = lens[0]
    err = abs(float(short[0]) - adj[0])
    assert short[0] != full[0]
    assert err <= (n + 1) * T.U / (1 - (n + 1) * T.U) * adj_abs[0]
    assert err > float(T.tree_bound(T.apply_t_depth(n), adj_abs[0]))
