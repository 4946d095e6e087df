"""CPU checks of the numpy restatement of deformable dose warping (tests/warp_reference.py) against what the rule must do: a zero
field is the resampler, whole-voxel displacements shift, the field holds its edges, a NaN in the field puts out exactly the voxels
that read it, the transposed rule puts the quantised weights where they belong and agrees with the float64 operator (no GPU needed)."""
import numpy as np

import resample_reference as rr
import warp_reference as wr

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def volume(dims, seed=5):
    return (np.random.default_rng(seed).random((dims[2], dims[1], dims[0]), dtype=F) * F(70.0)).astype(F)


def test_zero_field_is_the_resampler():
    src = volume(wr.SRC_DIMS)
    w = wr.standard()._replace(dvf=np.zeros((3, 5, 7, 9), dtype=F))
    got, inside = wr.warp(src, w, wr.DST_DIMS, scale=0.75)
    want, want_inside = rr.resample(src, w.m, w.v, wr.DST_DIMS, scale=0.75)
    assert (bits(got) == bits(want)).all() and (inside == want_inside).all()
    # negative entries of k turn the zero displacement into -0.0, which changes nothing either
    got, _ = wr.warp(src, w._replace(k=-w.k), wr.DST_DIMS, scale=0.75)
    assert (bits(got) == bits(want)).all()


def test_whole_voxel_displacement_shifts():
    src = volume(wr.SRC_DIMS)
    dvf = np.zeros((3, 2, 2, 2), dtype=F)
    dvf[0], dvf[1], dvf[2] = 6.0, -4.0, 1.0                           # k = diag(0.5, 0.5, 2): 3, -2, 2 source voxels
    fm, fv = wr.spanning((2, 2, 2), wr.SRC_DIMS)
    w = wr.make(np.eye(3), np.zeros(3), fm, fv, np.diag([0.5, 0.5, 2.0]), dvf)
    got, inside = wr.warp(src, w, wr.SRC_DIMS)
    want = np.zeros_like(src)
    want[:-2, 2:, :-3] = src[2:, :-2, 3:]
    assert (bits(got) == bits(want)).all()
    assert inside[:-2, 2:, :-3].all() and not inside[-1].any() and not inside[:, 0].any() and not inside[:, :, -1].any()


def test_edge_hold_and_a_dimension_of_one():
    src = volume(wr.SRC_DIMS)
    m, v = rr.rotation_map()
    # a single node: the same displacement everywhere, whatever the map into the field says
    one = np.array([1.5, -0.75, 0.25], dtype=F).reshape(3, 1, 1, 1)
    far = wr.make(m, v, np.diag([3.0, -2.0, 0.5]), (-7.0, 40.0, 2.0), wr.K, one)
    got, _ = wr.warp(src, far, wr.DST_DIMS)
    shift = (wr.K.astype(F).astype(np.float64) @ one.reshape(3).astype(np.float64))
    u, known = wr.displacement(far, wr.DST_DIMS)
    assert known.all() and all((u[c] == one[c, 0, 0, 0]).all() for c in range(3))
    p = wr.positions(far, wr.DST_DIMS)
    assert all(np.allclose(p[a], rr.positions(m, v, wr.DST_DIMS)[a] + shift[a], rtol=0, atol=1e-5) for a in range(3))
    assert got.max() > 0
    # a field that covers the destination's voxels 10..20 in x only: to the left of it the column at node 0, to the right the last one
    rng = np.random.default_rng(8)
    dvf = rng.uniform(-3, 3, (3, 1, 1, 6)).astype(F)
    w = wr.make(m, v, np.diag([0.5, 0.0, 0.0]), (-5.0, 0.0, 0.0), wr.K, dvf)
    u, _ = wr.displacement(w, wr.DST_DIMS)
    for c in range(3):
        assert (u[c][:, :, :11] == dvf[c, 0, 0, 0]).all() and (u[c][:, :, 20:] == dvf[c, 0, 0, 5]).all()
        assert (u[c][:, :, 12] == dvf[c, 0, 0, 1]).all() and (u[c][:, :, 13] != dvf[c, 0, 0, 1]).all()


def test_nan_in_the_field_puts_out_the_voxels_that_read_it():
    src = volume(wr.SRC_DIMS) + F(1.0)
    w = wr.standard(amplitude=0.25)
    clean, inside = wr.warp(src, w, wr.DST_DIMS)
    dvf = w.dvf.copy()
    dvf[1, 2, 3, 4] = np.nan                                          # component 1 of node (x 4, y 3, z 2)
    got, now = wr.warp(src, w._replace(dvf=dvf), wr.DST_DIMS)
    # a voxel reads the node iff it lies strictly within one field cell of it (at distance 0 in an axis, only the lower node has weight
    # ... but the blend a + t * (b - a) reads b with t = 0 too: a NaN times zero is a NaN)
    q = rr.positions(w.fm, w.fv, wr.DST_DIMS)
    reads = np.ones(inside.shape, dtype=bool)
    for a, node in enumerate((4, 3, 2)):
        i0 = np.floor(q[a]).astype(np.int64)
        reads &= (i0 == node) | (np.minimum(i0 + 1, wr.DVF_DIMS[a] - 1) == node)
    assert 0 < (reads & inside).sum() < inside.sum()
    assert (now == (inside & ~reads)).all()
    assert (bits(got[~reads]) == bits(clean[~reads])).all() and (bits(got[reads]) == 0).all()


def test_standard_case_is_mostly_inside_but_not_all():
    m, v = rr.rotation_map()
    _, plain = rr.resample(volume(wr.SRC_DIMS), m, v, wr.DST_DIMS)
    assert abs(plain.mean() - 0.80) < 0.01
    _, inside = wr.warp(volume(wr.SRC_DIMS), wr.standard(), wr.DST_DIMS)
    assert 0.5 < inside.mean() < 0.9
    assert abs(inside.mean() - 0.72) < 0.04


def test_transposed_single_voxel():
    """One non-zero g voxel: the 8 weights, quantised as stated, on the 8 expected nodes."""
    w = wr.standard()
    p = wr.positions(w, wr.DST_DIMS)
    z, y, x = 4, 11, 25
    pos = [float(p[a][z, y, x]) for a in range(3)]
    assert all(0.0 < pos[a] < wr.SRC_DIMS[a] - 1 and pos[a] != np.floor(pos[a]) for a in range(3))     # a voxel with 8 nodes on the grid
    g = np.zeros((wr.DST_DIMS[2], wr.DST_DIMS[1], wr.DST_DIMS[0]), dtype=F)
    g[z, y, x] = F(-3.7)
    got = wr.warp_t(g, w, wr.SRC_DIMS, scale=2.0)
    sg = F(2.0) * F(-3.7)
    e = 3                                                             # 7.4 = 0.925 * 2^3
    assert wr.exponent(abs(sg)) == e
    want = np.zeros_like(got)
    i0 = [int(np.floor(q)) for q in pos]
    t = [F(q) - F(np.floor(q)) for q in pos]
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                c = F(F(F(sg * (t[0] if dx else F(1.0) - t[0])) * (t[1] if dy else F(1.0) - t[1])) * (t[2] if dz else F(1.0) - t[2]))
                n = int(np.rint(float(c) * 2.0 ** (30 - e)))
                want[i0[2] + dz, i0[1] + dy, i0[0] + dx] = F(n * 2.0 ** (e - 30))
    assert np.count_nonzero(want) == 8 and (bits(got) == bits(want)).all()
    # every weight is a multiple of the quantum 2^(e - 30)
    assert (np.rint(got.astype(np.float64) * 2.0 ** (30 - e)) == got.astype(np.float64) * 2.0 ** (30 - e)).all()


def test_transposed_against_the_exact_operator():
    rng = np.random.default_rng(12)
    for w, nodes in ((wr.standard(), None), (wr.collapsing(), 8)):
        g = rng.standard_normal((wr.DST_DIMS[2], wr.DST_DIMS[1], wr.DST_DIMS[0])).astype(F)
        scale = 0.3
        got = wr.warp_t(g, w, wr.SRC_DIMS, scale=scale).reshape(-1).astype(np.float64)
        A = wr.warp_exact(w, wr.SRC_DIMS, wr.DST_DIMS)
        sg = wr.scaled_gradient(g, scale).reshape(-1).astype(np.float64)
        want = A.T @ sg
        big = np.abs(sg).max()
        # per contribution: three rounded float32 weights 1 - t and three float32 products (6 * 2^-24 of |c|, relative) and the
        # quantisation (M * 2^-30); the sum of integers is exact; the result is rounded to float32 once
        bound = 6.01 * 2.0 ** -24 * (abs(A).T @ np.abs(sg)) + 2.0 ** -30 * big * A.counts() + 2.0 ** -24 * np.abs(want)
        err = np.abs(got - want)
        assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
        assert np.count_nonzero(got) == nodes if nodes else np.count_nonzero(got) > 1000
        if nodes:
            assert (A.counts()[A.counts() > 0] == A.shape[0]).all()   # every destination voxel contributes to each of the 8


def test_transposed_edges():
    w = wr.standard()
    shape = (wr.DST_DIMS[2], wr.DST_DIMS[1], wr.DST_DIMS[0])
    base = volume(wr.SRC_DIMS, seed=2)
    zero = np.zeros(shape, dtype=F)
    assert (bits(wr.warp_t(zero, w, wr.SRC_DIMS)) == 0).all()
    assert (bits(wr.warp_t(zero, w, wr.SRC_DIMS, accumulate=True, base=base)) == bits(base)).all()
    g = np.random.default_rng(1).standard_normal(shape).astype(F)
    plain = wr.warp_t(g, w, wr.SRC_DIMS)
    g2 = g.copy()
    g2[0, 0, 0], g2[3, 4, 5] = np.nan, np.inf                         # what is not finite counts as zero
    g3 = g.copy()
    g3[0, 0, 0], g3[3, 4, 5] = 0.0, 0.0
    assert (bits(wr.warp_t(g2, w, wr.SRC_DIMS)) == bits(wr.warp_t(g3, w, wr.SRC_DIMS))).all()
    acc = wr.warp_t(g, w, wr.SRC_DIMS, accumulate=True, base=base)
    assert (bits(acc) == bits((base + plain).astype(F))).all()
    # a denormal maximum: E comes from the leading bit
    assert wr.exponent(F(2.0 ** -149)) == -148 and wr.exponent(F(2.0 ** -126)) == -125 and wr.exponent(F(0.75)) == 0 and wr.exponent(F(1.0)) == 1
    tiny = np.full(shape, F(3 * 2.0 ** -149), dtype=F)
    out = wr.warp_t(tiny, w, wr.SRC_DIMS)
    assert np.isfinite(out).all() and out.max() > 0
