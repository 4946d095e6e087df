"""CPU checks of the restatement of the 4D block (tests/fourd_reference.py): the properties of the phase sum that follow from the
header's rule, and the adjoint identity of the pair over three phases (no GPU needed)."""
import numpy as np

import fourd_reference as fr
import warp_reference as wr

F = np.float32
SRC, DST = wr.SRC_DIMS, wr.DST_DIMS


def shape_of(dims):
    return (dims[2], dims[1], dims[0])


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def volume(dims, seed):
    return (np.random.default_rng(seed).random(shape_of(dims), dtype=F) * F(70.0)).astype(F)


def identity(dims, dvf_dims=(3, 2, 2)):
    return wr.make(np.eye(3), np.zeros(3), *wr.spanning(dvf_dims, dims), wr.K, np.zeros((3, dvf_dims[2], dvf_dims[1], dvf_dims[0]), dtype=F))


def outside(dims):
    """A warp that sends every destination voxel far beyond the source."""
    return identity(dims)._replace(v=np.array([1.0e6, 0.0, 0.0], dtype=F))


def test_one_identity_phase_is_a_copy():
    src = volume(DST, 5)
    got, inside = fr.warp_sum([src], [identity(DST)], [1.0], DST)
    assert inside[0].all() and (bits(got) == bits(src)).all()


def test_a_phase_that_is_outside_leaves_the_sum():
    srcs = [volume(SRC, 5), volume(SRC, 6), volume(SRC, 7)]
    ws = [wr.standard(), outside(DST), wr.standard(seed=31)]
    a = (0.5, 0.3, 0.2)
    got, inside = fr.warp_sum(srcs, ws, a, DST)
    assert not inside[1].any() and inside[0].any() and inside[2].any()
    want, _ = fr.warp_sum([srcs[0], srcs[2]], [ws[0], ws[2]], (a[0], a[2]), DST)
    assert (bits(got) == bits(want)).all() and np.count_nonzero(got) > 5000


def test_with_phase_0_outside_a_sum_starts_from_plus_zero():
    """d = 0.0f, then d + weights[1] * e_1: where e_1 is zero and the weight negative the product is -0.0f, and 0.0f + -0.0f is +0.0f —
    not the -0.0f a written call would leave."""
    src = volume(SRC, 5).copy()
    src[:, :, :20] = 0.0
    w = wr.standard()
    got, inside = fr.warp_sum([src, src], [outside(DST), w], (1.0, -1.0), DST)
    alone, _ = wr.warp(src, w, DST, scale=-1.0)
    zero = inside[1] & (alone == 0)
    assert zero.sum() > 500 and (bits(alone[zero]) == 0x80000000).all() and (bits(got[zero]) == 0).all()
    rest = inside[1] & ~zero
    assert rest.sum() > 500 and (bits(got[rest]) == bits(alone[rest])).all() and (bits(got[~inside[1]]) == 0).all()


def test_adjoint_identity_over_three_phases():
    """|<sum_p a_p W_p x_p, y> - sum_p <x_p, a_p W_p^T y>| is bounded by the sum over the phases of the bound of
    tests/test_gpu_warp.py::test_adjoint_identity — (64 + P - 1) * 2^-24 * a_p * sum |W_p| |x_p| |y| + 2^-30 * M_p * sum_j cnt_j |x_pj| — where
    64 covers the rounded float32 operations of one phase's two rules as there, P - 1 more roundings per voxel come from the accumulated
    sums (each at most 2^-24 of a partial sum, which the sum of the phases' absolute terms bounds), and M_p = max |a_p y| sets phase p's
    quantum."""
    ws = [wr.standard(), wr.standard(seed=31), wr.standard(dvf_dims=(4, 3, 2), seed=32)]
    a = [F(0.5), F(0.3), F(0.2)]
    P = len(ws)
    xs = [np.random.default_rng(51 + p).standard_normal(shape_of(SRC)).astype(F) for p in range(P)]
    y = np.random.default_rng(6).standard_normal(shape_of(DST)).astype(F)
    acc, _ = fr.warp_sum(xs, ws, a, DST)
    backs = fr.warp_t_phases(y, ws, a, SRC)
    y64 = y.astype(np.float64).reshape(-1)
    lhs = float(np.dot(acc.astype(np.float64).reshape(-1), y64))
    rhs = sum(float(np.dot(x.astype(np.float64).reshape(-1), b.astype(np.float64).reshape(-1))) for x, b in zip(xs, backs))
    bound = 0.0
    for p in range(P):
        A = wr.warp_exact(ws[p], SRC, DST)
        x64 = np.abs(xs[p].astype(np.float64).reshape(-1))
        bound += (64 + P - 1) * 2.0 ** -24 * float(a[p]) * float(np.dot(abs(A) @ x64, np.abs(y64)))
        bound += 2.0 ** -30 * float(fr.phase_maximum(y, a[p])) * float(np.dot(A.counts(), x64))
    assert abs(lhs) > 100 * bound, (lhs, bound)                       # (the identity says something)
    assert abs(lhs - rhs) <= bound, (lhs, rhs, abs(lhs - rhs), bound)


class Dense:
    """A dose-influence matrix [voxels][spots] with the two products Reference4D asks for."""

    def __init__(self, a):
        self.a = a

    def matvec(self, w):
        return self.a @ np.asarray(w, dtype=np.float64)

    def rmatvec(self, g):
        return self.a.T @ np.asarray(g, dtype=np.float64)


def test_the_restated_iteration_descends():
    """Two phases of two fields (6 and 5 spots, random non-negative columns on the 37 x 19 x 11 grid), the objective on the 50 x 23 x 9
    reference grid: five iterations of Reference4D keep a finite history whose minimum lies below its first value, and the first
    objective is the objective of the restated sum of the start weights."""
    import optimizer_reference as OR
    rng = np.random.default_rng(9)
    nsrc, ndst = int(np.prod(SRC)), int(np.prod(DST))
    sizes = (6, 5)
    mats = [[Dense(rng.random((nsrc, n)) * (rng.random((nsrc, n)) < 0.2)) for n in sizes] for _ in range(2)]
    ws, a = [wr.standard(), wr.standard(seed=31)], (0.6, 0.4)
    w0 = rng.random(sum(sizes)).astype(F) + F(0.5)
    obj = OR.ReferenceObjective(ndst)
    it = fr.Reference4D(mats, sizes, ws, a, SRC, DST, obj, w0)
    acc, _ = fr.warp_sum(it.phase_doses(w0), ws, a, DST)
    target = acc.reshape(-1) > 0.5 * acc.max()
    obj.add_roi(target)
    obj.add_term(OR.SQ_DEVIATION, 0, 1.0, 1.2 * float(acc.reshape(-1)[target].mean()))
    first = obj.eval(acc.reshape(-1))[0][0]
    hist = [it.step() for _ in range(5)]
    assert hist[0] == first and np.isfinite(hist).all() and min(hist) < hist[0], hist
    assert np.array_equal(fr.combine([np.array([1.0, -0.0], dtype=F)]).view(np.uint32), np.array([1.0, -0.0], dtype=F).view(np.uint32))   # one phase hands its bits through


def test_the_maximum_of_a_phase_is_not_the_weight_times_one_maximum():
    """weights[p] * g overflows for the largest g and stays finite for the next: the overflowed product counts as zero, so M_p comes
    from the next one."""
    g = np.zeros(shape_of(DST), dtype=F)
    g[1, 2, 3], g[2, 3, 4] = F(3.0e38), F(-1.0e38)
    a = F(2.0)
    with np.errstate(over="ignore"):
        naive = F(a * np.abs(g).max())
    assert np.isinf(naive) and fr.phase_maximum(g, a) == F(2.0e38)
    back = fr.warp_t_phases(g, [identity(DST)], [a], DST)[0]
    assert np.isfinite(back).all() and back[2, 3, 4] == F(-2.0e38) and back[1, 2, 3] == 0
