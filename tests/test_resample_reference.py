"""The numpy restatement of the resampling rule and of the RT Dose quantiser (tests/resample_reference.py) against what the rule must
give in closed form: exact copies under the identity, a flip and a permutation, an affine field reproduced through a rotated map, zeros
outside, and the quantiser's round trip within half a step (no GPU needed)."""
import numpy as np
import pytest

import resample_reference as rr

F = np.float32
SHAPE = (11, 19, 37)                                                  # [Z][Y][X]: 37 x 19 x 11
DIMS = (37, 19, 11)


def volume(seed=5):
    return (np.random.default_rng(seed).random(SHAPE, dtype=F) * F(70.0)).astype(F)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def test_identity_returns_the_source():
    src = volume()
    out, inside = rr.resample(src, *rr.identity(), DIMS)
    assert inside.all() and (bits(out) == bits(src)).all()


def test_flip_and_permutation_are_exact_copies():
    src = volume()
    out, inside = rr.resample(src, np.diag([1.0, 1.0, -1.0]), (0.0, 0.0, 10.0), DIMS)
    assert inside.all() and (bits(out) == bits(src[::-1])).all()
    swap = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    out, inside = rr.resample(src, swap, np.zeros(3), (19, 37, 11))
    assert inside.all() and (bits(out) == bits(src.transpose(0, 2, 1))).all()


def test_affine_field_through_a_rotation():
    """A trilinear blend reproduces an affine field where all 8 nodes exist. Seven float32 blends of values up to 25: 1e-6 of the
    maximum is several roundings of room (measured 1.6e-7 while the rule was drafted)."""
    z, y, x = np.meshgrid(np.arange(11.0), np.arange(19.0), np.arange(37.0), indexing="ij")
    src = (2.0 + 0.5 * x + 0.25 * y + 0.125 * z).astype(F)                  # (every value is exact in float32)
    m, v = rr.rotation_map()
    out, inside = rr.resample(src, m, v, (50, 23, 9))
    p = rr.positions(m, v, (50, 23, 9))
    whole = np.ones(inside.shape, dtype=bool)
    for a, n in enumerate(DIMS):
        whole &= (p[a] >= 0) & (p[a] <= n - 1)
    want = 2.0 + 0.5 * p[0].astype(np.float64) + 0.25 * p[1].astype(np.float64) + 0.125 * p[2].astype(np.float64)
    err = np.abs(out.astype(np.float64) - want)[whole].max() / float(src.max())
    print("%d voxels with all nodes inside, %d outside, relative error %.3g" % (whole.sum(), (~inside).sum(), err))
    assert whole.sum() > 3000 and (~inside).sum() > 100
    assert err <= 1e-6
    assert (bits(out[~inside]) == 0).all()                                 # exactly +0.0f


def test_borders_fade_and_outside_is_zero():
    """One source voxel of 8 at node (0, 0, 0): half a voxel before it gives 4 along x alone, a full voxel gives nothing."""
    src = np.zeros((3, 3, 3), dtype=F)
    src[0, 0, 0] = 8.0
    out, inside = rr.resample(src, np.eye(3), (-0.5, 0.0, 0.0), (3, 3, 3))
    assert inside.all() and out[0, 0, 0] == 4.0 and out[0, 0, 1] == 4.0 and out[0, 0, 2] == 0.0
    out, inside = rr.resample(src, np.eye(3), (-1.0, 0.0, 0.0), (3, 3, 3))
    assert not inside[:, :, 0].any() and inside[:, :, 1:].all() and out[0, 0, 1] == 8.0
    out, inside = rr.resample(src, np.eye(3), (np.nan, 0.0, 0.0), (3, 3, 3))
    assert not inside.any() and (bits(out) == 0).all()


def test_options():
    src = volume()
    raw = np.random.default_rng(6).integers(0, 2 ** 32, SHAPE, dtype=np.uint32)
    out, _ = rr.resample(raw, *rr.identity(), DIMS, src_scale=1e-7)
    assert (bits(out) == bits((raw.astype(np.float64) * 1e-7).astype(F))).all()
    base = volume(7)
    m, v = np.diag([1.0, 1.0, 1.0]), (20.5, 0.0, 0.0)
    out, inside = rr.resample(src, m, v, DIMS, scale=0.5, accumulate=True, dst=base)
    plain, _ = rr.resample(src, m, v, DIMS, scale=0.5)
    assert 0 < inside.sum() < inside.size
    assert (bits(out[~inside]) == bits(base[~inside])).all()
    assert (bits(out[inside]) == bits((base + plain).astype(F)[inside])).all()


@pytest.mark.parametrize("nbits", (16, 32))
def test_quantiser_round_trip(nbits):
    d = volume()
    q, s, n_clamped = rr.quantize(d, nbits)
    assert n_clamped == 0 and q.dtype == (np.uint16 if nbits == 16 else np.uint32)
    x = float(d.max()) / (2 ** nbits - 1)
    assert float("%.10g" % s) == s and len("%.10g" % s) <= 16             # the text a writer stores gives the same double back
    assert s == float("%.10g" % x) or (nbits == 32 and 0 < s / x - 1 < 1.1e-9)
    # float(q s) is the Python float, a double: half a step, and 2^-20 of it for the two float64 roundings (d / s and q s, 2^-53 each
    # of at most 2^32 steps). Rounded on to float32 the product moves by up to half a float32 spacing of d, which at 16 bits is 2^-8
    # of a step: no bound of this form holds for the float32.
    back = q.astype(np.float64) * s
    err = np.abs(back - d.astype(np.float64)).max()
    print("%d bits: scaling %r, largest error %.6g steps" % (nbits, s, err / s))
    assert err <= s / 2 * (1 + 2.0 ** -20)
    if nbits == 32:
        big = d >= 1.0                                                     # there a step lies far below the float32 spacing: the dose itself returns
        assert (back.astype(F)[big] == d[big]).all()
    assert int(q.max()) >= 2 ** nbits - 1 - (6 if nbits == 32 else 0)     # the largest dose sits at the top: ten digits are 1e-9 of 2^32 steps


def test_quantiser_edges():
    d = volume()
    d[0, 0, 0], d[1, 2, 3], d[4, 5, 6] = -1.0, -0.25, np.nan
    for nbits in (16, 32):
        q, s, n_clamped = rr.quantize(d, nbits)
        assert n_clamped == 3 and q[0, 0, 0] == 0 and q[1, 2, 3] == 0 and q[4, 5, 6] == 0
    q, s, n_clamped = rr.quantize(np.zeros(SHAPE, dtype=F), 16)
    assert (s, n_clamped) == (1.0, 0) and not q.any()
    q, s, n_clamped = rr.quantize(volume(), 16, scaling=1e-4)              # 70 / 1e-4 lies above 65535
    assert s == 1e-4 and n_clamped > 0 and q.max() == 65535
    assert rr.quantize(np.array([0.5, 1.5, 2.5], dtype=F), 16, scaling=1.0)[0].tolist() == [0, 2, 2]   # ties to even
