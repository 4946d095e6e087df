"""rtd_dose_resample and rtd_dose_quantize on the device against the numpy restatement of the header's rule
(tests/resample_reference.py). Every comparison is exact: floats bit for bit (as uint32), integers and counts as integers. There are no
tolerances in this file."""
import ctypes as C

import numpy as np
import pytest

import resample_reference as rr
from gpu_support import bits
from raytracedicom_amd import abi

pytestmark = pytest.mark.gpu

F = np.float32
DIMS = (37, 19, 11)                                                   # (x, y, z) of the usual source


@pytest.fixture(scope="module")
def eng(engine):
    with engine.Engine(0) as e:
        yield e


def shape_of(dims):
    return (dims[2], dims[1], dims[0])


_VOLUMES = {}


def volume(dims=DIMS, seed=5):
    """A random dose in [0, 70) on dims (x, y, z): made once, never modified."""
    key = (tuple(dims), seed)
    if key not in _VOLUMES:
        v = (np.random.default_rng(seed).random(shape_of(dims), dtype=F) * F(70.0)).astype(F)
        v.setflags(write=False)
        _VOLUMES[key] = v
    return _VOLUMES[key]


def same(got, want, what=""):
    diff = bits(got) != bits(want)
    assert got.shape == want.shape
    assert not diff.any(), "%s: %d of %d voxels differ, first at %s: engine %r, restatement %r" % (
        what, diff.sum(), diff.size, np.argwhere(diff)[0], got[diff][0], want[diff][0])


def check(eng, src, m, v, dst_dims, **options):
    """Engine.resample_dose against the restatement -> (result, inside)."""
    want, inside = rr.resample(src, m, v, dst_dims, **options)
    kw = dict(options)
    if kw.pop("accumulate", False):
        kw["accumulate"] = 1
    got = eng.resample_dose(src, (m, v), dst_dims, **kw)
    same(got, want, "m %s v %s onto %s" % (np.asarray(m).tolist(), np.asarray(v).tolist(), (dst_dims,)))
    return got, inside


# ---- A. the rule ----

def test_identity(eng):
    got, inside = check(eng, volume(), *rr.identity(), DIMS)
    assert inside.all() and (bits(got) == bits(volume())).all()
    assert eng.resample_kernel_ms() > 0.0


def test_upsampling(eng):
    """Voxels outside on the low side, fading borders on the high side."""
    got, inside = check(eng, volume((13, 9, 7)), np.diag([0.26, 0.4, 0.75]), (-0.3, 0.2, -1.5), (50, 23, 9))
    assert 0 < (~inside).sum() < inside.size and (bits(got[~inside]) == 0).all()
    p = rr.positions(np.diag([0.26, 0.4, 0.75]), (-0.3, 0.2, -1.5), (50, 23, 9))
    assert (p[0] > 12).any() and (p[2] < 0).any()                     # the upper border and the lower one are both visited


def test_downsampling(eng):
    got, inside = check(eng, volume(), np.diag([1.7, 2.3, 1.1]), (0.35, 0.6, 0.15), (21, 8, 10))
    assert inside.all() and got.min() > 0


def test_flip_and_permutation_are_exact_copies(eng):
    src = volume()
    got, _ = check(eng, src, np.diag([1.0, 1.0, -1.0]), (0.0, 0.0, 10.0), DIMS)
    assert (bits(got) == bits(src[::-1])).all()
    swap = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    got, _ = check(eng, src, swap, np.zeros(3), (19, 37, 11))
    assert (bits(got) == bits(src.transpose(0, 2, 1))).all()


def test_rotation(eng):
    m, v = rr.rotation_map()
    got, inside = check(eng, volume(), m, v, (50, 23, 9))
    assert (~inside).sum() > 100 and inside.sum() > 3000


# ---- B. the edges of the kernel ----

@pytest.mark.parametrize("dst_dims", ((1, 7, 5), (2, 7, 5), (3, 7, 5), (5, 7, 5), (67, 7, 5), (1, 1, 1)), ids=lambda d: "x".join(map(str, d)))
def test_destination_widths(eng, dst_dims):
    check(eng, volume(), np.diag([0.53, 1.9, 1.6]), (0.4, 1.25, 0.5), dst_dims)


@pytest.mark.parametrize("dst_dims", ((2, 3, 70001), (2, 262149, 1)), ids=("slices", "rows"))
def test_more_rows_and_slices_than_a_grid_dimension_holds(eng, dst_dims):
    """Beyond 65535 slices, or 4 x 65535 rows, the kernel's blocks walk the rest in strides."""
    got, inside = check(eng, volume(), np.diag([0.5, 6e-5, 1.4e-4]), (0.25, 0.3, 0.5), dst_dims)
    assert inside.all() and got[-1, -1, -1] > 0


@pytest.mark.parametrize("pz", (0.0, 0.3))
def test_single_slice_source(eng, pz):
    got, inside = check(eng, volume((37, 19, 1)), np.diag([1.0, 1.0, 0.0]), (0.25, 0.5, pz), (30, 15, 3))
    assert inside.all() and got.max() > 0


def test_unaligned_view_between_sentinels(eng):
    """The destination starts one float past a 16-byte boundary inside a larger buffer; the 64 floats before and behind it keep their bits."""
    src = volume()
    dst_dims = (50, 23, 9)
    m, v = np.diag([0.7, 0.8, 1.2]), (0.1, 0.2, 0.3)
    want, _ = rr.resample(src, m, v, dst_dims)
    n, lead = want.size, 65                                           # hipMalloc aligns to at least 256 bytes: lead 64 is aligned, 65 is not
    host = np.full(lead + n + 64, np.float32(-7.25), dtype=F)
    d_src, d_buf = eng.device_alloc(src.nbytes), eng.device_alloc(host.nbytes)
    try:
        assert d_buf % 256 == 0
        eng.to_device(d_src, src)
        eng.to_device(d_buf, host)
        eng.resample_dose_device(d_src, DIMS, (m, v), d_buf + 4 * lead, dst_dims)
        eng.to_host(host, d_buf)
    finally:
        eng.sync()
        eng.device_free(d_src)
        eng.device_free(d_buf)
    same(host[lead:lead + n].reshape(want.shape), want, "view")
    assert (host[:lead] == F(-7.25)).all() and (host[lead + n:] == F(-7.25)).all()


def test_entirely_outside(eng):
    got, inside = check(eng, volume(), np.eye(3), (100.0, 0.0, 0.0), DIMS)
    assert not inside.any() and (bits(got) == 0).all()


def test_many_blocks(eng):
    src = volume((96, 80, 70), seed=9)
    got, inside = check(eng, src, np.diag([0.59, 0.62, 0.72]), (-1.4, -0.4, 0.3), (160, 128, 100))   # leaves the source below in x, above in z
    assert (~inside).any() and inside.sum() > 10 ** 6


def test_two_calls_give_equal_bits(eng):
    m, v = rr.rotation_map()
    a = eng.resample_dose(volume(), (m, v), (50, 23, 9))
    b = eng.resample_dose(volume(), (m, v), (50, 23, 9))
    assert a.tobytes() == b.tobytes()


# ---- C. options ----

def test_integer_sources(eng):
    rng = np.random.default_rng(11)
    m, v = rr.rotation_map()
    u16 = rng.integers(0, 2 ** 16, shape_of(DIMS), dtype=np.uint16)
    check(eng, u16, m, v, (50, 23, 9), src_scale=70.0 / 65535)
    u32 = rng.integers(0, 2 ** 32, shape_of(DIMS), dtype=np.uint32)
    assert (u32 > 2 ** 24).sum() > u32.size // 2                      # values a float32 cannot hold: the product is made in double
    got, _ = check(eng, u32, np.eye(3), np.zeros(3), DIMS, src_scale=1.6298e-08)
    assert (bits(got) == bits((u32.astype(np.float64) * 1.6298e-08).astype(F))).all()
    check(eng, u32, m, v, (50, 23, 9), src_scale=1.6298e-08, scale=2.0)


def test_scale_and_accumulate(eng):
    base = volume((50, 23, 9), seed=21)
    m, v = rr.rotation_map()
    want, inside = rr.resample(volume(), m, v, (50, 23, 9), scale=0.5, accumulate=True, dst=base)
    got = eng.resample_dose(volume(), (m, v), (50, 23, 9), scale=0.5, accumulate=1, dst=base)
    same(got, want, "accumulate")
    assert (~inside).sum() > 100 and (bits(got[~inside]) == bits(base[~inside])).all()
    assert (got[inside] != base[inside]).any()


def test_refusals_write_nothing(eng, engine):
    src, dst_dims = volume(), (50, 23, 9)
    pattern = np.full(shape_of(dst_dims), F(-3.5), dtype=F)
    d_src, d_dst = eng.device_alloc(src.nbytes), eng.device_alloc(pattern.nbytes)
    ident = abi.make_affine(np.eye(3), np.zeros(3))

    def affine_with(i, val):
        a = abi.make_affine(np.eye(3), np.zeros(3))
        if i < 9:
            a.m[i] = val
        else:
            a.v[i - 9] = val
        return a

    def opt_with(**kw):
        o = abi.default_resample_options()
        for k, val in kw.items():
            if k == "reserved":
                o.reserved[1] = val
            else:
                setattr(o, k, val)
        return o
    cases = {
        "null source": dict(src=None),
        "null destination": dict(dst=None),
        "zero source dimension": dict(src_dims=(37, 0, 11)),
        "zero destination dimension": dict(dst_dims=(0, 23, 9)),
        "too many source voxels": dict(src_dims=(2 ** 16, 2 ** 15, 1)),
        "too many destination voxels": dict(dst_dims=(2 ** 11, 2 ** 10, 2 ** 10)),
        "nan in the matrix": dict(affine=affine_with(4, float("nan"))),
        "inf in the offset": dict(affine=affine_with(10, float("inf"))),
        "unknown src_type": dict(opt=opt_with(src_type=3)),
        "infinite scale": dict(opt=opt_with(scale=float("inf"))),
        "nan scale": dict(opt=opt_with(scale=float("nan"))),
        "zero src_scale": dict(opt=opt_with(src_type=abi.RTD_DOSE_U16, src_scale=0.0)),
        "negative src_scale": dict(opt=opt_with(src_type=abi.RTD_DOSE_U32, src_scale=-1.0)),
        "nan src_scale": dict(opt=opt_with(src_type=abi.RTD_DOSE_U16, src_scale=float("nan"))),
        "reserved0": dict(opt=opt_with(reserved0=1)),
        "reserved word": dict(opt=opt_with(reserved=1)),
    }
    try:
        eng.to_device(d_src, src)
        eng.to_device(d_dst, pattern)
        for what, kw in cases.items():
            with pytest.raises(engine.RtdError) as ei:
                eng.resample_dose_device(kw.get("src", d_src), kw.get("src_dims", DIMS), kw.get("affine", ident), kw.get("dst", d_dst),
                                         kw.get("dst_dims", dst_dims), opt=kw.get("opt"))
            assert ei.value.status == abi.RTD_ERR_INVALID_ARG, what
        eng.sync()
        after = np.empty_like(pattern)
        eng.to_host(after, d_dst)
        assert (bits(after) == bits(pattern)).all()
        # ... a null affine or options record is refused by the C entry point itself
        L = engine.lib()
        assert L.rtd_dose_resample(eng._h, C.c_void_p(d_src), abi.uint3(DIMS), None, C.c_void_p(d_dst), abi.uint3(dst_dims),
                                   C.byref(abi.default_resample_options())) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_dose_resample(eng._h, C.c_void_p(d_src), abi.uint3(DIMS), C.byref(ident), C.c_void_p(d_dst), abi.uint3(dst_dims), None) == abi.RTD_ERR_INVALID_ARG
        # ... and the handle goes on working; an F32 source ignores src_scale
        eng.resample_dose_device(d_src, DIMS, ident, d_dst, dst_dims, opt=opt_with(src_scale=0.0))
        eng.to_host(after, d_dst)
        same(after, rr.resample(src, np.eye(3), np.zeros(3), dst_dims)[0], "after the refusals")
    finally:
        eng.sync()
        eng.device_free(d_src)
        eng.device_free(d_dst)


# ---- D. the quantiser ----

@pytest.mark.parametrize("nbits", (16, 32))
def test_quantiser(eng, nbits):
    d = volume()
    q, s, n = eng.quantize_dose(d, nbits)
    want_q, want_s, want_n = rr.quantize(d, nbits)
    assert s == want_s and n == want_n == 0 and q.dtype == want_q.dtype and (q == want_q).all()
    # all zero
    q, s, n = eng.quantize_dose(np.zeros_like(d), nbits)
    assert (s, n) == (1.0, 0) and not q.any()
    # two negative voxels and a NaN
    e = d.copy()
    e[0, 0, 0], e[3, 7, 20], e[10, 18, 36] = -1.0, -40.0, np.nan
    q, s, n = eng.quantize_dose(e, nbits)
    want_q, want_s, want_n = rr.quantize(e, nbits)
    assert n == 3 == want_n and s == want_s and (q == want_q).all()
    assert q[0, 0, 0] == 0 and q[3, 7, 20] == 0 and q[10, 18, 36] == 0
    # a caller's scaling is used as given, values above the range are clamped and counted
    given = 0.0123 if nbits == 16 else 1e-6
    q, s, n = eng.quantize_dose(e, nbits, scaling=given)
    want_q, want_s, want_n = rr.quantize(e, nbits, scaling=given)
    assert s == given == want_s and n == want_n and (q == want_q).all()
    q, s, n = eng.quantize_dose(d, 16, scaling=1e-4)                      # 70 / 1e-4 lies above 65535
    want_q, _, want_n = rr.quantize(d, 16, scaling=1e-4)
    assert n == want_n > 1000 and (q == want_q).all() and q.max() == 65535


def test_quantiser_refusals(eng, engine):
    for kw in (dict(bits=8), dict(scaling=-1.0), dict(scaling=float("nan")), dict(scaling=float("inf"))):
        with pytest.raises(engine.RtdError) as ei:
            eng.quantize_dose(volume(), **kw)
        assert ei.value.status == abi.RTD_ERR_INVALID_ARG, kw
