"""rtd_dose_warp and rtd_dose_warp_t on the device against the numpy restatement of the header's rules (tests/warp_reference.py).
Every comparison with the restatement is exact: floats bit for bit (as uint32). The only bound in this file is that of the adjoint
identity, which is derived in its test from the number of rounded operations and the quantum of the transposed rule."""
import ctypes as C

import numpy as np
import pytest

import resample_reference as rr
import warp_reference as wr
from gpu_support import bits, switches
from raytracedicom_amd import abi

pytestmark = pytest.mark.gpu

F = np.float32
SRC, DST = wr.SRC_DIMS, wr.DST_DIMS
LONG = (70, 6, 3)                                                     # x crosses a 64-lane block edge, the rows are no multiple of 4


@pytest.fixture(scope="module")
def eng(engine):
    with engine.Engine(0) as e:
        yield e


def shape_of(dims):
    return (dims[2], dims[1], dims[0])


_MADE = {}


def made(key, make):
    """make() once per key, read-only from then on."""
    if key not in _MADE:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _MADE[key] = v
    return _MADE[key]


def volume(dims=SRC, seed=5):
    return made(("volume", tuple(dims), seed), lambda: (np.random.default_rng(seed).random(shape_of(dims), dtype=F) * F(70.0)).astype(F))


def gradient(dims=DST, seed=6):
    return made(("gradient", tuple(dims), seed), lambda: np.random.default_rng(seed).standard_normal(shape_of(dims)).astype(F))


def standard():
    return made("standard", wr.standard)


def long_case():
    return made("long", lambda: wr.standard(dst_dims=LONG, seed=13))


def collapsing():
    return made("collapsing", wr.collapsing)


def pieces(w):
    """The restatement's warp as Engine.warp_dose takes it: (maps, dvf)."""
    return ((w.m, w.v), (w.fm, w.fv), w.k), w.dvf


def same(got, want, what=""):
    assert got.shape == want.shape
    diff = bits(got) != bits(want)
    assert not diff.any(), "%s: %d of %d voxels differ, first at %s: engine %r, restatement %r" % (
        what, diff.sum(), diff.size, np.argwhere(diff)[0], got[diff][0], want[diff][0])


def forward(eng, src, w, dst_dims, **options):
    """Engine.warp_dose against the restatement -> (result, inside)."""
    want, inside = wr.warp(src, w, dst_dims, **options)
    kw = dict(options)
    if kw.pop("accumulate", False):
        kw["accumulate"] = 1
    maps, dvf = pieces(w)
    got = eng.warp_dose(src, maps, dvf, dst_dims, **kw)
    same(got, want, "forward onto %s" % (dst_dims,))
    return got, inside


def transposed(eng, g, w, src_dims=SRC, **kw):
    """Engine.warp_dose_t against the restatement -> the result."""
    want = wr.warp_t(g, w, src_dims, kw.get("scale", 1.0), bool(kw.get("accumulate", 0)), kw.get("base"))
    maps, dvf = pieces(w)
    got = eng.warp_dose_t(g, maps, dvf, src_dims, **kw)
    same(got, want, "transposed onto %s" % (src_dims,))
    return got


# ---- 1. a zero field is the resampler ----

def test_zero_field_equals_the_resampler(eng):
    w = standard()._replace(dvf=np.zeros_like(standard().dvf))
    maps, dvf = pieces(w)
    got = eng.warp_dose(volume(), maps, dvf, DST, scale=0.75)
    assert eng.warp_kernel_ms() > 0.0
    want = eng.resample_dose(volume(), (w.m, w.v), DST, scale=0.75)
    same(got, want, "zero field")
    assert np.count_nonzero(got) > 5000


# ---- 2. forward against the restatement ----

def test_forward_standard(eng):
    got, inside = forward(eng, volume(), standard(), DST)
    assert 0.5 < inside.mean() < 0.9 and (bits(got[~inside]) == 0).all() and got[inside].min() >= 0 and np.count_nonzero(got) > 5000


def test_forward_across_a_block_edge(eng):
    got, inside = forward(eng, volume(), long_case(), LONG)
    assert inside[:, :, 64:].any() and (~inside).any()


@pytest.mark.parametrize("dvf_dims", ((1, 1, 1), (9, 1, 5)), ids=lambda d: "x".join(map(str, d)))
def test_forward_field_dimensions_of_one(eng, dvf_dims):
    w = wr.standard(dvf_dims=dvf_dims, seed=17)
    got, inside = forward(eng, volume(), w, DST)
    assert inside.any() and (~inside).any()


def test_forward_edge_hold(eng):
    """A field that covers the destination's voxels 10..20 x 4..12 x 2..4 only: beyond it, its edge values."""
    s = standard()
    w = s._replace(fm=np.diag([0.8, 0.75, 2.0]).astype(F), fv=np.array([-8.0, -3.0, -4.0], dtype=F))
    q = rr.positions(w.fm, w.fv, DST)
    assert all((q[a] < 0).any() and (q[a] > wr.DVF_DIMS[a] - 1).any() for a in range(3))
    forward(eng, volume(), w, DST)


def test_forward_nan_and_inf_in_the_field(eng):
    s = wr.standard(amplitude=0.5)
    dvf = s.dvf.copy()
    dvf[1, 2, 3, 4], dvf[0, 1, 5, 7], dvf[2, 3, 1, 1] = np.nan, np.inf, -np.inf
    clean, inside = wr.warp(volume(), s, DST)
    got, now = forward(eng, volume(), s._replace(dvf=dvf), DST)
    lost = inside & ~now
    assert 100 < lost.sum() < inside.sum() // 2 and (bits(got[lost]) == 0).all()
    assert (bits(got[now]) == bits(clean[now])).all()


def test_forward_integer_sources(eng):
    rng = np.random.default_rng(11)
    u16 = rng.integers(0, 2 ** 16, shape_of(SRC), dtype=np.uint16)
    forward(eng, u16, standard(), DST, src_scale=70.0 / 65535)
    u32 = rng.integers(0, 2 ** 32, shape_of(SRC), dtype=np.uint32)
    forward(eng, u32, standard(), DST, src_scale=1.6298e-08, scale=2.0)


def test_forward_scale_and_accumulate(eng):
    base = volume(DST, seed=21)
    got, inside = forward(eng, volume(), standard(), DST, scale=0.5, accumulate=True, dst=base)
    assert (bits(got[~inside]) == bits(base[~inside])).all() and (got[inside] != base[inside]).any()


# ---- 3. phases ----

def test_accumulate_phases(eng):
    ws = [standard(), wr.standard(seed=31), wr.standard(dvf_dims=(4, 3, 2), seed=32)]
    doses = [volume(), volume(seed=41), volume(seed=42)]
    weights = (0.5, 0.3, 0.2)
    want, _ = wr.warp(doses[0], ws[0], DST, scale=weights[0])
    for d, w, a in list(zip(doses, ws, weights))[1:]:
        want, _ = wr.warp(d, w, DST, scale=a, accumulate=True, dst=want)
    got = eng.accumulate_phases(doses, [pieces(w) for w in ws], weights, DST)
    same(got, want, "three phases")
    assert np.count_nonzero(got) > 5000


# ---- 4. transposed against the restatement ----

def test_transposed_standard(eng):
    got = transposed(eng, gradient(), standard(), scale=0.3)
    assert np.count_nonzero(got) > 2000
    ms = eng.warp_t_kernel_ms()
    assert len(ms) == 4 and all(t > 0.0 for t in ms)


def test_transposed_across_a_block_edge(eng):
    got = transposed(eng, gradient(LONG, seed=7), long_case())
    assert np.count_nonzero(got) > 200


def test_transposed_accumulate(eng):
    base = volume(SRC, seed=22)
    got = transposed(eng, gradient(), standard(), scale=-1.5, accumulate=1, base=base)
    assert (got != base).sum() > 2000


def test_transposed_special_values(eng):
    g = gradient().copy()
    g[:, ::3, :] = 0.0
    g[2] = -np.abs(g[2])
    g[0, 1, 1], g[4, 11, 25], g[5, 12, 26], g[6, 10, 20] = np.nan, np.inf, F(2.0 ** -140), F(-2.0 ** -149)
    got = transposed(eng, g, standard())
    assert np.isfinite(got).all() and np.count_nonzero(got) > 2000
    # a gradient of denormals only: the quantum follows the leading bit of the maximum
    tiny = (gradient() * F(2.0 ** -140)).astype(F)
    assert 0 < np.abs(tiny).max() < 2.0 ** -126
    got = transposed(eng, tiny, standard())
    assert np.count_nonzero(got) > 2000


def test_transposed_all_zero(eng):
    zero = np.zeros(shape_of(DST), dtype=F)
    zero[1, 2, 3] = np.nan                                            # (counts as zero)
    base = volume(SRC, seed=23)
    got = transposed(eng, zero, standard(), accumulate=1, base=base)
    assert (bits(got) == bits(base)).all()
    maps, dvf = pieces(standard())
    got = eng.warp_dose_t(zero, maps, dvf, SRC, base=np.full(shape_of(SRC), F(-7.25)))      # written over, not added to
    assert (bits(got) == 0).all()


def test_transposed_contention(eng):
    """Every destination voxel lands in one source cell: 10 350 contributions on each of 8 nodes. A lost or doubled atomic shows."""
    w = collapsing()
    A = made("collapsing exact", lambda: wr.warp_exact(w, SRC, DST))
    assert (A.counts()[A.counts() > 0] == 50 * 23 * 9).all() and np.count_nonzero(A.counts()) == 8
    got = transposed(eng, gradient(), w)
    assert np.count_nonzero(got) == 8
    got = transposed(eng, np.abs(gradient()), w, scale=2.0)
    assert np.count_nonzero(got) == 8 and got.sum() > 10000


def test_transposed_with_plain_atomics(eng, engine):
    """The scatter with eight global atomics per voxel (RTD_WARP_T_PLAIN when the handle is made) gives the bits of the one that merges in
    an LDS tile first."""
    with switches(RTD_WARP_T_PLAIN="1"):
        with engine.Engine(0) as plain:
            for g, w, dims in ((gradient(), standard(), SRC), (gradient(), collapsing(), SRC), (gradient(LONG, seed=7), long_case(), SRC)):
                maps, dvf = pieces(w)
                same(plain.warp_dose_t(g, maps, dvf, dims), eng.warp_dose_t(g, maps, dvf, dims), "plain scatter")
                transposed(plain, g, w)


def test_transposed_identity_map_stays_in_the_tile(eng):
    """An identity map with a sub-voxel field: the contributions of a block fall into its LDS tile, the case the tile is for."""
    w = wr.make(np.eye(3), np.zeros(3), *wr.spanning(wr.DVF_DIMS, LONG), wr.K, wr.random_field(wr.DVF_DIMS, amplitude=0.4, seed=19))
    p = wr.positions(w, LONG)
    assert (np.diff(np.floor(p[0]), axis=2) == 1).mean() > 0.9
    got = transposed(eng, gradient(LONG, seed=7), w, src_dims=LONG)
    assert np.count_nonzero(got) > 1000


def test_transposed_flipped_map(eng):
    """x and z run backwards: the tile lies below the block's first voxel, not above it."""
    flip = (np.diag([-1.0, 1.0, -1.0]), np.array([LONG[0] - 1.0, 0.0, LONG[2] - 1.0]))
    w = wr.make(*flip, *wr.spanning(wr.DVF_DIMS, LONG), wr.K, wr.random_field(wr.DVF_DIMS, amplitude=0.4, seed=23))
    got = transposed(eng, gradient(LONG, seed=7), w, src_dims=LONG)
    assert np.count_nonzero(got) > 1000


@pytest.mark.parametrize("dst_dims, scale", (((2, 1, 262149), (0.5, 0.3, 3.8e-5)), ((2, 262149, 1), (0.5, 6e-5, 0.3))), ids=("slices", "rows"))
def test_more_rows_and_slices_than_a_grid_dimension_holds(eng, dst_dims, scale):
    """Beyond 65535 slices (4 x 65535 for the tile scatter, which takes four at a time) or 4 x 65535 rows, the blocks of the forward
    kernel and of the scatter walk the rest in strides."""
    w = wr.make(np.diag(scale), (0.25, 0.3, 0.5), *wr.spanning((2, 2, 2), dst_dims), wr.K, wr.random_field((2, 2, 2), amplitude=0.4, seed=29))
    got, inside = forward(eng, volume(), w, dst_dims)
    assert inside.all() and got[-1, -1, -1] > 0
    g = gradient(dst_dims, seed=8)
    back = transposed(eng, g, w)
    assert np.count_nonzero(back) > 20                                # (compared bit for bit above: a walk that stops early shows)


# ---- 5. determinism ----

def test_two_calls_give_equal_bits(eng):
    maps, dvf = pieces(standard())
    a, b = (eng.warp_dose(volume(), maps, dvf, DST) for _ in range(2))
    assert a.tobytes() == b.tobytes()
    a, b = (eng.warp_dose_t(gradient(), maps, dvf, SRC) for _ in range(2))
    assert a.tobytes() == b.tobytes()


def test_both_directions_are_hipgraph_capturable(engine):
    """Both calls only launch on the handle's stream: captured into one graph (a single chain) on a caller's stream and replayed twice,
    they give the bits of the restatement; a captured call is not timed."""
    import torch
    w = standard()
    dev = torch.device("cuda:0")
    with engine.Engine(0) as e:
        src, g, dvf = (torch.from_numpy(np.array(a)).to(dev) for a in (volume(), gradient(), w.dvf))
        out = torch.full(shape_of(DST), float("nan"), dtype=torch.float32, device=dev)
        back = torch.full(shape_of(SRC), float("nan"), dtype=torch.float32, device=dev)
        nws = e.warp_t_workspace_bytes(SRC)
        ws = torch.full((nws,), 0xff, dtype=torch.uint8, device=dev)  # (what the workspace holds on entry is irrelevant)
        warp = abi.make_warp((w.m, w.v), (w.fm, w.fv), w.k, dvf.data_ptr(), wr.DVF_DIMS)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        e.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                e.warp_dose_device(src.data_ptr(), SRC, warp, out.data_ptr(), DST, scale=0.75)
                e.warp_dose_t_device(g.data_ptr(), DST, warp, back.data_ptr(), SRC, ws.data_ptr(), nws, scale=0.3)
            for _ in range(2):
                graph.replay()
        torch.cuda.synchronize()
        for call in (e.warp_kernel_ms, e.warp_t_kernel_ms):
            with pytest.raises(engine.RtdError) as ei:
                call()
            assert ei.value.status == abi.RTD_ERR_NOT_READY
        e.set_stream(None)
        same(out.cpu().numpy(), wr.warp(volume(), w, DST, scale=0.75)[0], "captured forward")
        same(back.cpu().numpy(), wr.warp_t(gradient(), w, SRC, 0.3), "captured transposed")


# ---- 6. the adjoint identity ----

def test_adjoint_identity(eng):
    """|<W x, y> - <x, W^T y>| <= 64 * 2^-24 * sum |W| |x| |y| + 2^-30 * M * sum_j cnt_j |x_j|, in float64 from the device results. The
    first term covers the at most 21 + 4 + 1 rounded float32 operations of the two rules (7 blends of three, against three weights,
    three products and the final rounding), the second the quantisation of each contribution by at most M * 2^-30."""
    w = standard()
    maps, dvf = pieces(w)
    x = np.random.default_rng(51).standard_normal(shape_of(SRC)).astype(F)
    y = gradient()
    wx = eng.warp_dose(x, maps, dvf, DST).astype(np.float64).reshape(-1)
    wty = eng.warp_dose_t(y, maps, dvf, SRC).astype(np.float64).reshape(-1)
    x64, y64 = x.astype(np.float64).reshape(-1), y.astype(np.float64).reshape(-1)
    A = wr.warp_exact(w, SRC, DST)
    lhs, rhs = float(np.dot(wx, y64)), float(np.dot(x64, wty))
    bound = 64 * 2.0 ** -24 * float(np.dot(abs(A) @ np.abs(x64), np.abs(y64))) + 2.0 ** -30 * float(np.abs(y64).max()) * float(np.dot(A.counts(), np.abs(x64)))
    assert abs(lhs) > 1000 * bound                                    # (the two products are not both small: the identity says something)
    assert abs(lhs - rhs) <= bound, (lhs, rhs, abs(lhs - rhs), bound)


# ---- 7. refusals ----

def test_refusals_write_nothing(eng, engine):
    src, g = volume(), gradient()
    w = standard()
    pat_dst, pat_src = np.full(shape_of(DST), F(-3.5), dtype=F), np.full(shape_of(SRC), F(-4.5), dtype=F)
    nws = eng.warp_t_workspace_bytes(SRC)
    bufs = [eng.device_alloc(n) for n in (src.nbytes, w.dvf.nbytes, pat_dst.nbytes, g.nbytes, pat_src.nbytes, nws)]
    d_src, d_dvf, d_dst, d_g, d_gsrc, d_ws = bufs

    def warp_with(**kw):
        r = abi.make_warp((w.m, w.v), (w.fm, w.fv), w.k, kw.pop("dvf", d_dvf), kw.pop("dvf_dims", wr.DVF_DIMS))
        for name, (i, val) in kw.items():
            if name in ("m", "v"):
                getattr(getattr(r, i), name)[val[0]] = val[1]
            elif name == "k":
                r.disp_to_src_idx[i] = val
            elif name == "reserved":
                r.reserved[i] = val
            else:
                r.reserved0 = val
        return r

    def opt_with(**kw):
        o = abi.default_resample_options()
        for k, val in kw.items():
            if k == "reserved":
                o.reserved[1] = val
            else:
                setattr(o, k, val)
        return o
    good = warp_with()
    bad_warps = {
        "null warp": None,
        "null dev_dvf": warp_with(dvf=None),
        "zero field dimension": warp_with(dvf_dims=(9, 0, 5)),
        "nan in the source map": warp_with(m=("dst_idx_to_src_idx", (4, float("nan")))),
        "inf in the source offset": warp_with(v=("dst_idx_to_src_idx", (1, float("inf")))),
        "nan in the field map": warp_with(m=("dst_idx_to_dvf_idx", (0, float("nan")))),
        "inf in the field offset": warp_with(v=("dst_idx_to_dvf_idx", (2, float("-inf")))),
        "nan in k": warp_with(k=(5, float("nan"))),
        "inf in k": warp_with(k=(0, float("inf"))),
        "reserved0 of the warp": warp_with(reserved0=(0, 1)),
        "a reserved word of the warp": warp_with(reserved=(4, 1)),
    }
    fwd = {what: dict(warp=r) for what, r in bad_warps.items()}
    fwd.update({
        "null source": dict(src=None),
        "null destination": dict(dst=None),
        "zero source dimension": dict(src_dims=(37, 0, 11)),
        "zero destination dimension": dict(dst_dims=(0, 23, 9)),
        "too many source voxels": dict(src_dims=(2 ** 16, 2 ** 15, 1)),
        "too many destination voxels": dict(dst_dims=(2 ** 11, 2 ** 10, 2 ** 10)),
        "unknown src_type": dict(opt=opt_with(src_type=3)),
        "accumulate 2": dict(opt=opt_with(accumulate=2)),
        "infinite scale": dict(opt=opt_with(scale=float("inf"))),
        "zero src_scale": dict(opt=opt_with(src_type=abi.RTD_DOSE_U16, src_scale=0.0)),
        "reserved0": dict(opt=opt_with(reserved0=1)),
        "reserved word": dict(opt=opt_with(reserved=1)),
    })
    back = {what: dict(warp=r) for what, r in bad_warps.items()}
    back.update({
        "null gradient": dict(g=None),
        "null result": dict(out=None),
        "null workspace": dict(ws=None),
        "zero source dimension": dict(src_dims=(37, 0, 11)),
        "zero destination dimension": dict(dst_dims=(0, 23, 9)),
        "too many source voxels": dict(src_dims=(2 ** 16, 2 ** 15, 1)),
        "nan scale": dict(scale=float("nan")),
        "infinite scale": dict(scale=float("inf")),
        "accumulate 2": dict(accumulate=2),
        "workspace one byte short": dict(ws_bytes=nws - 1),
        "no workspace bytes": dict(ws_bytes=0),
        "misaligned workspace": dict(ws=d_ws + 4),
    })
    try:
        for d, a in ((d_src, src), (d_dvf, w.dvf), (d_dst, pat_dst), (d_g, g), (d_gsrc, pat_src)):
            eng.to_device(d, a)
        for what, kw in fwd.items():
            with pytest.raises(engine.RtdError) as ei:
                eng.warp_dose_device(kw.get("src", d_src), kw.get("src_dims", SRC), kw.get("warp", good), kw.get("dst", d_dst), kw.get("dst_dims", DST),
                                     opt=kw.get("opt"))
            assert ei.value.status == abi.RTD_ERR_INVALID_ARG, what
        for what, kw in back.items():
            with pytest.raises(engine.RtdError) as ei:
                eng.warp_dose_t_device(kw.get("g", d_g), kw.get("dst_dims", DST), kw.get("warp", good), kw.get("out", d_gsrc), kw.get("src_dims", SRC),
                                       kw.get("ws", d_ws), kw.get("ws_bytes", nws), scale=kw.get("scale", 1.0), accumulate=kw.get("accumulate", 0))
            assert ei.value.status == abi.RTD_ERR_INVALID_ARG, what
        eng.sync()
        for d, pattern in ((d_dst, pat_dst), (d_gsrc, pat_src)):
            after = np.empty_like(pattern)
            eng.to_host(after, d)
            assert (bits(after) == bits(pattern)).all()
        # ... a null options record is refused by the C entry point itself
        L = engine.lib()
        assert L.rtd_dose_warp(eng._h, C.c_void_p(d_src), abi.uint3(SRC), C.byref(good), C.c_void_p(d_dst), abi.uint3(DST), None) == abi.RTD_ERR_INVALID_ARG
        # ... and the handle goes on working, in both directions, on the buffers of the refusals
        eng.warp_dose_device(d_src, SRC, good, d_dst, DST)
        eng.warp_dose_t_device(d_g, DST, good, d_gsrc, SRC, d_ws, nws)
        after_dst, after_src = np.empty_like(pat_dst), np.empty_like(pat_src)
        eng.to_host(after_dst, d_dst)
        eng.to_host(after_src, d_gsrc)
        same(after_dst, wr.warp(src, w, DST)[0], "after the refusals")
        same(after_src, wr.warp_t(g, w, SRC), "after the refusals, transposed")
    finally:
        eng.sync()
        for d in bufs:
            eng.device_free(d)


# ---- 8. the times ----

def test_kernel_times(eng, engine):
    with engine.Engine(0) as fresh:
        for call in (fresh.warp_kernel_ms, fresh.warp_t_kernel_ms):
            with pytest.raises(engine.RtdError) as ei:
                call()
            assert ei.value.status == abi.RTD_ERR_NOT_READY
        maps, dvf = pieces(standard())
        fresh.warp_dose(volume(), maps, dvf, DST)
        assert fresh.warp_kernel_ms() > 0.0
