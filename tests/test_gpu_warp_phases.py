"""rtd_dose_warp_sum and rtd_dose_warp_t_phases on the device against the numpy restatement (tests/fourd_reference.py) and against the
per-phase public calls run in the same test. Every comparison is exact: floats bit for bit (as uint32)."""
import ctypes as C

import numpy as np
import pytest

import fourd_reference as fr
import warp_reference as wr
from gpu_support import bits, switches
from raytracedicom_amd import abi

pytestmark = pytest.mark.gpu

F = np.float32
SRC, DST = wr.SRC_DIMS, wr.DST_DIMS
LONG = (70, 6, 3)                                                     # x crosses a 64-lane block edge, the rows are no multiple of 4
FIELD_DIMS = ((9, 7, 5), (4, 3, 2), (9, 1, 5), (1, 1, 1))            # the phases' fields differ in dims; two have a dimension of 1


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


def phases(n, dst_dims=DST):
    """n warps onto dst_dims whose fields cycle through FIELD_DIMS, with their sources and weights."""
    ws = [made(("phase", p, tuple(dst_dims)), lambda p=p: wr.standard(dvf_dims=FIELD_DIMS[p % 4], dst_dims=dst_dims, seed=30 + p)) for p in range(n)]
    weights = [F(1.0 / n) * F(1.0 + 0.1 * p) for p in range(n)]
    return ws, [volume(seed=40 + p) for p in range(n)], weights


def same(got, want, what=""):
    assert got.shape == want.shape
    diff = bits(got) != bits(want)
    assert not diff.any(), "%s: %d of %d voxels differ, first at %s: engine %r, expected %r" % (
        what, diff.sum(), diff.size, np.argwhere(diff)[0], got[diff][0], want[diff][0])


class Device:
    """The buffers of one test, freed at its end."""

    def __init__(self, eng):
        self.eng, self.bufs = eng, []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.eng.sync()
        for p in self.bufs:
            self.eng.device_free(p)

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.eng.device_alloc(a.nbytes)
        self.bufs.append(p)
        self.eng.to_device(p, a)
        return p

    def down(self, p, shape):
        out = np.empty(shape, dtype=F)
        self.eng.to_host(out, p)
        return out

    def records(self, ws):
        return [abi.make_warp((w.m, w.v), (w.fm, w.fv), w.k, self.up(w.dvf), (w.dvf.shape[3], w.dvf.shape[2], w.dvf.shape[1])) for w in ws]


def pattern(dims, value):
    return np.full(shape_of(dims), F(value), dtype=F)


def run_sum(eng, srcs, ws, weights, dst_dims, src_dims=SRC, repeat=1):
    """rtd_dose_warp_sum into a destination that held a pattern, and the sequence of rtd_dose_warp calls into another -> (fused, sequence)."""
    with Device(eng) as d:
        recs = d.records(ws)
        ptrs = [d.up(s) for s in srcs]
        d_a, d_b = d.up(pattern(dst_dims, -3.5)), d.up(pattern(dst_dims, -3.5))
        for _ in range(repeat):
            eng.warp_sum_device(ptrs, src_dims, recs, weights, d_a, dst_dims)
        for p, (ptr, rec, a) in enumerate(zip(ptrs, recs, weights)):
            eng.warp_dose_device(ptr, src_dims, rec, d_b, dst_dims, scale=a, accumulate=1 if p else 0)
        return d.down(d_a, shape_of(dst_dims)), d.down(d_b, shape_of(dst_dims))


def run_t(eng, g, ws, weights, src_dims=SRC, repeat=1):
    """rtd_dose_warp_t_phases into volumes that held a pattern (the workspace holds 0xff on entry), and rtd_dose_warp_t per phase
    -> ([fused_p], [sequence_p])."""
    dst_dims = (g.shape[2], g.shape[1], g.shape[0])
    n = len(ws)
    with Device(eng) as d:
        recs = d.records(ws)
        d_g = d.up(g)
        outs = [d.up(pattern(src_dims, -4.5)) for _ in range(n)]
        seqs = [d.up(pattern(src_dims, -4.5)) for _ in range(n)]
        nws, one = eng.warp_t_phases_workspace_bytes(src_dims, n), eng.warp_t_workspace_bytes(src_dims)
        d_ws, d_one = d.up(np.full(nws, 0xff, dtype=np.uint8)), d.up(np.full(one, 0xff, dtype=np.uint8))
        for _ in range(repeat):
            eng.warp_dose_t_phases_device(d_g, dst_dims, recs, weights, outs, src_dims, d_ws, nws)
        for rec, a, out in zip(recs, weights, seqs):
            eng.warp_dose_t_device(d_g, dst_dims, rec, out, src_dims, d_one, one, scale=a)
        return [d.down(p, shape_of(src_dims)) for p in outs], [d.down(p, shape_of(src_dims)) for p in seqs]


def check_sum(eng, srcs, ws, weights, dst_dims, what):
    want, inside = made(("sum", what), lambda: fr.warp_sum(srcs, ws, weights, dst_dims))
    fused, seq = run_sum(eng, srcs, ws, weights, dst_dims)
    same(fused, want, what + ": fused against the restatement")
    same(fused, seq, what + ": fused against the sequence of public calls")
    return fused, inside


def check_t(eng, g, ws, weights, what, src_dims=SRC):
    want = made(("t", what), lambda: fr.warp_t_phases(g, ws, weights, src_dims))
    fused, seq = run_t(eng, g, ws, weights, src_dims)
    for p in range(len(ws)):
        same(fused[p], want[p], "%s: phase %d against the restatement" % (what, p))
        same(fused[p], seq[p], "%s: phase %d against the public call" % (what, p))
    return fused


# ---- 1. phase counts on both shapes (16 fills the argument record); the fields differ in dims ----

@pytest.mark.parametrize("dst_dims", (DST, LONG), ids=("standard", "long"))
@pytest.mark.parametrize("n", (1, 2, 3, 16))
def test_phase_counts(eng, n, dst_dims):
    ws, srcs, weights = phases(n, dst_dims)
    fused, inside = check_sum(eng, srcs, ws, weights, dst_dims, "%d phases onto %s" % (n, dst_dims))
    assert np.count_nonzero(fused) > (5000 if dst_dims == DST else 300) and all(i.any() and not i.all() for i in inside)
    back = check_t(eng, gradient(dst_dims, seed=7), ws, weights, "%d phases from %s" % (n, dst_dims))
    assert all(np.count_nonzero(b) > 200 for b in back)


# ---- 2. who is inside ----

def test_a_nan_in_one_phases_field(eng):
    ws, srcs, weights = phases(3)
    dvf = wr.standard(amplitude=0.5, seed=31).dvf.copy()
    dvf[1, 2, 3, 4] = np.nan
    clean = wr.standard(amplitude=0.5, seed=31)
    ws = [ws[0], clean._replace(dvf=dvf), ws[2]]
    fused, inside = check_sum(eng, srcs, ws, weights, DST, "a NaN in phase 1's field")
    lost = wr.warp(srcs[1], clean, DST)[1] & ~inside[1]
    assert 100 < lost.sum() and (inside[0] & lost).any()             # (phase 1 alone is outside there)
    check_t(eng, gradient(), ws, weights, "a NaN in phase 1's field")


def test_phase_0_outside_where_phase_1_is_inside(eng):
    ws, srcs, _ = phases(2)
    ws = [ws[0]._replace(v=(ws[0].v + np.array([25.0, 0.0, 0.0], dtype=F)).astype(F)), ws[1]]
    src = volume().copy()
    src[:, :, :20] = 0.0                                              # (a zero times a negative weight: -0.0f, which a sum from 0.0f loses)
    fused, inside = check_sum(eng, [srcs[0], src], ws, [F(1.0), F(-1.0)], DST, "phase 0 outside")
    only = ~inside[0] & inside[1]
    alone = wr.warp(src, ws[1], DST, scale=-1.0)[0]
    assert only.sum() > 1000 and (inside[0] & inside[1]).any()
    assert (bits(alone[only]) == 0x80000000).sum() > 100 and (bits(fused[only]) != 0x80000000).all()


def test_negative_and_zero_weights(eng):
    ws, srcs, _ = phases(3)
    fused, _ = check_sum(eng, srcs, ws, [F(-1.0), F(0.0), F(0.5)], DST, "weights -1, 0, 0.5")
    assert (fused < 0).any() and (fused > 0).any()
    check_t(eng, gradient(), ws, [F(-1.0), F(0.0), F(0.5)], "weights -1, 0, 0.5")


# ---- 3. gradients ----

def test_special_values_in_the_gradient(eng):
    ws, _, weights = phases(3)
    g = gradient().copy()
    g[:, ::3, :] = 0.0
    g[2] = -np.abs(g[2])
    g[0, 1, 1], g[4, 11, 25], g[5, 12, 26], g[6, 10, 20] = np.nan, np.inf, F(2.0 ** -140), F(-2.0 ** -149)
    back = check_t(eng, g, ws, weights, "special values")
    assert all(np.isfinite(b).all() and np.count_nonzero(b) > 2000 for b in back[:2])
    tiny = (gradient() * F(2.0 ** -140)).astype(F)                    # denormals only: each phase's quantum follows the leading bit of its maximum
    assert 0 < np.abs(tiny).max() < 2.0 ** -126
    check_t(eng, tiny, ws, weights, "denormals")


def test_all_zero_gradient(eng):
    ws, _, weights = phases(3)
    zero = np.zeros(shape_of(DST), dtype=F)
    zero[1, 2, 3] = np.nan                                            # (counts as zero)
    back = check_t(eng, zero, ws, weights, "all zero")
    assert all((bits(b) == 0).all() for b in back)                    # +0.0f over the pattern, in every phase


def test_a_weight_that_overflows_the_largest_gradient_only(eng):
    """weights[0] * g is infinite for the largest g and finite for every other: phase 0's maximum is not float32(weights[0] * max |g|)."""
    ws, _, _ = phases(2)
    g = (gradient() * F(2.0e36)).astype(F).copy()
    g[3, 7, 20] = F(3.0e38)
    weights = [F(2.0), F(0.5)]
    with np.errstate(over="ignore"):
        naive = F(weights[0] * np.abs(g).max())
    m0 = fr.phase_maximum(g, weights[0])
    assert np.isinf(naive) and np.isfinite(m0) and m0 > 0 and fr.phase_maximum(g, weights[1]) == F(1.5e38)
    back = check_t(eng, g, ws, weights, "overflow in phase 0")
    assert all(np.isfinite(b).all() and np.count_nonzero(b) > 2000 for b in back)


def test_the_collapsing_field_in_one_phase_of_three(eng):
    ws, _, weights = phases(3)
    ws = [ws[0], made("collapsing", wr.collapsing), ws[2]]
    back = check_t(eng, gradient(), ws, weights, "collapsing in phase 1")
    assert np.count_nonzero(back[1]) == 8 and np.count_nonzero(back[0]) > 2000


def test_plain_atomics_against_the_tile(eng, engine):
    with switches(RTD_WARP_T_PLAIN="1"):
        with engine.Engine(0) as plain:
            for dims, n in ((DST, 3), (LONG, 2)):
                ws, _, weights = phases(n, dims)
                g = gradient(dims, seed=7)
                a = check_t(plain, g, ws, weights, "%d phases from %s" % (n, dims))
                b, _ = run_t(eng, g, ws, weights)
                for p in range(n):
                    same(a[p], b[p], "plain scatter, phase %d" % p)


# ---- 4. determinism, capture ----

def test_two_calls_give_equal_bits(eng):
    ws, srcs, weights = phases(3)
    once, _ = run_sum(eng, srcs, ws, weights, DST)
    twice, _ = run_sum(eng, srcs, ws, weights, DST, repeat=2)
    assert once.tobytes() == twice.tobytes()
    once, _ = run_t(eng, gradient(), ws, weights)
    twice, _ = run_t(eng, gradient(), ws, weights, repeat=2)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(once, twice))


def test_both_calls_are_hipgraph_capturable(engine):
    """Both calls only launch on the handle's stream: captured into one graph on a caller's stream and replayed twice, they give the
    bits of the restatement."""
    import torch
    ws, srcs, weights = phases(3)
    dev = torch.device("cuda:0")
    with engine.Engine(0) as e:
        t_src = [torch.from_numpy(np.array(a)).to(dev) for a in srcs]
        t_dvf = [torch.from_numpy(np.array(w.dvf)).to(dev) for w in ws]
        g = torch.from_numpy(np.array(gradient())).to(dev)
        out = torch.full(shape_of(DST), float("nan"), dtype=torch.float32, device=dev)
        backs = [torch.full(shape_of(SRC), float("nan"), dtype=torch.float32, device=dev) for _ in ws]
        nws = e.warp_t_phases_workspace_bytes(SRC, 3)
        wsp = torch.full((nws,), 0xff, dtype=torch.uint8, device=dev)
        recs = [abi.make_warp((w.m, w.v), (w.fm, w.fv), w.k, t.data_ptr(), (w.dvf.shape[3], w.dvf.shape[2], w.dvf.shape[1])) for w, t in zip(ws, t_dvf)]
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        e.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                e.warp_sum_device([t.data_ptr() for t in t_src], SRC, recs, weights, out.data_ptr(), DST)
                e.warp_dose_t_phases_device(g.data_ptr(), DST, recs, weights, [b.data_ptr() for b in backs], SRC, wsp.data_ptr(), nws)
            for _ in range(2):
                graph.replay()
        torch.cuda.synchronize()
        e.set_stream(None)
        same(out.cpu().numpy(), fr.warp_sum(srcs, ws, weights, DST)[0], "captured sum")
        for p, want in enumerate(fr.warp_t_phases(gradient(), ws, weights, SRC)):
            same(backs[p].cpu().numpy(), want, "captured transposed, phase %d" % p)


# ---- 5. the host conveniences ----

def test_host_volumes(eng):
    ws, srcs, weights = phases(3)
    pieces = [(((w.m, w.v), (w.fm, w.fv), w.k), w.dvf) for w in ws]
    same(eng.warp_sum(srcs, pieces, weights, DST), eng.accumulate_phases(srcs, pieces, weights, DST), "warp_sum against accumulate_phases")
    for got, want in zip(eng.warp_dose_t_phases(gradient(), pieces, weights, SRC), fr.warp_t_phases(gradient(), ws, weights, SRC)):
        same(got, want, "warp_dose_t_phases")


# ---- 6. refusals ----

def test_refusals_write_nothing(eng, engine):
    ws, srcs, weights = phases(2)
    g = gradient()
    with Device(eng) as d:
        recs = d.records(ws)
        ptrs = [d.up(s) for s in srcs]
        d_dst, d_g = d.up(pattern(DST, -3.5)), d.up(g)
        outs = [d.up(pattern(SRC, -4.5)) for _ in ws]
        nws = eng.warp_t_phases_workspace_bytes(SRC, 2)
        d_ws = d.up(np.zeros(nws, dtype=np.uint8))

        def bad_record(**kw):
            r = abi.make_warp((ws[1].m, ws[1].v), (ws[1].fm, ws[1].fv), ws[1].k, kw.get("dvf", recs[1].dev_dvf), kw.get("dvf_dims", FIELD_DIMS[1]))
            if "k" in kw:
                r.disp_to_src_idx[4] = kw["k"]
            if "m" in kw:
                r.dst_idx_to_src_idx.m[2] = kw["m"]
            if "reserved" in kw:
                r.reserved[2] = kw["reserved"]
            return r
        one_more = [recs[0]] * 17
        common = {
            "no phases": dict(recs=[], weights=[], vols=[]),
            "17 phases": dict(recs=one_more, weights=[F(0.1)] * 17, vols=None),
            "a null dev_dvf in phase 1": dict(recs=[recs[0], bad_record(dvf=None)]),
            "a zero field dimension in phase 1": dict(recs=[recs[0], bad_record(dvf_dims=(4, 0, 2))]),
            "a NaN in phase 1's k": dict(recs=[recs[0], bad_record(k=float("nan"))]),
            "an infinite map entry in phase 1": dict(recs=[recs[0], bad_record(m=float("inf"))]),
            "a reserved word in phase 1": dict(recs=[recs[0], bad_record(reserved=1)]),
            "a NaN weight": dict(weights=[F(0.5), F(np.nan)]),
            "an infinite weight": dict(weights=[F(np.inf), F(0.5)]),
            "a zero source dimension": dict(src_dims=(37, 0, 11)),
            "a zero destination dimension": dict(dst_dims=(0, 23, 9)),
            "too many source voxels": dict(src_dims=(2 ** 16, 2 ** 15, 1)),
        }
        fwd = dict(common)
        fwd.update({"a null source": dict(vols=[ptrs[0], None]), "a null destination": dict(dst=None)})
        back = dict(common)
        back.update({"a null output": dict(vols=[outs[0], None]), "a null gradient": dict(g=None), "a null workspace": dict(ws=None),
                     "a workspace one byte short": dict(ws_bytes=nws - 1), "a misaligned workspace": dict(ws=d_ws + 4)})
        for what, kw in fwd.items():
            r = kw.get("recs", recs)
            vols = kw.get("vols") or (ptrs * 9)[:len(r)]
            with pytest.raises(engine.RtdError) as ei:
                eng.warp_sum_device(vols, kw.get("src_dims", SRC), r, kw.get("weights", weights), kw.get("dst", d_dst), kw.get("dst_dims", DST))
            assert ei.value.status == abi.RTD_ERR_INVALID_ARG, what
        for what, kw in back.items():
            r = kw.get("recs", recs)
            vols = kw.get("vols") or (outs * 9)[:len(r)]
            with pytest.raises(engine.RtdError) as ei:
                eng.warp_dose_t_phases_device(kw.get("g", d_g), kw.get("dst_dims", DST), r, kw.get("weights", weights), vols, kw.get("src_dims", SRC),
                                              kw.get("ws", d_ws), kw.get("ws_bytes", nws))
            assert ei.value.status == abi.RTD_ERR_INVALID_ARG, what
        # ... null arrays are refused by the C entry points themselves
        L = engine.lib()
        arr, wa = (C.c_void_p * 2)(*ptrs), (abi.RtdWarp * 2)(*recs)
        wt = np.array(weights, dtype=F)
        for a, b, c in ((None, wa, abi.fptr(wt)), (arr, None, abi.fptr(wt)), (arr, wa, None)):
            assert L.rtd_dose_warp_sum(eng._h, a, abi.uint3(SRC), b, c, 2, C.c_void_p(d_dst), abi.uint3(DST)) == abi.RTD_ERR_INVALID_ARG
        eng.sync()
        assert (bits(d.down(d_dst, shape_of(DST))) == bits(pattern(DST, -3.5))).all()
        for o in outs:
            assert (bits(d.down(o, shape_of(SRC))) == bits(pattern(SRC, -4.5))).all()
        # ... and the handle goes on working on the buffers of the refusals
        eng.warp_sum_device(ptrs, SRC, recs, weights, d_dst, DST)
        same(d.down(d_dst, shape_of(DST)), fr.warp_sum(srcs, ws, weights, DST)[0], "after the refusals")
