"""The gamma index on the device (rtd_dose_gamma) against the CPU oracle where the oracle applies (node samples, global, no mask)
and against the numpy restatement of the header's definition (tests/gamma_reference.py) everywhere else. Every comparison is exact:
counts as integers, gamma values bit for bit. There are no tolerances in this file."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gamma_child
import gamma_reference as gr
import gamma_scenes as gs
from conftest import ROOT
from gpu_support import bits
from raytracedicom_amd import abi, luts, scenarios

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def eng(engine):
    with engine.Engine(0) as e:
        yield e


_REFERENCE = {}


def reference(name, **opts):
    """The restatement's Result for a scene of gamma_scenes under the options of Engine.gamma: computed once, never modified."""
    key = (name,) + tuple(sorted(opts.items()))
    if key not in _REFERENCE:
        s = gs.by_name(name)
        ref, ev = gs.pair(s)
        o = dict(opts)
        mask = gamma_child.box_mask(ref.shape) if o.pop("box", False) else None
        res = gr.gamma(ref, ev, s.spacing, s.dd, s.dta, 0.10, mask=mask, **o)
        res.map.setflags(write=False)
        _REFERENCE[key] = res
    return _REFERENCE[key]


def device(eng, name, **opts):
    s = gs.by_name(name)
    ref, ev = gs.pair(s)
    o = dict(opts)
    mask = gamma_child.box_mask(ref.shape) if o.pop("box", False) else None
    return eng.gamma(ref, ev, s.spacing, s.dd, s.dta, 0.10, mask=mask, want_map=True, **o)


def same(got, want):
    """Engine.gamma's (rate, n, max_gamma, map) against a Result of the restatement."""
    rate, n, gmax, gmap = got
    print("engine: n_evaluated %d pass rate %.6f max_gamma %r; restatement: n_evaluated %d n_passed %d max_gamma %r"
          % (n, rate, gmax, want.n_evaluated, want.n_passed, float(want.max_gamma)))
    assert n == want.n_evaluated
    assert rate == (want.n_passed / want.n_evaluated if want.n_evaluated else 1.0)
    assert bits(F(gmax)) == bits(F(want.max_gamma)), (gmax, float(want.max_gamma))
    diff = bits(gmap) != bits(want.map)
    assert not diff.any(), "%d map voxels differ, first at %s: engine %r, restatement %r" % (
        diff.sum(), np.argwhere(diff)[0], gmap[diff][0], want.map[diff][0])


@pytest.mark.parametrize("s", gs.SCENES, ids=lambda s: s.name)
def test_oracle_parity(eng, orc, s):
    ref, ev = gs.pair(s)
    rate, n_eval, gmax = orc.gamma_pass_rate(ref, ev, s.spacing, s.dd, s.dta, 0.10)
    got = device(eng, s.name)
    assert got[1] == n_eval
    assert got[0] == rate                                             # (n_passed / n_evaluated in float64 on both sides)
    assert bits(F(got[2])) == bits(F(gmax)), (got[2], gmax)
    want = reference(s.name)
    same(got, want)
    assert ((got[3] == -1.0) == (ref < F(0.10) * ref.max())).all()
    assert eng.gamma_kernel_ms() > 0.0


@pytest.mark.parametrize("interp", (2, 4))
@pytest.mark.parametrize("name", ("iso2mm", "thin"))
def test_interpolation(eng, name, interp):
    same(device(eng, name, interp=interp), reference(name, interp=interp))


@pytest.mark.parametrize("opts", ({"local": True}, {"box": True}, {"norm_dose": 1.5}, {"interp": 2, "local": True, "box": True, "norm_dose": 1.5},
                                  {"search_mult": 1.0}),
                         ids=("local", "mask", "norm_dose", "all", "search_mult"))
def test_options(eng, opts):
    want = reference("aniso", **opts)
    assert 0 < want.n_passed < want.n_evaluated
    same(device(eng, "aniso", **opts), want)


def test_naive_path_gives_the_same_bits(eng, tmp_path):
    """The plain second implementation (RTD_GAMMA_NAIVE, read when a handle is created) in a child process, the brick kernel here."""
    out = str(tmp_path / "naive.npz")
    env = dict(os.environ, RTD_GAMMA_NAIVE="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gamma_child.py"), out], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "RTD_GAMMA_NAIVE" not in os.environ
    naive = np.load(out)
    for i, (name, opts) in enumerate(gamma_child.CASES):
        counts, gmap = gamma_child.run(eng, name, opts)
        assert counts[1] > 1000 and 0 < counts[0], counts
        assert (counts == naive["counts%d" % i]).all(), (name, opts, counts, naive["counts%d" % i])
        assert (bits(gmap) == bits(naive["map%d" % i])).all(), (name, opts)


# The brick is 32 x 4 x 4 (x, y, z): (31, 3, 3) is the last lane of the first brick, (32, 4, 4) the first lane of the brick diagonally
# behind it, (64, 8, 8) the far corner of the 65 x 9 x 9 grid and alone in its brick.
@pytest.mark.parametrize("hot, step", (((31, 3, 3), (1, 0, 0)), ((31, 3, 3), (0, 1, 0)), ((31, 3, 3), (0, 0, 1)),
                                       ((32, 4, 4), (-1, 0, 0)), ((32, 4, 4), (0, -1, 0)), ((32, 4, 4), (0, 0, -1)),
                                       ((64, 8, 8), (-1, -1, -1))),
                         ids=("+x", "+y", "+z", "-x", "-y", "-z", "corner"))
@pytest.mark.parametrize("interp", (1, 2))
def test_halo(eng, hot, step, interp):
    """One hot reference voxel at the edge of a brick; the only evaluated dose that matches it lies a full search radius away, in the
    neighbouring brick: found through the halo or not at all."""
    sp, dta = (1.0, 2.0, 1.5), 3.0
    r = gr.radii(sp, dta)
    assert r == [5, 3, 3]
    ref = np.zeros((9, 9, 65), dtype=F)
    ev = np.zeros_like(ref)
    ref[hot[2], hot[1], hot[0]] = 1.0
    at = [hot[a] + step[a] * r[a] for a in range(3)]
    ev[at[2], at[1], at[0]] = 1.0
    want = gr.gamma(ref, ev, sp, 0.02, dta, 0.10, interp=interp)
    # the match is exact, so gamma is the distance to it over dta: far below the 1 / 0.02 of the voxel's own node
    dist = F(np.sqrt(sum((step[a] * r[a] * sp[a]) ** 2 for a in range(3))))
    assert want.n_evaluated == 1 and abs(float(want.max_gamma) - float(dist) / dta) < 1e-5, (float(want.max_gamma), dist)
    same(eng.gamma(ref, ev, sp, 0.02, dta, 0.10, interp=interp, want_map=True), want)


def test_water_cube_pair(eng, engine, orc):
    """The field of smoke(): the engine's dose against the oracle's. All-pass, which is the point of this case."""
    es = luts.synth_luts()
    scn = scenarios.water_cube(es, n=64, n_layers=1, spots=9, pitch=5.0)
    ref = orc.compute(scn)
    dose = np.zeros_like(scn.ct)
    with engine.Engine(0) as e2:
        e2.set_luts(es)
        e2.set_ct(scn.ct)
        e2.compute(scn.beams, dose)
    want = orc.gamma_pass_rate(ref, dose, scn.spacing)
    got = eng.gamma(ref, dose, scn.spacing)
    assert want[0] == 1.0 and want[1] > 0
    assert (got[0], got[1]) == (want[0], want[1]) and bits(F(got[2])) == bits(F(want[2])), (got, want)


class Buffers:
    """Two small device volumes and a result record pre-filled with a pattern."""

    def __init__(self, eng, shape=(6, 7, 9)):
        self.eng, self.shape = eng, shape
        self.dims = (shape[2], shape[1], shape[0])
        rng = np.random.default_rng(3)
        self.ref = rng.random(shape, dtype=F) + F(0.5)
        self.ev = (self.ref * (1 + 0.05 * rng.standard_normal(shape))).astype(F)
        self.d_ref, self.d_ev = eng.device_alloc(self.ref.nbytes), eng.device_alloc(self.ref.nbytes)
        self.d_map, self.d_res = eng.device_alloc(self.ref.nbytes), eng.device_alloc(32)
        eng.to_device(self.d_ref, self.ref)
        eng.to_device(self.d_ev, self.ev)
        self.pattern = np.arange(0xa0, 0xa0 + 32, dtype=np.uint8)
        eng.to_device(self.d_res, self.pattern)

    def result_bytes(self):
        out = np.empty(32, dtype=np.uint8)
        self.eng.to_host(out, self.d_res)
        return out

    def map(self):
        out = np.empty(self.shape, dtype=F)
        self.eng.to_host(out, self.d_map)
        return out

    def close(self):
        for p in (self.d_ref, self.d_ev, self.d_map, self.d_res):
            self.eng.device_free(p)


@pytest.fixture
def buffers(eng):
    b = Buffers(eng)
    yield b
    b.close()


def test_refusals_write_nothing(eng, engine, buffers):
    b = buffers
    reserved = abi.default_gamma_options()
    reserved.reserved[3] = 1
    cases = {
        "radius 11": dict(dims=b.dims, spacing=(0.14, 1.0, 1.0)),     # ceil(1.5 * 1.0 / 0.14) = 11
        "interp 3": dict(dims=b.dims, spacing=(1.0, 1.0, 1.0), interp=3),
        "zero dim": dict(dims=(b.dims[0], 0, b.dims[2]), spacing=(1.0, 1.0, 1.0)),
        "reserved word": dict(dims=b.dims, spacing=(1.0, 1.0, 1.0), opt=reserved),
    }
    assert gr.radii((0.14, 1.0, 1.0), 1.0)[0] == 11
    for what, kw in cases.items():
        dims, spacing = kw.pop("dims"), kw.pop("spacing")
        with pytest.raises(engine.RtdError) as ei:
            eng.gamma_device(b.d_ref, b.d_ev, dims, spacing, b.d_res, gamma_map=b.d_map, **kw)
        assert ei.value.status == abi.RTD_ERR_INVALID_ARG, what
        eng.sync()
        assert (b.result_bytes() == b.pattern).all(), what
    # ... and the handle goes on working: radius 10 is accepted
    eng.gamma_device(b.d_ref, b.d_ev, b.dims, (0.15, 1.0, 1.0), b.d_res, gamma_map=b.d_map)
    res = abi.RtdGammaResult.from_buffer_copy(b.result_bytes().tobytes())
    want = gr.gamma(b.ref, b.ev, (0.15, 1.0, 1.0))
    assert gr.radii((0.15, 1.0, 1.0), 1.0)[0] == 10
    assert (res.n_evaluated, res.n_passed) == (want.n_evaluated, want.n_passed) and bits(F(res.max_gamma)) == bits(want.max_gamma)
    assert res.norm_dose == b.ref.max() and list(res.reserved) == [0, 0]
    assert (bits(b.map()) == bits(want.map)).all()


def test_two_calls_give_equal_bits(eng, buffers):
    b = buffers
    seen = []
    for _ in range(2):
        eng.device_zero(b.d_map, b.ref.nbytes)
        eng.gamma_device(b.d_ref, b.d_ev, b.dims, (1.0, 1.0, 1.0), b.d_res, gamma_map=b.d_map, dd=0.03, dta=2.0, interp=2)
        seen.append((b.result_bytes().tobytes(), b.map().tobytes()))
    assert seen[0] == seen[1]
    res = abi.RtdGammaResult.from_buffer_copy(seen[0][0])
    assert res.n_evaluated == b.ref.size and 0 < res.n_passed


def test_zero_reference(eng):
    ev = np.ones((5, 6, 40), dtype=F)
    rate, n, gmax, gmap = eng.gamma(np.zeros_like(ev), ev, (1.0, 1.0, 1.0), want_map=True)
    assert (rate, n, gmax) == (1.0, 0, 0.0)
    assert (gmap == -1.0).all()
