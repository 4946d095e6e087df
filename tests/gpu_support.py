"""What more than one tests/test_gpu_*.py file uses, and nothing else: scene and option builders, the comparison helpers, the
switch for RTD_* environment variables, the single-field rig and the rig_of fixture factory. A plain module like asym_scenes.py and
target_scenes.py (no tests, no plugin); the rigs of the plan optimisers are in gpu_plan_rigs.py.

The rule for the tests: a test_*.py file imports from raytracedicom_amd, from oracle and from the non-test modules of tests/. It
never imports from another test_*.py.

pytest does not rewrite the asserts of this module, so every assert here carries a message with the values it compared."""
import contextlib
import math

import numpy as np
import pytest

from raytracedicom_amd import abi, luts, scenarios


# ---- scenes and options ------------------------------------------------------------------------------------------------------

def options(cutoff, timing=0, nuclear=0):
    o = abi.default_options()
    o.ray_weight_cutoff = cutoff
    o.fine_grained_timing = timing
    o.nuclear_corr = nuclear
    return o


def hetero_scene(synth, n, angles, source_dist=(math.inf, math.inf), spots=5, pitch=8.0, layers=3, seed=5, **kw):
    """One field per angle on the n^3 heterogeneous phantom."""
    ct, _ = scenarios.hetero_phantom(n)
    return scenarios.hetero_ct(synth, n=n, spots=spots, pitch=pitch, n_layers=layers, angles=list(angles), ct=ct, source_dist=source_dist,
                               seed=seed, **kw)


def radii_above_16(synth):
    ct, _ = scenarios.hetero_phantom(96)
    beam = scenarios.make_field(synth, 96, 256.0 / 96, (-128.0, -128.0, -106.0), 0.0, 4, 6.0, 3, 21, steps=200, ray_spacing=(0.5, 0.5),
                                weight_lo=400.0)
    return scenarios.Scenario("rays 0.5 mm", synth, ct, (256.0 / 96,) * 3, [beam])


@pytest.fixture(scope="module")
def nuc_luts():
    return luts.synth_luts(nuclear=True)


@contextlib.contextmanager
def switches(**env):
    """The given RTD_* variables in the environment (None: absent) for the duration of the block; what was there before comes back
    at its end. The engine reads its switches when a field is created."""
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            if v is None:
                mp.delenv(k, raising=False)
            else:
                mp.setenv(k, v)
        yield


# ---- the single-field rig ----------------------------------------------------------------------------------------------------

class FieldRig:
    """One engine with the scenario's options (None: the engine's own), LUTs and CT (a host upload unless set_ct is false), one
    device dose volume on the dose grid dims (x, y, z; default the CT's) and the plumbing of the calls that take a field."""

    def __init__(self, engine, scn, opt, dims=None, set_ct=True):
        self.engine = engine
        self.eng = engine.Engine(0)
        if opt is not None:
            self.eng.set_options(opt)
        self.eng.set_luts(scn.luts)
        if set_ct:
            self.eng.set_ct(scn.ct)
        self.dims = tuple(dims or scn.dims)
        self.shape = (self.dims[2], self.dims[1], self.dims[0])
        self.nb = int(np.prod(self.shape)) * 4
        self.dDose = self.eng.device_alloc(self.nb)
        self.dG = None                                                # (the voxel-weight volume of the transposed calls, on first use)
        self.fields = []

    def field(self, beam, **env):
        """A field created with the given RTD_* switches in the environment."""
        with switches(**env):
            f = self.eng.create_field(beam, self.dims)
        self.fields.append(f)
        return f

    def compute(self, f):
        """One compute into the zeroed volume, with a finish -> (dose, info, timing)."""
        self.eng.device_zero(self.dDose, self.nb)
        f.compute(self.dDose)
        timing, info = f.finish()
        dose = np.empty(self.shape, dtype=np.float32)
        self.eng.to_host(dose, self.dDose)
        return dose, info, timing

    def dose(self, beam):
        f = self.field(beam)
        d, _, _ = self.compute(f)
        self.fields.remove(f)
        f.destroy()
        return d

    def _spot_call(self, f, call, g):
        if self.dG is None:
            self.dG = self.eng.device_alloc(self.nb)
        self.eng.to_device(self.dG, np.ascontiguousarray(g, dtype=np.float32))
        shape = f._beam.spotWeights.shape
        dOut = self.eng.device_alloc(int(np.prod(shape)) * 4)
        try:
            call(self.dG, dOut)
            out = np.empty(shape, dtype=np.float32)
            self.eng.to_host(out, dOut)
        finally:
            self.eng.device_free(dOut)
        return out

    def grad(self, f, g):
        return self._spot_call(f, f.spot_gradient, g)

    def apply_t(self, f, g):
        """Dij^T g on the device -> [L][ny][nx] float32."""
        return self._spot_call(f, f.dose_influence_apply_t, g)

    def apply(self, f, w, into=None, init=True):
        """Dij w on the device into a copy of `into` (default: a NaN-filled volume) -> the volume."""
        vol = np.full(self.shape, np.nan, dtype=np.float32) if into is None else np.ascontiguousarray(into, dtype=np.float32)
        w = np.ascontiguousarray(w, dtype=np.float32)
        dW = self.eng.device_alloc(w.nbytes)
        try:
            self.eng.to_device(dW, w)
            self.eng.to_device(self.dDose, vol)
            f.dose_influence_apply(dW, self.dDose, init=init)
            out = np.empty(self.shape, dtype=np.float32)
            self.eng.to_host(out, self.dDose)
        finally:
            self.eng.device_free(dW)
        return out

    def product(self, f, w):
        """Dij w as a flat float32 volume with zeros where nothing was written."""
        return self.apply(f, w, into=np.zeros(self.shape, dtype=np.float32), init=True).reshape(-1)

    def close(self):
        for f in self.fields:
            f.destroy()
        self.eng.device_free(self.dDose)
        if self.dG is not None:
            self.eng.device_free(self.dG)
        self.eng.close()


def rig_fixture(cls, name="rig_of"):
    """The fixture `name` of a rig class: a function that makes rigs (the engine module first, then the caller's arguments); all of
    them are closed at teardown."""
    @pytest.fixture(name=name)
    def rig_of(engine):
        rigs = []

        def make(*args, **kw):
            r = cls(engine, *args, **kw)
            rigs.append(r)
            return r
        yield make
        for r in rigs:
            r.close()
    return rig_of


# ---- comparisons -------------------------------------------------------------------------------------------------------------

def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def rel_close(a, b, rtol, floor_frac=1e-3, atol_frac=1e-6):
    a = a.astype(np.float64); b = b.astype(np.float64)
    mx = np.abs(b).max()
    mask = np.abs(b) > floor_frac * mx
    err = np.abs(a - b)
    assert (err[mask] <= rtol * np.abs(b[mask]) + atol_frac * mx).all(), \
        "max rel err %g" % (err[mask] / np.abs(b[mask])).max()
    assert (err[~mask] <= 2 * rtol * floor_frac * mx + atol_frac * mx).all(), \
        "max abs err %g below the floor, bound %g" % (err[~mask].max(), 2 * rtol * floor_frac * mx + atol_frac * mx)


def dot(a, b):
    """(<a, b>, <|a|, |b|>) in float64."""
    a = np.asarray(a).reshape(-1)
    b = np.asarray(b).reshape(-1)
    s = m = 0.0
    for i in range(0, a.size, 1 << 24):
        x, y = a[i:i + (1 << 24)].astype(np.float64), b[i:i + (1 << 24)].astype(np.float64)
        s += float(np.dot(x, y))
        m += float(np.dot(np.abs(x), np.abs(y)))
    return s, m


def close(p, q, tol):
    (a, ma), (b, mb) = p, q
    scale = max(ma, mb)
    assert scale > 0, "both scales are zero: %r, %r" % (p, q)
    assert abs(a - b) <= tol * scale, "%.9g vs %.9g (diff %.3g of scale %.3g)" % (a, b, abs(a - b), scale)


U = 2.0 ** -24


def gamma(n):
    k = (np.asarray(n, dtype=np.float64) + 1.0) * U
    return k / (1.0 - k)


def col_of_entry(d):
    return np.repeat(np.arange(d.shape[1], dtype=np.int64), np.diff(d.indptr))


def row_bound(d, w):
    """Per voxel: (entries of the row, sum |a| |w| in float64)."""
    n = np.bincount(d.indices, minlength=d.shape[0])
    s = np.bincount(d.indices, weights=np.abs(d.data.astype(np.float64)) * np.abs(np.asarray(w, dtype=np.float64).reshape(-1))[col_of_entry(d)],
                    minlength=d.shape[0])
    return n, s


def col_bound(d, g):
    """Per spot: (entries of the column, sum |a| |g| in float64)."""
    n = np.diff(d.indptr)
    s = np.bincount(col_of_entry(d), weights=np.abs(d.data.astype(np.float64)) * np.abs(np.asarray(g, dtype=np.float64).reshape(-1))[d.indices],
                    minlength=d.shape[1])
    return n, s


def worst_ratio(err, bound):
    live = bound > 0
    return float(np.max(err[live] / bound[live])) if live.any() else 0.0


def box_mask(rig, info):
    lo, hi = info["dose_box_min"], info["dose_box_max"]
    m = np.zeros(rig.shape, dtype=bool)
    m[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    return m


def compare_field(orc, engine, scn, beam, options=None, dose_dims=None, dose_spacing=None, inspect=None):
    """One field of the engine against the CPU oracle, stage by stage (the tolerances: tests/test_gpu_parity.py) -> (dose, the
    oracle's dose, timing, info). dose_dims, dose_spacing: the dose grid of the beam's gantryToDoseIdx when it is not the CT's.
    inspect: called with the computed field in front of the comparisons (what a test fetches beyond them, "launch_builds" say)."""
    dose_dims = tuple(scn.dims if dose_dims is None else dose_dims)
    dose_spacing = scn.spacing if dose_spacing is None else dose_spacing
    dose_ref = np.zeros((dose_dims[2], dose_dims[1], dose_dims[0]), dtype=np.float32)
    of = orc.run_field(scn, beam, dose_ref, options=options, keep_layers=True, dose_dims=dose_dims)
    assert of.status == 0, (of.status, of.error)
    rig = FieldRig(engine, scn, options, dose_dims)
    try:
        fld = rig.field(beam)
        dose, info, timing = rig.compute(fld)
        if inspect is not None:
            inspect(fld)
        oi = of.info
        for k in ("ray_dims", "beam_first_inside", "beam_first_outside", "beam_first_guaranteed_passive",
                  "beam_first_calculated_passive", "bbox_min", "bbox_max", "live_steps", "max_radius"):
            assert info[k] == oi[k], (k, info[k], oi[k])
        np.testing.assert_array_equal(np.array(info["ray_offset"], np.float32), np.array(oi["ray_offset"], np.float32))
        W, H, L = oi["ray_dims"]
        S = beam.tracerSteps
        # stage 1: tracer — bit-exact
        for name in ("density", "wepl", "first_inside", "first_outside", "wepl_min"):
            np.testing.assert_array_equal(fld.fetch(name), of.get(name), err_msg=name)
        # stage 2: plan + spot->ray weights
        np.testing.assert_allclose(fld.fetch("layer_plan").reshape(L, 8)[:, :6], of.get("layer_plan").reshape(L, 8)[:, :6], rtol=1e-6)
        np.testing.assert_array_equal(fld.fetch("ray_weights"), of.get("ray_weights"))
        # stage 3: fill
        first, calc = oi["beam_first_inside"], oi["beam_first_calculated_passive"]
        np.testing.assert_array_equal(fld.fetch("first_passive"), of.get("first_passive"))
        plan = of.get("layer_plan").reshape(L, 8)
        idd_g, idd_o = fld.fetch("idd").reshape(L, S, H, W), of.get("idd").reshape(L, S, H, W)
        rs_g, rs_o = fld.fetch("rsigma").reshape(L, S, H, W), of.get("rsigma").reshape(L, S, H, W)
        tr_g = fld.fetch("tile_radius").reshape(L, S, H // 8, W // 32)
        tr_o = of.get("tile_radius").reshape(L, S, H // 8, W // 32)
        for l in range(L):
            a0, a1 = first, int(plan[l, 5])
            np.testing.assert_allclose(idd_g[l, a0:a1], idd_o[l, a0:a1], rtol=2e-5, atol=1e-12, err_msg="idd layer %d" % l)
            fin = np.isfinite(rs_o[l, a0:a1])
            np.testing.assert_array_equal(np.isfinite(rs_g[l, a0:a1]), fin)
            np.testing.assert_allclose(rs_g[l, a0:a1][fin], rs_o[l, a0:a1][fin], rtol=2e-5)
            lfp = int(plan[l, 6])
            # index work: radius class of every (step, tile) bit-exact (tileRadCalc, kernel_wrapper.cuh:256-313)
            if not np.array_equal(tr_g[l, a0:lfp], tr_o[l, a0:lfp]):
                ks, tys, txs = np.nonzero(tr_g[l, a0:lfp] != tr_o[l, a0:lfp])
                k, ty, tx = int(ks[0]) + a0, int(tys[0]), int(txs[0])
                mg = rs_g[l, k, 8 * ty:8 * ty + 8, 32 * tx:32 * tx + 32].min()
                mo = rs_o[l, k, 8 * ty:8 * ty + 8, 32 * tx:32 * tx + 32].min()
                raise AssertionError("tile_radius differs on %d (step, tile) of layer %d; first at step %d tile (%d, %d): engine %d, oracle %d; "
                                     "tile minimum of 1/sigma: engine %r (0x%08x), oracle %r (0x%08x)"
                                     % (ks.size, l, k, tx, ty, tr_g[l, k, ty, tx], tr_o[l, k, ty, tx], float(mg), np.float32(mg).view(np.uint32),
                                        float(mo), np.float32(mo).view(np.uint32)))
        # batch radius per radius class (host batching rule, kernel_wrapper.cu:966-976)
        np.testing.assert_array_equal(fld.fetch("eff_radius").reshape(L, -1), of.get("eff_radius").reshape(L, -1))
        # stage 4/5: BEV and final dose
        bev_g, bev_o = fld.fetch("bev"), of.get("bev")
        rel_close(bev_g, bev_o, rtol=1e-4)
        rel_close(dose, dose_ref, rtol=1e-4)
        rate, n_eval, gmax = orc.gamma_pass_rate(dose_ref, dose, dose_spacing)
        assert n_eval > 0 and rate == 1.0, (rate, n_eval, gmax)
        return dose, dose_ref, timing, info
    finally:
        rig.close()


def compare_nuclear_field(orc, engine, scn, opt, dose_dims=None, dose_spacing=None, inspect=None):
    """The scenario's first beam under a nuclear correction against the oracle -> (dose, the oracle's dose, the oracle's info).
    dose_dims, dose_spacing: the dose grid of the beam's gantryToDoseIdx when it is not the CT's (default). inspect: as in
    compare_field."""
    dose_dims = tuple(scn.dims if dose_dims is None else dose_dims)
    dose_spacing = scn.spacing if dose_spacing is None else dose_spacing
    ref = np.zeros((dose_dims[2], dose_dims[1], dose_dims[0]), dtype=np.float32)
    of = orc.run_field(scn, scn.beams[0], ref, options=opt, keep_layers=True, dose_dims=dose_dims)
    assert of.status == 0, of.error
    rig = FieldRig(engine, scn, opt, dose_dims)
    try:
        f = rig.field(scn.beams[0])
        dose, info, _ = rig.compute(f)
        if inspect is not None:
            inspect(f)
        W, H, L = of.info["ray_dims"]
        S = scn.beams[0].tracerSteps
        # the sigma chain with the variant's constants: radius classes stay bit-exact (over the steps the reference classifies)
        plan = of.get("layer_plan").reshape(L, 8)
        tr_g = f.fetch("tile_radius").reshape(L, S, H // 8, W // 32)
        tr_o = of.get("tile_radius").reshape(L, S, H // 8, W // 32)
        for l in range(L):
            a0, lfp = of.info["beam_first_inside"], int(plan[l, 6])
            np.testing.assert_array_equal(tr_g[l, a0:lfp], tr_o[l, a0:lfp])
        np.testing.assert_array_equal(f.fetch("eff_radius"), of.get("eff_radius"))
        idd_g, idd_o = f.fetch("idd").reshape(L, S, H, W), of.get("idd").reshape(L, S, H, W)
        for l in range(L):
            a0, a1 = of.info["beam_first_inside"], int(plan[l, 5])
            np.testing.assert_allclose(idd_g[l, a0:a1], idd_o[l, a0:a1], rtol=2e-5, atol=1e-12)
    finally:
        rig.close()
    mx = float(ref.max())
    assert mx > 0, "the oracle's dose is zero everywhere (max %g)" % mx
    thr = ref > 1e-3 * mx
    assert (np.abs(dose - ref)[thr] <= 1e-4 * ref[thr] + 1e-6 * mx).all(), float((np.abs(dose - ref)[thr] / ref[thr]).max())
    assert np.abs(dose - ref).max() <= 2e-5 * mx, "max abs err %g, bound %g" % (np.abs(dose - ref).max(), 2e-5 * mx)
    rate, n_eval, gmax = orc.gamma_pass_rate(ref, dose, dose_spacing)
    assert rate == 1.0 and n_eval > 0, (rate, n_eval, gmax)
    return dose, ref, of.info


def stage_identities(rig, beam, g, tol):
    """<g, D> = <grad_bev, bev> = <grad_ray_weights, ray_weights> = <grad, w> of one forward run -> (field, dose, grad, info)."""
    f = rig.field(beam)
    dose, info, _ = rig.compute(f)
    assert dose.max() > 0, "the dose is zero everywhere (max %g)" % dose.max()
    grad = rig.grad(f, g)
    bev, gbev = f.fetch("bev"), f.fetch("grad_bev")
    rw, grw = f.fetch("ray_weights"), f.fetch("grad_ray_weights")
    close(dot(g, dose), dot(gbev, bev), tol)
    close(dot(gbev, bev), dot(grw, rw), tol)
    close(dot(grw, rw), dot(grad, beam.spotWeights), tol)
    return f, dose, grad, info


def end_to_end(rig, beam, g, seed, tol=1e-5):
    """<D(w + delta) - D(w), g> = <delta, grad(w)> for a seeded random delta >= 0 -> the info of the forward at w."""
    rng = np.random.default_rng(seed)
    w = beam.spotWeights
    delta = (0.5 * w * rng.random(w.shape)).astype(np.float32)
    f = rig.field(beam)
    d0, info, _ = rig.compute(f)
    grad = rig.grad(f, g)
    d1 = rig.dose(beam.replace(spotWeights=w + delta))
    dd = (d1.astype(np.float64) - d0.astype(np.float64))
    assert np.abs(dd).max() > 0, "D(w + delta) equals D(w): delta max %g" % delta.max()
    close(dot(dd, g), dot(delta, grad), tol)
    return info
