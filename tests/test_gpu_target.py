"""GPU tests of rtd_field_project_target / rtd_field_select_spots (include/rtd.h "Spots from a target"): the
packed projection, the layer hits, the spot mask and every field of the summary are compared bit for bit with the numpy restatement
(tests/target_reference.py) fed with the engine's own "wepl" and "layer_plan". Fields and targets: tests/target_scenes.py (the scenes of
tests/asym_scenes.py with 9 x 7 spots and 8 layers); tests/test_target_reference.py pins on the CPU that they select what they should."""
import ctypes as C
import math

import numpy as np
import pytest

import asym_scenes as S
import target_reference as T
import target_scenes as TS
from raytracedicom_amd import abi, spots

pytestmark = pytest.mark.gpu

EMPTY_INFO = {"n_samples": 0, "wepl_min": 0.0, "wepl_max": 0.0, "ray_lo": [0, 0], "ray_hi": [0, 0], "step_lo": 0, "step_hi": 0}


class Rig:
    """One engine with one computed field of a scene, its trace on the host, and the comparison with the restatement."""

    def __init__(self, engine, luts, name, beam=None):
        self.scn = TS.scene(luts, name)
        self.beam = beam if beam is not None else self.scn.beams[0]
        self.dims = self.scn.dose_dims
        self.nvox = int(np.prod(self.dims))
        self.eng = engine.Engine(0)
        self.eng.set_options(TS.options())
        self.eng.set_luts(self.scn.luts)
        self.eng.set_ct(self.scn.ct)
        self.d_dose = self.eng.device_alloc(4 * self.nvox)
        self.eng.device_zero(self.d_dose, 4 * self.nvox)
        self.field = self.eng.create_field(self.beam, self.dims)
        self.field.compute(self.d_dose)
        _, self.info = self.field.finish()
        self.g = T.geometry_of(self.info, self.beam)
        self.wepl = self.field.fetch("wepl").reshape(self.g.S, self.g.H, self.g.W)
        self.peaks = self.field.fetch("layer_plan").reshape(-1, 8)[:, 2].copy()
        assert (np.diff(self.wepl, axis=0) >= 0).all()
        self._inside = {}

    def inside(self, key, mask):
        """The restatement's projection of `mask`, computed once per key."""
        if key not in self._inside:
            self._inside[key] = T.project(self.g, mask)
        return self._inside[key]

    def check(self, key, mask, margins):
        """project + one select per (lateral, proximal, distal) of `margins`, everything compared; returns (info, [spot masks])."""
        inside = self.inside(key, mask)
        info = self.field.project_target(mask)
        assert info == T.summary(inside, self.wepl)
        words = (self.g.S + 31) // 32
        np.testing.assert_array_equal(self.field.fetch("target_bev").reshape(words, self.g.H, self.g.W), T.pack(inside))
        out = []
        for lateral, proximal, distal in margins:
            sel = self.field.select_spots(lateral, proximal, distal)
            hit = T.hits(inside, self.wepl, self.peaks, proximal, distal)
            np.testing.assert_array_equal(self.field.fetch("target_hit").reshape(hit.shape), hit, err_msg=str((proximal, distal)))
            np.testing.assert_array_equal(sel, T.spots(self.g, hit, lateral), err_msg=str((lateral, proximal, distal)))
            out.append(sel)
        return info, out

    def count(self, lateral=0.0, proximal=0.0, distal=0.0):
        """rtd_field_select_spots with n_selected: (mask, count)."""
        o = abi.RtdTargetOptions()
        o.lateral_margin_mm, o.proximal_margin_mm, o.distal_margin_mm = lateral, proximal, distal
        out = np.empty(self.beam.spotWeights.shape, dtype=np.uint8)
        d = self.eng.device_alloc(out.nbytes)
        n = C.c_uint32(0xffffffff)
        self.eng._check(_lib(self.eng).rtd_field_select_spots(self.eng._h, self.field._h, C.byref(o), C.c_void_p(d), C.byref(n)))
        self.eng.to_host(out, d)
        self.eng.device_free(d)
        return out, int(n.value)

    def volume(self, ptr):
        out = np.empty(self.nvox, dtype=np.float32)
        self.eng.to_host(out, ptr)
        return out

    def close(self):
        self.field.destroy()
        self.eng.device_free(self.d_dose)
        self.eng.close()


def _lib(eng):
    from raytracedicom_amd import engine
    return engine.lib()


@pytest.fixture(scope="module")
def rigs(engine, synth):
    """name -> the scene's rig, made once and shared; the tests leave its field's weights and compute as they found them."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Rig(engine, synth, name)
        return cache[name]
    yield get
    for r in cache.values():
        r.close()


# ---------------------------------------------------------------------------------------------------- bits against the restatement

@pytest.mark.parametrize("margins", TS.MARGINS, ids=["zero", "6-2-5"])
@pytest.mark.parametrize("name", ["A", "B", "C", "F"])
def test_bits_against_the_restatement(rigs, name, margins):
    """A: oblique, divergent, coarse grid, 300 steps (a partial last word). B: the fine grid that overhangs the CT, the target cut by the
    grid's last slice. C: a parallel beam, infinite source distances. F: rays of 0.5 x 0.75 mm, a disc that is no circle in rays."""
    r = rigs(name)
    mask = TS.target(r.scn, r.g, r.wepl, r.peaks)
    info, (sel,) = r.check("target", mask, [margins])
    assert info["n_samples"] > 1000 and sel.any() and not sel.all()
    if name == "A":
        assert (r.g.W, r.g.H, r.g.S) == (128, 80, 300)
    if name == "F":
        assert r.info["ray_res"][:2] == [0.5, 0.75]
    if name == "B":
        # the target touches the grid's face, and rays leave the grid from inside it: a target sample next to one without a voxel
        _, in_grid = T.nearest_voxel(r.g, r.dims)
        inside = r.inside("target", mask)
        assert mask[-1].any()
        assert ((inside[:-1] & ~in_grid[1:]) | (inside[1:] & ~in_grid[:-1])).any()


# ----------------------------------------------------------------------------------------------------------- shapes that can go wrong

def test_empty_mask_and_whole_grid(rigs):
    r = rigs("A")
    shape = (r.dims[2], r.dims[1], r.dims[0])
    info, (sel,) = r.check("empty", np.zeros(shape, dtype=np.uint8), [(6.0, 2.0, 5.0)])
    assert info == EMPTY_INFO and not sel.any()
    assert not r.field.fetch("target_bev").any()
    sel, n = r.count(6.0, 2.0, 5.0)
    assert n == 0 and not sel.any()
    info, (sel0, sel1) = r.check("full", np.ones(shape, dtype=bool), [(0.0, 0.0, 0.0), (6.0, 2.0, 5.0)])
    assert info["n_samples"] > 100000 and 0 < info["step_lo"] < info["step_hi"] < r.g.S - 1     # the rays enter the grid and leave it
    got, n = r.count(6.0, 2.0, 5.0)
    np.testing.assert_array_equal(got, sel1)
    assert n == int(sel1.sum()) > int(sel0.sum()) > 0


def test_layer_beyond_every_ray(engine, synth):
    """220 MeV/u: a peak depth of 307 mm where no ray collects more than 150 mm. kLo == S on every ray: no hit, whatever the target."""
    r = Rig(engine, synth, "A", beam=TS.with_last_energy(synth, TS.scene(synth, "A").beams[0], 220.0))
    try:
        assert r.peaks[-1] > r.wepl.max() + 5.0
        mask = np.ones((r.dims[2], r.dims[1], r.dims[0]), dtype=np.uint8)
        _, (sel0, sel1) = r.check("full", mask, [(0.0, 0.0, 0.0), (6.0, 2.0, 5.0)])
        hit = r.field.fetch("target_hit").reshape(-1, r.g.H, r.g.W)
        assert not sel0[-1].any() and not sel1[-1].any() and not hit[-1].any()
        assert sel1[:-1].any() and hit[:-1].any()
    finally:
        r.close()


@pytest.mark.parametrize("name", ["A", "F"])
def test_lateral_margin_wider_than_the_ray_grid(rigs, name):
    """The window is clipped to the ray grid: every spot takes every ray, so a layer with a hit anywhere selects all its spots."""
    r = rigs(name)
    mask = TS.target(r.scn, r.g, r.wepl, r.peaks)
    _, sels = r.check("target", mask, [(1000.0, 0.0, 0.0), (3.0e38, 0.0, 0.0)])
    hit = r.field.fetch("target_hit").reshape(-1, r.g.H, r.g.W)
    for sel in sels:
        for l in range(sel.shape[0]):
            assert sel[l].all() if hit[l].any() else not sel[l].any()
    assert 0 < sum(int(hit[l].any()) for l in range(hit.shape[0])) < hit.shape[0]


def test_hollow_two_slab_target(rigs):
    """Scene U (parallel beam, water): the peaks of layers 3 and 4 fall between the two parts of the target on every ray."""
    r = rigs("U")
    mask = TS.two_slabs(r.scn, r.g, r.wepl, r.peaks)
    _, (sel0, prox, dist, both) = r.check("slabs", mask, [(0.0, 0.0, 0.0), (0.0, 8.0, 0.0), (0.0, 0.0, 8.0), (0.0, 8.0, 8.0)])
    n0 = sel0.sum(axis=(1, 2))
    assert n0[2] > 0 and n0[3] == 0 and n0[4] == 0 and n0[5] > 0, n0
    assert not prox[3].any() and prox[4].any() and dist[3].any() and not dist[4].any() and both[3].any() and both[4].any()


# --------------------------------------------------------------------------------------------------------------- nothing else moves

def test_nothing_else_moves(engine, synth, rigs):
    r = rigs("A")
    mask = TS.target(r.scn, r.g, r.wepl, r.peaks)
    d2 = r.eng.device_alloc(4 * r.nvox)

    def transferred():
        r.eng.device_zero(d2, 4 * r.nvox)
        r.field.transfer(d2)
        return r.volume(d2)
    bev0, dose0 = r.field.fetch("bev").copy(), transferred()
    assert dose0.max() > 0
    info, (sel0, sel1) = r.check("target", mask, TS.MARGINS)
    bev_words = r.field.fetch("target_bev").copy()
    np.testing.assert_array_equal(r.field.fetch("bev").view(np.uint32), bev0.view(np.uint32))
    np.testing.assert_array_equal(transferred().view(np.uint32), dose0.view(np.uint32))
    np.testing.assert_array_equal(r.field.fetch("wepl").reshape(r.wepl.shape).view(np.uint32), r.wepl.view(np.uint32))
    r.eng.device_free(d2)
    # a second engine: the same bits
    other = Rig(engine, synth, "A")
    try:
        assert other.field.project_target(mask) == info
        np.testing.assert_array_equal(other.field.fetch("target_bev"), bev_words)
        np.testing.assert_array_equal(other.field.select_spots(*TS.MARGINS[1]), sel1)
        np.testing.assert_array_equal(other.field.select_spots(), sel0)
        hit0 = other.field.fetch("target_hit").copy()
        # new weights, a compute that keeps the trace: the selection, made from the stored projection, is the same
        w = (50.0 + 20.0 * np.random.default_rng(5).random(other.beam.spotWeights.shape)).astype(np.float32)
        d_w = other.eng.device_alloc(w.nbytes)
        other.eng.to_device(d_w, w)
        other.field.set_spot_weights(d_w)
        other.eng.device_zero(other.d_dose, 4 * other.nvox)
        other.field.compute(other.d_dose)
        other.field.finish()
        assert int(other.field.fetch("trace_reused")[0]) == 1
        np.testing.assert_array_equal(other.field.select_spots(), sel0)
        np.testing.assert_array_equal(other.field.fetch("target_hit"), hit0)
        np.testing.assert_array_equal(other.field.select_spots(*TS.MARGINS[1]), sel1)
        other.eng.device_free(d_w)
    finally:
        other.close()


# ------------------------------------------------------------------------------------------------------------------------- refusals

def _status(call):
    from raytracedicom_amd import engine
    with pytest.raises(engine.RtdError) as e:
        call()
    return e.value.status


def test_refusals_leave_the_handle_usable(engine, synth):
    scn = TS.scene(synth, "A")
    dims, beam = scn.dose_dims, scn.beams[0]
    n = int(np.prod(dims))
    L = engine.lib()
    with engine.Engine(0) as eng:
        eng.set_options(TS.options())
        eng.set_luts(scn.luts)
        eng.set_ct(scn.ct)
        d_mask, d_out, d_dose = eng.device_alloc(n), eng.device_alloc(beam.spotWeights.size), eng.device_alloc(4 * n)
        eng.device_zero(d_dose, 4 * n)
        f = eng.create_field(beam, dims)
        # before any compute
        assert _status(lambda: f.project_target(d_mask)) == abi.RTD_ERR_NOT_READY
        assert _status(lambda: f.select_spots(dev_out=d_out)) == abi.RTD_ERR_NOT_READY
        f.compute(d_dose)
        _, info = f.finish()
        g = T.geometry_of(info, beam)
        wepl = f.fetch("wepl").reshape(g.S, g.H, g.W)
        peaks = f.fetch("layer_plan").reshape(-1, 8)[:, 2].copy()
        mask = TS.target(scn, g, wepl, peaks)
        eng.to_device(d_mask, mask)
        # select before project
        assert _status(lambda: f.select_spots(dev_out=d_out)) == abi.RTD_ERR_NOT_READY
        # a remote field
        rf = eng.create_field(beam, dims, remote=True)
        assert _status(lambda: rf.project_target(d_mask)) == abi.RTD_ERR_INVALID_ARG
        assert _status(lambda: rf.select_spots(dev_out=d_out)) == abi.RTD_ERR_INVALID_ARG
        rf.destroy()
        # null pointers
        ti = abi.RtdTargetInfo()
        assert L.rtd_field_project_target(eng._h, f._h, None, C.byref(ti)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_project_target(eng._h, f._h, C.c_void_p(d_mask), None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_project_target(eng._h, None, C.c_void_p(d_mask), C.byref(ti)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_field_select_spots(eng._h, f._h, None, None, None) == abi.RTD_ERR_INVALID_ARG
        want = f.project_target(d_mask)
        assert want["n_samples"] > 1000
        assert L.rtd_field_select_spots(eng._h, f._h, None, None, None) == abi.RTD_ERR_INVALID_ARG
        # margins
        for bad in (-1.0, -1e-30, math.nan, math.inf, -math.inf):
            for which in ("lateral", "proximal", "distal"):
                assert _status(lambda: f.select_spots(dev_out=d_out, **{which: bad})) == abi.RTD_ERR_INVALID_ARG, (which, bad)
        # everything still works, and gives what the restatement gives; opt == NULL means no margins
        inside = T.project(g, mask)
        assert f.project_target(d_mask) == want == T.summary(inside, wepl)
        sel0 = f.select_spots()
        np.testing.assert_array_equal(sel0, T.spots(g, T.hits(inside, wepl, peaks), 0.0))
        cnt = C.c_uint32(0)
        assert L.rtd_field_select_spots(eng._h, f._h, None, C.c_void_p(d_out), C.byref(cnt)) == abi.RTD_OK
        got = np.empty(beam.spotWeights.shape, dtype=np.uint8)
        eng.to_host(got, d_out)
        np.testing.assert_array_equal(got, sel0)
        assert cnt.value == sel0.sum() > 0
        # the numpy and the bool form of the mask give the same projection as the device pointer
        assert f.project_target(mask) == want and f.project_target(mask.astype(bool)) == want
        f.destroy()
        for p in (d_mask, d_out, d_dose):
            eng.device_free(p)


def test_nuclear_corr_is_refused(engine):
    from raytracedicom_amd import luts
    nuc = luts.synth_luts(nuclear=True)
    scn = S.scene(nuc, "N")
    n = int(np.prod(scn.dose_dims))
    with engine.Engine(0) as eng:
        eng.set_options(S.options("N", cutoff=0.0))
        eng.set_luts(scn.luts)
        eng.set_ct(scn.ct)
        d_mask, d_out = eng.device_alloc(n), eng.device_alloc(scn.beams[0].spotWeights.size)
        eng.device_zero(d_mask, n)
        f = eng.create_field(scn.beams[0], scn.dose_dims)
        assert _status(lambda: f.project_target(d_mask)) == abi.RTD_ERR_INVALID_ARG
        assert _status(lambda: f.select_spots(dev_out=d_out)) == abi.RTD_ERR_INVALID_ARG
        f.destroy()
        eng.device_free(d_mask)
        eng.device_free(d_out)


# ------------------------------------------------------------------------------------------------------------------------ end to end

def _ellipsoid_contours(scn, centre, semi_axes, n_points=40):
    """The ellipsoid as closed contours on the planes of the dose grid's slices (what an RT Structure Set would carry)."""
    out = []
    t = np.linspace(0.0, 2.0 * np.pi, n_points, endpoint=False)
    for k in range(scn.dose_dims[2]):
        z = scn.dose_origin[2] + scn.dose_spacing[2] * k
        s2 = 1.0 - ((z - centre[2]) / semi_axes[2]) ** 2
        if s2 <= 0.05:
            continue
        s = math.sqrt(s2)
        out.append(np.stack([centre[0] + semi_axes[0] * s * np.cos(t), centre[1] + semi_axes[1] * s * np.sin(t), np.full_like(t, z)], axis=1).astype(np.float32))
    return out


def test_target_to_optimiser(engine, synth, rigs):
    """Contours -> ROI -> spots.place_spots -> the field of the placed beam -> its dose-influence matrix -> the resident optimiser with
    a squared-deviation term on the target."""
    r = rigs("A")
    scn, cand = r.scn, r.beam
    centre = TS.central_point(scn, r.g, r.wepl, r.peaks)
    sp, origin = np.asarray(scn.dose_spacing), np.asarray(scn.dose_origin)
    world_to_idx = (np.diag(1.0 / sp).astype(np.float32), (-origin / sp).astype(np.float32))
    with engine.Engine(0) as eng:
        eng.set_options(TS.options())
        eng.set_luts(scn.luts)
        eng.set_ct(scn.ct)
        roi = eng.rasterize_roi(scn.dose_dims, world_to_idx, _ellipsoid_contours(scn, centre, TS.SEMI_AXES), scn.dose_spacing[2])
        voxels = roi.voxels()
        assert voxels.size > 200
        placed = spots.place_spots(eng, cand, roi, scn.dose_dims, lateral=3.0, proximal=2.0, distal=2.0)
        assert placed is not None
        w = placed.spotWeights
        assert 1 <= w.size < cand.spotWeights.size and w.sum() >= 1 and set(np.unique(w)) <= {0.0, 1.0}
        assert w.any(axis=(1, 2)).all() and w.any(axis=(0, 2)).all() and w.any(axis=(0, 1)).all()     # cropped: no empty layer, row or column
        assert w.shape[0] < cand.spotWeights.shape[0] and set(placed.beamEnergies) <= set(cand.beamEnergies)
        field = eng.create_field(placed, scn.dose_dims)
        dij = field.dose_influence()
        dose = dij.matvec(w)
        level = 1.5 * float(dose[voxels].mean())
        assert level > 0
        obj = eng.create_objective(scn.dose_dims)
        obj.add_term(abi.RTD_OBJ_SQ_DEVIATION, obj.add_roi(voxels), 1.0, level)
        opt = eng.create_optimizer([field], obj)
        opt.run(30)
        rep, hist = opt.result()
        assert hist.size == 30 and math.isfinite(rep["f_best"]) and rep["f_best"] < hist[0]
        opt.destroy()
        obj.destroy()
        field.destroy()
        roi.close()
