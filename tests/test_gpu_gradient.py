"""GPU tests of the spot-weight gradient (rtd_field_spot_gradient / rtd_spot_gradient): the transposed dose path.

Dot products are taken in float64 on the host; every tolerance is relative to sum |a| |b| of the pair compared. Unless stated
otherwise the ray-weight cut-off is 0, so the live set does not depend on the weights (the gradient is then exact for every
delta >= 0)."""

import numpy as np
import pytest

from gpu_support import FieldRig, close, dot, end_to_end, hetero_scene, options, radii_above_16, rig_fixture, stage_identities
from raytracedicom_amd import abi, scenarios

pytestmark = pytest.mark.gpu

rig_of = rig_fixture(FieldRig)


def test_stage_transposes_from_one_forward_run(rig_of, synth):
    """<g, D> = <grad_bev, bev> = <grad_ray_weights, ray_weights> = <grad, w>: heterogeneous CT, rotated divergent beam."""
    scn = hetero_scene(synth, 96, [30.0], source_dist=(2000.0, 2300.0))
    rng = np.random.default_rng(1)
    b = scn.beams[0].replace(spotWeights=20.0 + 80.0 * rng.random(scn.beams[0].spotWeights.shape))
    g = rng.random(scn.ct.shape).astype(np.float32)
    stage_identities(rig_of(scn, options(0.0)), b, g, 1e-5)


CASES = ["row_sweep", "radii_above_16", "water_uniform", "beam_along_x", "finite_source", "infinite_source"]


@pytest.mark.parametrize("case", CASES)
def test_end_to_end_dot_product(rig_of, synth, case):
    """<D(w + delta) - D(w), g> = <delta, grad(w)> for random delta >= 0 and signed g, on every superposition / transfer path."""
    if case == "row_sweep":
        scn = hetero_scene(synth, 96, [0.0])
    elif case == "radii_above_16":
        scn = radii_above_16(synth)
    elif case == "water_uniform":
        scn = scenarios.water_cube(synth, n=96, n_layers=3, spots=6, pitch=5.0)
    elif case == "beam_along_x":
        scn = hetero_scene(synth, 96, [90.0])
        # the host routes a transfer to k_transfer_t when the BEV x index moves more than 0.8x as fast along dose y or z as along x
        # (rtd_engine.hip, kTransferAxisRatio): here it does not move along dose x at all
        m = np.linalg.inv(np.asarray(scn.beams[0].gantryToDoseIdx.m, dtype=np.float64))[0]   # gantry x per dose-index step
        assert max(abs(m[1]), abs(m[2])) > 100.0 * abs(m[0])
    elif case == "finite_source":
        scn = hetero_scene(synth, 96, [20.0], source_dist=(1800.0, 2100.0))
    else:
        scn = hetero_scene(synth, 96, [20.0])
    g = (np.random.default_rng(3).random(scn.ct.shape) - 0.3).astype(np.float32)
    rig = rig_of(scn, options(0.0))
    info = end_to_end(rig, scn.beams[0], g, seed=4)
    if case == "radii_above_16":
        assert info["max_radius"] > 16
    if case == "water_uniform":
        assert info["uniform_sigma"] == 1
    else:
        assert info["uniform_sigma"] == 0


def test_zero_weight_spots(rig_of, synth):
    """Spots of weight 0 have the gradient their dose would have: the finite difference (<D(w + h e_i) - D(w), g>) / h equals
    grad_i, and is > 0 with g > 0. The first five of the nine rows of the map are zero in EVERY layer, so the forward's extents that
    follow the rays that carry dose — actUnion, bevLo / bevHi, the dose box (tbox) and the transfer's early-out, unions over all
    layers and steps — stay well away from the edge row: the test first checks that a good part of those spots' dose lies outside
    the dose box of D(w), i.e. that an adjoint culled with any of those extents would fail here. An interior spot of weight 0 sits
    among its neighbours."""
    scn = hetero_scene(synth, 96, [15.0], spots=(6, 9), pitch=7.0, layers=2)
    b = scn.beams[0]
    w = b.spotWeights.copy()
    w[:, :5, :] = 0.0                                                # rows 0 .. 4, in every layer
    w[1, 6, 3] = 0.0                                                 # an interior spot
    b = b.replace(spotWeights=w)
    g = (0.1 + np.random.default_rng(8).random(scn.ct.shape)).astype(np.float32)
    rig = rig_of(scn, options(0.0))
    f = rig.field(b)
    d0, info, _ = rig.compute(f)
    lo, hi = info["dose_box_min"], info["dose_box_max"]               # [x, y, z]; arrays are [z][y][x]
    inside = np.zeros(scn.ct.shape, dtype=bool)
    inside[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    grad = rig.grad(f, g)
    h = 50.0
    for idx, edge in [((1, 0, 2), True), ((0, 0, 4), True), ((1, 1, 0), True), ((1, 6, 3), False)]:
        w1 = w.copy()
        w1[idx] += h
        dd = rig.dose(b.replace(spotWeights=w1)).astype(np.float64) - d0.astype(np.float64)
        fd, scale = dot(dd, g)
        if edge:                                                     # the guard is not hollow: the box of D(w) misses much of this spot's dose
            outside = float(np.dot(np.abs(dd[~inside]), g[~inside].astype(np.float64)))
            assert outside > 0.05 * scale, (idx, outside, scale)
        assert grad[idx] > 0, idx
        assert abs(fd / h - float(grad[idx])) <= 1e-4 * scale / h, (idx, fd / h, float(grad[idx]))


def test_independent_of_the_gpu_forward(rig_of, synth, orc):
    """The identity of the end-to-end test with D from the CPU oracle (C1 size: water 128^3, one layer)."""
    scn = scenarios.water_cube(synth, n=128, n_layers=1)
    opt = options(0.0)
    b = scn.beams[0]
    rng = np.random.default_rng(12)
    delta = (0.5 * b.spotWeights * rng.random(b.spotWeights.shape)).astype(np.float32)
    g = (rng.random(scn.ct.shape) - 0.4).astype(np.float32)
    rig = rig_of(scn, opt)
    f = rig.field(b)
    rig.compute(f)
    grad = rig.grad(f, g)
    d0 = orc.compute(scn, options=opt)
    scn1 = scenarios.Scenario("c1 + delta", scn.luts, scn.ct, scn.spacing, [b.replace(spotWeights=b.spotWeights + delta)])
    d1 = orc.compute(scn1, options=opt)
    close(dot(d1.astype(np.float64) - d0.astype(np.float64), g), dot(delta, grad), 1e-4)


def test_default_cutoff_keeps_the_stage_identities(rig_of, synth):
    """With ray_weight_cutoff = 1 some rays are dead (their weights are below it): the identities still hold."""
    scn = hetero_scene(synth, 96, [30.0], source_dist=(2000.0, 2300.0))
    rng = np.random.default_rng(2)
    b = scn.beams[0].replace(spotWeights=20.0 + 80.0 * rng.random(scn.beams[0].spotWeights.shape))
    g = rng.random(scn.ct.shape).astype(np.float32)
    f, _, _, _ = stage_identities(rig_of(scn, options(1.0)), b, g, 1e-5)
    rw = f.fetch("ray_weights")
    assert (rw < 1.0).any() and (rw >= 1.0).any()


def test_reproducible_and_without_side_effects(rig_of, synth):
    """Two gradient calls give identical bits; the field's BEV dose and what it transfers afterwards are unchanged; calls with
    different g are independent."""
    scn = hetero_scene(synth, 96, [30.0])
    b = scn.beams[0]
    rng = np.random.default_rng(6)
    g1 = rng.random(scn.ct.shape).astype(np.float32)
    g2 = (rng.random(scn.ct.shape) - 0.5).astype(np.float32)
    rig = rig_of(scn, options(0.0))
    f = rig.field(b)
    dose, _, _ = rig.compute(f)
    bev0 = f.fetch("bev").copy()
    a = rig.grad(f, g1)
    c = rig.grad(f, g2)
    a2 = rig.grad(f, g1)
    assert np.abs(a).max() > 0
    assert np.array_equal(a.view(np.uint32), a2.view(np.uint32))
    assert not np.array_equal(a, c)
    assert np.array_equal(f.fetch("bev").view(np.uint32), bev0.view(np.uint32))
    rig.eng.device_zero(rig.dDose, rig.nb)
    f.transfer(rig.dDose)
    f.finish()
    again = np.empty(rig.shape, dtype=np.float32)
    rig.eng.to_host(again, rig.dDose)
    assert np.array_equal(again.view(np.uint32), dose.view(np.uint32))


def test_host_form_equals_the_field_calls(rig_of, synth):
    """rtd_spot_gradient over two beams = the per-field gradients, bit for bit, in beam order."""
    ct, _ = scenarios.hetero_phantom(96)
    scn = scenarios.hetero_ct(synth, n=96, spots=5, pitch=8.0, n_layers=2, angles=[0.0, 70.0], ct=ct)
    g = np.random.default_rng(9).random(scn.ct.shape).astype(np.float32)
    rig = rig_of(scn, options(0.0))
    per = []
    for b in scn.beams:
        f = rig.field(b)
        rig.compute(f)
        per.append(rig.grad(f, g))
    host = rig.eng.spot_gradient(scn.beams, g)
    assert len(host) == 2
    for p, q in zip(per, host):
        assert p.shape == q.shape and np.abs(p).max() > 0
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32))


def test_errors(engine, synth):
    """NOT_READY before a compute; INVALID_ARG for null pointers, remote fields and nuclear_corr; a radius overflow of the forward
    is reported."""
    scn = hetero_scene(synth, 64, [0.0], spots=3, layers=1)
    b = scn.beams[0]
    eng = engine.Engine(0)
    try:
        eng.set_options(options(0.0))
        eng.set_luts(synth)
        eng.set_ct(scn.ct)
        dims = (64, 64, 64)
        nb = 64 ** 3 * 4
        dG, dOut, dDose = eng.device_alloc(nb), eng.device_alloc(4096), eng.device_alloc(nb)
        eng.device_zero(dG, nb)
        f = eng.create_field(b, dims)
        with pytest.raises(engine.RtdError) as e:
            f.spot_gradient(dG, dOut)
        assert e.value.status == abi.RTD_ERR_NOT_READY
        eng.device_zero(dDose, nb)
        f.compute(dDose)
        f.finish()
        for args in [(0, dOut), (dG, 0)]:
            with pytest.raises(engine.RtdError) as e:
                f.spot_gradient(*args)
            assert e.value.status == abi.RTD_ERR_INVALID_ARG
        f.spot_gradient(dG, dOut)
        eng.sync()
        r = eng.create_field(b, dims, remote=True)
        with pytest.raises(engine.RtdError) as e:
            r.spot_gradient(dG, dOut)
        assert e.value.status == abi.RTD_ERR_INVALID_ARG
        r.destroy()
        f.destroy()
        # radius overflow (0.05 mm rays: radius > 32), reported like rtd_field_finish reports it
        big = scenarios.make_field(synth, 32, 8.0, (-128.0, -128.0, -106.0), 0.0, 3, 1.0, 1, 5, ray_spacing=(0.05, 0.05), steps=256, weight_lo=1e5)
        ct32 = np.full((32, 32, 32), 1000.0, dtype=np.float32)
        eng.set_ct(ct32)
        fo = eng.create_field(big, (32, 32, 32))
        eng.device_zero(dDose, 32 ** 3 * 4)
        fo.compute(dDose)
        with pytest.raises(engine.RtdError) as e:
            fo.spot_gradient(dG, dOut)
        assert e.value.status == abi.RTD_ERR_RADIUS_OVERFLOW
        fo.destroy()
        for p in (dG, dOut, dDose):
            eng.device_free(p)
    finally:
        eng.close()
    # nuclear_corr: refused
    from raytracedicom_amd import luts
    nl = luts.synth_luts(nuclear=True)
    scn = scenarios.water_cube(nl, n=64, n_layers=1, spots=5, pitch=6.0)
    eng = engine.Engine(0)
    try:
        opt = options(0.0)
        opt.nuclear_corr = abi.RTD_NUC_SOUKUP
        eng.set_options(opt)
        eng.set_luts(nl)
        eng.set_ct(scn.ct)
        nb = 64 ** 3 * 4
        dG, dOut, dDose = eng.device_alloc(nb), eng.device_alloc(4096), eng.device_alloc(nb)
        f = eng.create_field(scn.beams[0], (64, 64, 64))
        eng.device_zero(dDose, nb)
        f.compute(dDose)
        f.finish()
        with pytest.raises(engine.RtdError) as e:
            f.spot_gradient(dG, dOut)
        assert e.value.status == abi.RTD_ERR_INVALID_ARG
        f.destroy()
        for p in (dG, dOut, dDose):
            eng.device_free(p)
    finally:
        eng.close()


def test_projected_gradient_descent(rig_of, synth):
    """Optimiser smoke test: 96^3 heterogeneous field, target D* = D(w_true), start from uniform weights; ten steps of projected
    gradient descent on f(w) = 1/2 |D(w) - D*|^2 with exact line search. f decreases at every step and ends at most half its start."""
    scn = hetero_scene(synth, 96, [0.0], spots=5, pitch=8.0, layers=3)
    b = scn.beams[0]
    rng = np.random.default_rng(21)
    w_true = (40.0 + 120.0 * rng.random(b.spotWeights.shape)).astype(np.float32)
    rig = rig_of(scn, options(0.0))
    target = rig.dose(b.replace(spotWeights=w_true)).astype(np.float64)
    w = np.full(w_true.shape, float(w_true.mean()), dtype=np.float32)

    def objective(wv):
        f = rig.field(b.replace(spotWeights=wv))
        d, _, _ = rig.compute(f)
        r = d.astype(np.float64) - target
        return f, d.astype(np.float64), r, 0.5 * float(np.dot(r.reshape(-1), r.reshape(-1)))

    f, d, r, fv = objective(w)
    f0 = fv
    for _ in range(10):
        grad = rig.grad(f, r.astype(np.float32)).astype(np.float64)
        step = -grad
        step[(w <= 0.0) & (step < 0.0)] = 0.0                        # bound-active spots stay at 0
        # A step (D is linear in w >= 0 with cut-off 0): A p = D(p+) - D(p-)
        pp, pm = np.maximum(step, 0.0), np.maximum(-step, 0.0)
        ap = rig.dose(b.replace(spotWeights=pp)).astype(np.float64) - rig.dose(b.replace(spotWeights=pm)).astype(np.float64)
        t = -float(np.dot(r.reshape(-1), ap.reshape(-1))) / float(np.dot(ap.reshape(-1), ap.reshape(-1)))
        neg = step < 0.0
        if neg.any():
            t = min(t, float(np.min(w[neg] / -step[neg])))           # stay feasible: a shorter step along a descent direction still descends
        w = np.maximum(w + t * step, 0.0).astype(np.float32)
        f, d, r, fn = objective(w)
        assert fn < fv, (fn, fv)
        fv = fn
    assert fv <= 0.5 * f0, (fv, f0)


def test_stage_identities_full_size(rig_of, synth):
    """Test 1's identities on the C3 bench field (512^3 heterogeneous CT, 10x10 spots x 20 layers)."""
    scn = scenarios.hetero_ct(synth, n=512)
    b = scn.beams[0]
    g = np.random.default_rng(31).random(scn.ct.shape, dtype=np.float32)
    stage_identities(rig_of(scn, options(0.0)), b, g, 1e-5)
