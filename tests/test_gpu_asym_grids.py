"""GPU tests of the dose path, its transposes, the dose-influence matrix and the optimiser on a non-cubic CT with a dose grid of its
own (tests/asym_scenes.py): CT 90 x 61 x 103 voxels of 2.0 x 2.5 x 1.5 mm; dose grids 45 x 52 x 37 (coarser, inside the CT) and
150 x 70 x 77 (finer, overhanging it), each with its own voxel sizes and origin; spot map off the axis, sigma_y = 1.4 sigma_x.
tests/test_asym_scenes_reference.py pins, on the CPU, that these scenes exercise what they are meant to.

No tolerance is new: every comparison uses the helper and the bound of the test of the same operation on cubes (named at each test)."""
import numpy as np
import pytest

import asym_scenes as S
import dvh_reference as D
import optimizer_reference as R
from gpu_support import (FieldRig, bits, box_mask, col_bound, compare_field, compare_nuclear_field, end_to_end, gamma, nuc_luts,  # noqa: F401
                         rel_close, row_bound, stage_identities, worst_ratio)

pytestmark = pytest.mark.gpu

NAN_BITS = np.float32(np.nan).view(np.uint32)


@pytest.fixture(scope="module")
def oracle_dose(orc, synth):
    """(name, cut-off) -> (scene, the oracle's dose of its first beam into zeros): computed once, shared, not to be written to."""
    cache = {}

    def get(name, cutoff=None):
        if (name, cutoff) not in cache:
            scn = S.scene(synth, name)
            ref = np.zeros(scn.dose_shape, dtype=np.float32)
            of = orc.run_field(scn, scn.beams[0], ref, options=S.options(name, cutoff), keep_layers=False, dose_dims=scn.dose_dims)
            assert of.status == 0, of.error
            of.close()
            ref.setflags(write=False)
            cache[(name, cutoff)] = (scn, ref)
        return cache[(name, cutoff)]
    return get


def _box(shape, lo, hi):
    m = np.zeros(shape, dtype=bool)
    m[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    return m


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- forward, by stage

@pytest.mark.parametrize("name", ["A", "B", "C", "D", "F", "H", "W", "U"])
def test_stage_parity_with_the_oracle(orc, engine, synth, name):
    """gpu_support.compare_field, every assertion of it, with the dose grid apart from the CT's: tracer outputs, ray weights,
    first_passive, tile and batch radii bit-exact; layer_plan 1e-6; idd, 1/sigma 2e-5; BEV, dose 1e-4; gamma 100 % with the dose
    grid's own anisotropic spacing. F has radii above 16 (second sweep launch); U is the one scene with one sigma per slice (the
    separable kernels); W, water as well, is not: its oblique divergent beam has per-ray sigmas."""
    scn = S.scene(synth, name)
    dose, ref, _, info = compare_field(orc, engine, scn, scn.beams[0], dose_dims=scn.dose_dims, dose_spacing=scn.dose_spacing)
    assert dose.shape == scn.dose_shape and dose.max() > 0
    assert info["uniform_sigma"] == (1 if name == "U" else 0)
    if name == "F":
        assert info["max_radius"] > 16


def test_stage_parity_with_nuclear_correction(orc, engine, nuc_luts):
    """Scene N: W with the nuclear tables and RTD_NUC_SOUKUP, through test_gpu_nuclear's comparison (radius classes bit-exact, idd 2e-5,
    dose 1e-4 / 2e-5 of the maximum, gamma 100 %)."""
    scn = S.scene(nuc_luts, "N")
    dose, ref, info = compare_nuclear_field(orc, engine, scn, S.options("N"), dose_dims=scn.dose_dims, dose_spacing=scn.dose_spacing)
    assert dose.shape == scn.dose_shape
    assert info["beam_first_inside"] == 0                             # the beam starts in the water: the halo's slice 0 is deposited


# ------------------------------------------------------------------------------------------------------- host side: CT box, z-slabs

@pytest.mark.parametrize("name", ["A", "D"])
def test_deferred_ct_upload_on_the_non_cubic_ct(engine, synth, name):
    """test_gpu_multi.test_deferred_ct_uploads_only_what_the_rays_cross on the 90 x 61 x 103 CT: the device volume is poisoned with
    NaN, then each field uploads the CT box its tracer samples; the dose (onto a random base, on the coarse grid) equals the direct
    upload bit for bit."""
    scn = S.scene(synth, name)
    base = (1e-7 * np.random.default_rng(3).random(scn.dose_shape)).astype(np.float32)
    want = base.copy()
    with engine.Engine(0) as eng:
        eng.set_luts(scn.luts)
        eng.set_ct(scn.ct)
        eng.compute(scn.beams, want)
    assert (want > base).any()
    got = base.copy()
    with engine.Engine(0) as eng:
        eng.set_luts(scn.luts)
        eng.set_ct(np.full_like(scn.ct, np.nan))
        eng.set_ct(scn.ct, deferred=True)
        eng.compute(scn.beams, got)
    np.testing.assert_array_equal(got, want)


def test_reference_shaped_call_and_in_process_plan(orc, engine, synth):
    """Two beams (A and H) on the coarse grid: rtd_compute against orc_compute (rel_close, 1e-4); rtd_plan_compute with two and three
    handles equal to it bit for bit — 37 dose slices give uneven z-slabs."""
    scn = S.scene(synth, "AH")
    assert scn.dose_dims == (45, 52, 37)
    base = np.full(scn.dose_shape, 1e-7, dtype=np.float32)
    ref = orc.compute(scn, dose=base.copy(), dose_dims=scn.dose_dims)
    want = base.copy()
    with engine.Engine(0) as eng:
        eng.set_luts(scn.luts)
        eng.set_ct(scn.ct)
        eng.compute(scn.beams, want)
    assert want.max() > 1e-6
    rel_close(want, ref, rtol=1e-4)
    for devices in ([0, 0], [0, 0, 0]):
        got = base.copy()
        with engine.Plan(devices) as plan:
            plan.set_luts(scn.luts)
            plan.set_ct(scn.ct)
            _, pt = plan.compute(scn.beams, got)
            assert pt["n_devices"] == len(devices)
        np.testing.assert_array_equal(got, want, err_msg="%d handles" % len(devices))


# ------------------------------------------------------------------------------------------------------------------------ transfers

def test_transfers_and_clip_boxes(engine, synth, oracle_dose):
    """Fields A and H on the coarse grid (k_transfer<INIT>, k_transfer / k_transfer_t, k_clear_box, k_transfer_multi with nx != ny != nz):
    transfer_init into a NaN-filled volume and transfer onto a random base against the oracle's dose (rel_close, 1e-4); the same two
    clipped to the inclusive box (5, 3, 2)-(37, 44, 30) — six different bounds, none on a brick edge — change nothing outside it and
    give the unclipped bits inside; clear_dose_box zeroes the part of the dose box inside it and nothing else; transfer_fields_init of
    both fields equals transfer_init + transfer bit for bit, on the whole grid and in the box."""
    refs = [oracle_dose("A")[1], oracle_dose("H")[1]]
    scn = S.scene(synth, "AH")
    shape, n = scn.dose_shape, scn.n_dose_voxels
    lo, hi = S.CLIP_BOX
    clip = _box(shape, lo, hi)
    nans = np.full(shape, np.nan, dtype=np.float32)
    base = (1e-7 * np.random.default_rng(5).random(shape)).astype(np.float32)
    with engine.Engine(0) as eng:
        eng.set_luts(scn.luts)
        eng.set_ct(scn.ct)
        d = eng.device_alloc(4 * n)
        fields = [eng.create_field(b, scn.dose_dims) for b in scn.beams]

        def run(start, call, *args):
            eng.to_device(d, start)
            call(d, *args)
            eng.sync()
            out = np.empty(shape, dtype=np.float32)
            eng.to_host(out, d)
            return out
        for f, ref in zip(fields, refs):
            f.compute_bev()
            info, _ = f.wait_plan()
            box = _box(shape, info["dose_box_min"], info["dose_box_max"])
            assert (box & clip).any() and (box & ~clip).any()
            init = run(nans, f.transfer_init)
            assert (init.view(np.uint32)[~box] == NAN_BITS).all() and np.isfinite(init[box]).all()
            rel_close(np.where(box, init, np.float32(0.0)), ref, rtol=1e-4)
            acc = run(base, f.transfer)
            rel_close(acc, base + ref, rtol=1e-4)
            assert _same_bits(acc[~box], base[~box])
            # clipped: outside the box nothing changes, inside it the unclipped bits
            init_c = run(nans, f.transfer_init, lo, hi)
            assert (init_c.view(np.uint32)[~clip] == NAN_BITS).all() and _same_bits(init_c[clip], init[clip])
            acc_c = run(base, f.transfer, lo, hi)
            assert _same_bits(acc_c[~clip], base[~clip]) and _same_bits(acc_c[clip], acc[clip])
            assert (acc_c[clip] != base[clip]).any()
            cleared = run(base, f.clear_dose_box, lo, hi)
            want = base.copy()
            want[clip & box] = 0.0
            assert _same_bits(cleared, want)
        # both fields in one launch
        eng.device_zero(d, 4 * n)
        fields[0].transfer_init(d)
        fields[1].transfer(d)
        eng.sync()
        seq = np.empty(shape, dtype=np.float32)
        eng.to_host(seq, d)
        assert seq.max() > 0
        multi = run(nans, lambda p: eng.transfer_fields_init(fields, p))
        assert _same_bits(multi, seq)
        multi_c = run(nans, lambda p: eng.transfer_fields_init(fields, p, lo, hi))
        assert (multi_c.view(np.uint32)[~clip] == NAN_BITS).all() and _same_bits(multi_c[clip], seq[clip])
        for f in fields:
            f.finish()
            f.destroy()
        eng.device_free(d)


# ------------------------------------------------------------------------------------------------------------------ transposed path

@pytest.mark.parametrize("name", ["A", "C", "F", "W", "U"])
def test_transposed_path(engine, synth, name):
    """test_gpu_gradient's stage identities (<g, D> = <grad_bev, bev> = <grad_ray_weights, ray_weights> = <grad, w>) and end-to-end
    identity (<D(w + delta) - D(w), g> = <delta, grad>) at their 1e-5, cut-off 0, g random and signed on the dose grid: k_adj_transfer
    and the adjoint superposition with the dose dims apart from the CT's. U takes the separable kernels, F radii above 16."""
    scn = S.scene(synth, name)
    g = (np.random.default_rng(3).random(scn.dose_shape) - 0.3).astype(np.float32)
    rig = FieldRig(engine, scn, S.options(name, cutoff=0.0), dims=scn.dose_dims)
    try:
        assert rig.dims == scn.dose_dims
        _, _, _, info = stage_identities(rig, scn.beams[0], g, 1e-5)
        assert info["uniform_sigma"] == (1 if name == "U" else 0)
        if name == "F":
            assert info["max_radius"] > 16
        end_to_end(rig, scn.beams[0], g, seed=4, tol=1e-5)
    finally:
        rig.close()


def test_host_form_of_the_gradient(engine, synth):
    """rtd_spot_gradient over beams A and H with g on the coarse grid = the per-field gradients bit for bit, in beam order (the bar of
    test_gpu_gradient.test_host_form_equals_the_field_calls)."""
    scn = S.scene(synth, "AH")
    g = (np.random.default_rng(9).random(scn.dose_shape) - 0.3).astype(np.float32)
    rig = FieldRig(engine, scn, S.options(cutoff=0.0), dims=scn.dose_dims)
    try:
        per = []
        for b in scn.beams:
            f = rig.field(b)
            rig.compute(f)
            per.append(rig.grad(f, g))
        host = rig.eng.spot_gradient(scn.beams, g)
        assert len(host) == 2
        for p, q in zip(per, host):
            assert p.shape == q.shape and np.abs(p).max() > 0
            assert _same_bits(p, q)
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------ Dij and its products

@pytest.mark.parametrize("name", ["A", "F"])
def test_dose_influence_and_its_products(engine, synth, oracle_dose, name):
    """On the coarse grid (gather, clear-box and k_dijap kernels with nx != ny): columns are single-spot doses (1e-6 of the column
    maximum, test_columns_are_single_spot_doses); Dij w is the oracle's dose at cut-off 0 (1e-4 of the maximum,
    test_against_the_cpu_oracle); apply(w) is the forward and apply_t(g) the gradient (bounds of test_apply_is_the_forward /
    test_apply_t_is_the_gradient); apply(init = 1) into NaNs writes the dose box and nothing else."""
    scn, ref = oracle_dose(name, 0.0)
    b = scn.beams[0]
    rig = FieldRig(engine, scn, S.options(name, cutoff=0.0), dims=scn.dose_dims)
    try:
        f = rig.field(b)
        d = f.dose_influence()
        _, info = f.finish()
        assert d.shape == (scn.n_dose_voxels, b.spotWeights.size) and d.nnz > 0
        assert d.indices.min() >= 0 and d.indices.max() < scn.n_dose_voxels
        # against the oracle
        a = d.matvec(b.spotWeights)
        r64 = ref.reshape(-1).astype(np.float64)
        assert float(np.abs(a - r64).max()) <= 1e-4 * float(r64.max())
        # columns: a corner spot of the first layer, the opposite corner of the last, an interior spot
        L, ny, nx = b.spotWeights.shape
        for p in [(0, 0, 0), (L - 1, ny - 1, nx - 1), (1, 1, 2)]:
            e = np.zeros(b.spotWeights.shape, dtype=np.float32)
            e[p] = 1.0
            dense = rig.dose(b.replace(spotWeights=e)).reshape(-1)
            col = np.zeros(d.shape[0], dtype=np.float32)
            rows, vals = d.column((p[0] * ny + p[1]) * nx + p[2])
            col[rows] = vals
            assert dense.max() > 0, p
            assert float(np.abs(col - dense).max()) <= 1e-6 * float(dense.max()), (p, float(np.abs(col - dense).max()), float(dense.max()))
        # apply = the forward at other weights
        w = (b.spotWeights * (0.5 + np.random.default_rng(11).random(b.spotWeights.shape))).astype(np.float32)
        dw, _, _ = rig.compute(rig.field(b.replace(spotWeights=w)))
        fwd = dw.reshape(-1).astype(np.float64)
        got = rig.product(f, w)
        nr, sr = row_bound(d, w)
        err = np.abs(got.astype(np.float64) - fwd)
        assert fwd.max() > 0 and np.all(err <= 1e-5 * fwd.max() + gamma(nr) * sr), float(np.max(err - gamma(nr) * sr)) / fwd.max()
        # apply(init = 1) into NaNs: the dose box is written (sum or 0), nothing outside it
        box = box_mask(rig, info)
        assert box.any()
        into_nan = rig.apply(f, w)
        assert (into_nan.view(np.uint32)[~box] == NAN_BITS).all()
        assert _same_bits(into_nan[box], got.reshape(rig.shape)[box])
        assert (got.reshape(rig.shape)[~box] == 0).all()
        # apply_t = the gradient
        g = (np.random.default_rng(6).random(rig.shape) - 0.3).astype(np.float32)
        grad = rig.grad(f, g).reshape(-1).astype(np.float64)
        got_t = rig.apply_t(f, g).reshape(-1).astype(np.float64)
        nc, sc = col_bound(d, g)
        assert (sc > 0).sum() > 0
        err_t = np.abs(got_t - grad)
        assert np.all(err_t <= (1e-5 + gamma(nc)) * sc + 1e-30), worst_ratio(err_t, (1e-5 + gamma(nc)) * sc)
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------------------ optimiser

def test_optimizer_and_dvh_on_the_coarse_grid(engine, synth):
    """Fields A and H with their matrices on the 45 x 52 x 37 grid; a target ROI (a 7 x 5 x 3 box in the high-dose region) and an
    organ-at-risk ROI (a 9 x 9 x 5 box beside it), both given as linear indices (x fastest). Ten iterations, each against
    tests/optimizer_reference.py as test_gpu_optimizer.test_one_iteration_against_the_restatement compares one: f within the summation
    bound of the objective, alpha within (n + 2) * 2^-52, the new weights bit for bit. Every iteration the optimiser's volume is the
    zeroed volume + apply(init = 0) of the fields at the weights that entered it, bit for bit (k_opt_clear_box with nx != ny). The
    cumulative DVH of the final dose against tests/dvh_reference.py, count for count."""
    scn = S.scene(synth, "AH")
    nx, ny, nz = scn.dose_dims
    nvox = scn.n_dose_voxels
    eng = engine.Engine(0)
    bufs, fields, opt, obj = [], [], None, None

    def alloc(nbytes):
        bufs.append(eng.device_alloc(nbytes))
        return bufs[-1]
    try:
        eng.set_options(S.options(cutoff=0.0))
        eng.set_luts(scn.luts)
        eng.set_ct(scn.ct)
        fields = [eng.create_field(b, scn.dose_dims) for b in scn.beams]
        mats = [f.dose_influence() for f in fields]
        shapes = [b.spotWeights.shape for b in scn.beams]
        sizes = [int(np.prod(s)) for s in shapes]
        n = sum(sizes)
        w_true = [(40.0 + 120.0 * np.random.default_rng(21 + i).random(s)).astype(np.float32) for i, s in enumerate(shapes)]
        vol = sum(m.matvec(w) for m, w in zip(mats, w_true)).reshape(scn.dose_shape)
        mx = float(vol.max())
        cz, cy, cx = (int(round(float(v.mean()))) for v in np.nonzero(vol > 0.5 * mx))
        k, j, i = np.meshgrid(np.arange(cz - 1, cz + 2), np.arange(cy - 2, cy + 3), np.arange(cx - 3, cx + 4), indexing="ij")
        target = np.sort(((k * ny + j) * nx + i).reshape(-1))
        k, j, i = np.meshgrid(np.arange(cz - 1, cz + 4), np.arange(cy - 2, cy + 7), np.arange(cx + 5, cx + 14), indexing="ij")
        assert k.max() < nz and j.max() < ny and i.max() < nx and min(k.min(), j.min(), i.min()) >= 0
        oar = np.sort(((k * ny + j) * nx + i).reshape(-1))
        flat = vol.reshape(-1)
        assert flat[target].min() > 0.25 * mx and flat[oar].mean() > 0.02 * mx and not np.intersect1d(target, oar).size
        level = float(flat[target].mean())
        obj = eng.create_objective(scn.dose_dims)
        ref = D.DvhReferenceObjective(nvox)
        for roi in (target, oar):
            obj.add_roi(roi)
            ref.add_roi(roi)
        for t in [(R.SQ_DEVIATION, 0, 1.0, level), (R.SQ_UNDERDOSE, 0, 5.0, 0.95 * level), (R.SQ_OVERDOSE, 1, 1.0, 0.3 * level),
                  (R.MEAN, 1, 1e-3 * level, 0.0)]:
            obj.add_term(*t)
            ref.add_term(*t)
        opt = eng.create_optimizer(fields, obj)
        dG, dDose = alloc(4 * nvox), alloc(4 * nvox)
        eng.device_zero(dG, 4 * nvox)
        dGrad = [alloc(4 * s) for s in sizes]
        dW = [alloc(4 * s) for s in sizes]
        nmax = max(r.size for r in ref.rois)
        w_prev = grad_prev = None
        f_best = np.inf
        dose = np.empty(nvox, dtype=np.float32)
        for it in range(10):
            ws = [opt.weights(q) for q in range(2)]
            w = np.concatenate([x.reshape(-1) for x in ws])
            opt.run(1)
            rep, hist = opt.result()
            eng.to_host(dose, opt.dose())
            # the optimiser's volume = zero + apply(init = 0) per field in list order at the weights that entered the iteration
            eng.device_zero(dDose, 4 * nvox)
            for f, p, x in zip(fields, dW, ws):
                eng.to_device(p, x)
                f.dose_influence_apply(p, dDose, init=False)
            seq = np.empty(nvox, dtype=np.float32)
            eng.to_host(seq, dDose)
            assert seq.max() > 0 and _same_bits(dose, seq), it
            vals = obj.eval(opt.dose(), dG)
            grad = []
            for f, p, s in zip(fields, dGrad, sizes):
                f.dose_influence_apply_t(dG, p)
                grad.append(np.empty(s, dtype=np.float32))
                eng.to_host(grad[-1], p)
            grad = np.concatenate(grad)
            assert rep["iterations"] == it + 1 and hist.size == it + 1 and hist[it] == rep["f_last"] == vals[0]
            f_ref = ref.eval(dose)[0][0]
            assert abs(hist[it] - f_ref) <= (nmax + 4) * 2.0 ** -52 * f_ref
            f_best = min(f_best, hist[it])
            assert rep["f_best"] == f_best and hist[rep["best_iteration"]] == f_best and rep["guarded"] == 0
            a_ref = R.step_length(w, w_prev, grad, grad_prev, it > 0)
            rel = abs(rep["step"] - a_ref) / a_ref
            print("iteration %d: f %.9g, alpha %.17g on the device, %.17g restated: relative difference %.3g of the bound %.3g"
                  % (it, hist[it], rep["step"], a_ref, rel, (n + 2) * 2.0 ** -52))
            assert a_ref > 0 and rel <= (n + 2) * 2.0 ** -52
            w_new = np.concatenate([opt.weights(q).reshape(-1) for q in range(2)])
            assert np.array_equal(bits(w_new), bits(R.update(w, grad, rep["step"])))
            assert not np.array_equal(w_new, w)
            w_prev, grad_prev = w, grad
        # the DVH of the volume of the last iteration
        top = float(dose.max())
        for n_bins, dose_max in ((100, 0.6 * top), (333, 1.01 * top)):
            got = obj.dvh(opt.dose(), n_bins, dose_max)
            assert got.shape == (2, n_bins) and got.dtype == np.uint32
            np.testing.assert_array_equal(got, ref.dvh(dose, n_bins, dose_max))
            assert list(got[:, 0]) == [target.size, oar.size]
    finally:
        if opt is not None:
            opt.destroy()
        if obj is not None:
            obj.destroy()
        for p in bufs:
            eng.device_free(p)
        for f in fields:
            f.destroy()
        eng.close()
