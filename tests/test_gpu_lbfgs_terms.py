"""GPU tests of rtd_optimizer_create_lbfgs_ex (include/rtd.h "L-BFGS with DVH and EUD terms, and on the compact matrix", DESIGN.md
section 30): the K trials of the line search against rtd_objective_eval, _dose_at_volume and _eud on the float32 trial volumes, the
exact chain from an accepted trial to the next history entry, the numpy restatement for plain + DVH terms, the shapes at which the
K-wide kernels take another path, the compact products, residency and the refusals."""
import ctypes as C

import numpy as np
import pytest

import eud_reference as E
import lbfgs_reference as LB
import optimizer_reference as R
from gpu_support import bits, hetero_scene, rig_fixture
from lbfgs_rig import chunk_scene, lbfgs_options
from lbfgs_terms_rig import LbfgsTermsRig, check_products, check_trials, step_terms
from raytracedicom_amd import abi, rbe as rbe_models

pytestmark = pytest.mark.gpu

rig_of = rig_fixture(LbfgsTermsRig)


def scene(synth):
    return hetero_scene(synth, 64, (0.0,))


def overshoot_scale(make_ref, steps=6):
    """The natural run takes unit steps almost only: the first rule's scale times 4, 16, ... until the restatement made by
    make_ref(initial_step) backtracks as well as takes a unit step within `steps` iterations -> (scale, its accepted trials)."""
    first = make_ref(0.0).step()["delta"][-1]
    for j in range(1, 16):
        ref = make_ref(first * 4.0 ** j)
        marks = [ref.step()["k"] for _ in range(steps)]
        if any(k > 0 for k in marks) and any(k == 0 for k in marks):
            return first * 4.0 ** j, marks
    raise AssertionError("no scale at which the restatement backtracks and takes a unit step")


def plain_float64(rig, **kw):
    """The float64 restatement on the rig's reference objective with the host copies of the matrices (no device work)."""
    return lambda step: LB.LbfgsReference(rig.ref, rig.matvec, rig.rmatvec, np.zeros(rig.n), tree=False, initial_step=step, **kw)


@pytest.mark.parametrize("K", (1, 3, 8))
def test_trial_values_bit_for_bit(rig_of, synth, K):
    """The mixed objective, seven iterations from zero at a first scale where the line search backtracks: every F_k is
    rtd_objective_eval(r_k).values[0], every threshold the dose at volume of r_k, every E rtd_objective_eud(r_k), on the bits; the
    iteration's other quantities against the restatement fed those values."""
    rig = rig_of(scene(synth))
    rig.set_mixed()
    kw = dict(memory=3, max_halvings=K - 1)
    if K > 1:
        kw["initial_step"], marks = overshoot_scale(plain_float64(rig, **kw))
        print("first scale %.6g: the float64 restatement accepts %s" % (kw["initial_step"], marks))
    w0 = np.zeros(rig.n, dtype=np.float32)
    opt = rig.lbfgs_ex(start=0.0, **kw)
    ref = rig.value_restatement(w0, **kw)
    d0 = rig.product(w0)
    events = ""
    for k in range(7):
        out, d0 = step_terms(rig, opt, ref, k, d0, fresh=k == 0)
        events += LB.event_letter(out)
    print("K = %d: events %s" % (K, events))
    assert sum(c.isdigit() for c in events) >= 4, events
    if K > 1:
        assert any(c.isdigit() and c != "0" for c in events), "no backtracked step: %s" % events


def test_the_exact_chain(rig_of, synth):
    """Thirty run(1) from zero on the mixed objective: after an accepted trial k the next history entry is trial_values[k] on the bits,
    no history entry rises, f_best never increases, and every iteration is counted once."""
    rig = rig_of(scene(synth))
    rig.set_mixed()
    opt = rig.lbfgs_ex(start=0.0)
    pending, f_best, prev, accepted, idle = None, np.inf, None, 0, 0
    for i in range(30):
        opt.run(1)
        rep, hist = opt.result()
        lb = opt.lbfgs_report()
        assert hist.size == i + 1
        if pending is not None:
            np.testing.assert_array_equal(bits(hist[i:i + 1]), bits(np.array([pending])), "history[%d] is not the accepted trial value" % i)
        assert rep["f_best"] <= f_best, (i, rep["f_best"], f_best)
        f_best = rep["f_best"]
        counts = (lb["unit_steps"], lb["backtracked_steps"], lb["stalls"], lb["resets"])
        delta = sum(counts) - (sum(prev) if prev else 0)
        prev = counts
        if lb["last_trial"] >= 0:
            pending = lb["trial_values"][lb["last_trial"]]
            accepted += 1
            assert delta == 1, (i, counts)
        else:
            pending = None
            assert lb["last_step"] == 0.0 and delta in (0, 1), (i, counts)
            idle += delta == 0
    rep, hist = opt.result()
    lb = opt.lbfgs_report()
    rises = int((np.diff(hist) > 0).sum())
    print("history %.9g -> %.9g, accepted %d, report %s" % (hist[0], hist[-1], accepted, {k: lb[k] for k in ("unit_steps", "backtracked_steps", "halvings", "stalls", "resets")}))
    assert rises == 0, (rises, hist)
    assert lb["unit_steps"] + lb["backtracked_steps"] == accepted and accepted >= 10
    assert lb["unit_steps"] + lb["backtracked_steps"] + lb["stalls"] + lb["resets"] + idle == rep["iterations"] == 30
    assert hist[-1] < hist[0] and rep["f_best"] == hist.min()


def test_step_by_step_against_the_numpy_restatement(rig_of, synth):
    """Plain + DVH terms, where numpy restates the evaluation to the bit (the selection is an exact order statistic): weights, ring,
    Gram matrix, events, F_k and the updated dose against LbfgsTermsReference, at a first scale where the restatement alone, on the
    host copies of the matrices, takes a backtracked step and a unit step."""
    rig = rig_of(scene(synth))
    L = rig.level
    rig.set_terms([("plain", E.SQ_DEVIATION, 0, 1.0, L), ("dvh", E.MAX_DVH, 1, 2.0, 0.3 * L, 0.1), ("dvh", E.MIN_DVH, 0, 5.0, 0.95 * L, 0.98),
                   ("plain", E.MEAN, 1, 1e-3 * L, 0.0)], [rig.ref.rois[0], rig.ref.rois[1]])
    w0 = np.zeros(rig.n, dtype=np.float32)
    scale, marks = overshoot_scale(lambda step: rig.terms_restatement(w0, memory=3, initial_step=step))
    print("first scale %.6g: the restatement alone accepts %s" % (scale, marks))
    assert any(k > 0 for k in marks) and any(k == 0 for k in marks), marks
    opt = rig.lbfgs_ex(start=0.0, memory=3, initial_step=scale)
    ref = rig.terms_restatement(w0, memory=3, initial_step=scale)
    d0 = rig.product(w0)
    events = ""
    for k in range(6):
        out, d0 = step_terms(rig, opt, ref, k, d0, fresh=k == 0)
        events += LB.event_letter(out)
    print("events %s" % events)
    assert "0" in events and any(c.isdigit() and c != "0" for c in events), events


def _first(idx, n):
    assert idx.size >= n, (idx.size, n)
    return idx[:n]


def test_shapes_of_the_kernels(rig_of, synth):
    """ROIs at the edges of the K-wide kernels: one voxel with a DVH term, 4096 and 4097 voxels (kDvhChunk), 2048 and 2049 (kEudChunk),
    a union that is no multiple of 256, an ROI outside the field's row box (all +0 at every trial: the single-bin path). Four
    iterations, every trial against the evaluation on the bits."""
    rig = rig_of(scene(synth))
    L = rig.level
    has = np.flatnonzero(np.bincount(rig.mats[0].indices, minlength=rig.nvox) > 0)
    target, other = rig.ref.rois[0], rig.ref.rois[1]
    outside = _first(np.setdiff1d(np.arange(rig.nvox), has), 300)
    rois = [target, target[len(target) // 2:len(target) // 2 + 1], _first(other, 4096), _first(other, 4097), _first(has, 2048), _first(has[::-1][:2049][::-1], 2049), outside]
    terms = [("plain", E.SQ_DEVIATION, 0, 1.0, L), ("dvh", E.MIN_DVH, 1, 1.0, 0.95 * L, 1.0), ("dvh", E.MAX_DVH, 2, 2.0, 0.2 * L, 0.25),
             ("dvh", E.MAX_DVH, 3, 2.0, 0.2 * L, 0.001), ("eud", E.SQ_MAX_EUD, 4, 1.0, 0.3 * L, 4.0), ("eud", E.SQ_EUD, 5, 1.0, 0.5 * L, -2.0),
             ("dvh", E.MIN_DVH, 6, 1.0, 0.1 * L, 0.5), ("eud", E.SQ_MIN_EUD, 6, 1.0, 0.1 * L, 1.0)]
    rig.set_terms(terms, rois)
    n_union = int(rig.ref.union().sum())
    assert n_union % 256 != 0, n_union
    w0 = np.zeros(rig.n, dtype=np.float32)
    opt = rig.lbfgs_ex(start=0.0, memory=3, max_halvings=3)
    ref = rig.value_restatement(w0, memory=3, max_halvings=3)
    d0 = rig.product(w0)
    for k in range(4):
        out, d0 = step_terms(rig, opt, ref, k, d0, fresh=k == 0)
        assert not d0[outside].any()
    assert ref.unit + ref.backtracked >= 2


def test_a_nan_in_a_trial_volume(rig_of, synth):
    """A NaN weight through set_weights: d0 holds NaNs in the ROIs, so r_k does for k >= 1 (r_0 = d1 is finite: P sends a NaN to +0).
    The iteration is guarded; the trial values, thresholds and E still are those of the evaluation on r_k, on the bits."""
    rig = rig_of(scene(synth))
    rig.set_mixed()
    w = [np.full(s, 50.0, dtype=np.float32) for s in rig.shapes]
    w[0].reshape(-1)[w[0].size // 2] = np.nan
    opt = rig.lbfgs_ex(start=w, max_halvings=2)
    d0 = rig.product(np.concatenate([x.reshape(-1) for x in w]))
    assert np.isnan(d0[rig.ref.rois[0]]).any()
    opt.run(1)
    ln = rig.line(opt)
    assert np.array_equal(ln["d0"], d0, equal_nan=True), "the tracked dose of a guarded iteration is the product"
    assert not np.isnan(ln["d1"]).any()
    check_trials(rig, opt, ln["d0"], ln["d1"])
    lb = opt.lbfgs_report()
    assert lb["last_trial"] == -1 and np.isnan(lb["trial_values"][1])


def test_ex_is_create_lbfgs_where_it_can_be(rig_of, synth):
    """Flags 0 and a plain-only objective: 12 iterations on the chunk scene give the weights, best weights, history, report and dose
    of rtd_optimizer_create_lbfgs, on the bits; the line buffers then hold no threshold or EUD array."""
    rig = rig_of(chunk_scene(synth))
    a, b = rig.lbfgs(start=0.0), rig.lbfgs_ex(start=0.0)
    a.run(12)
    b.run(12)
    ra, ha = a.result()
    rb, hb = b.result()
    assert ra == rb and np.array_equal(bits(ha), bits(hb)) and a.lbfgs_report() == b.lbfgs_report(), (ra, rb)
    for best in (False, True):
        assert np.array_equal(bits(rig.all_weights(a, best)), bits(rig.all_weights(b, best)))
    assert np.array_equal(bits(rig.volume(a.dose())), bits(rig.volume(b.dose())))
    for o in (a, b):
        ln = rig.line(o)
        assert not ln["coupled"] and ln["K"] == 6 and ln["n_terms"] == 4
        assert np.array_equal(bits(ln["d0"]), bits(rig.volume(o.dose())))


@pytest.mark.parametrize("mixed", (False, True))
def test_compact(rig_of, synth, mixed):
    """RTD_LBFGS_COMPACT: 12 iterations equal the restatement driven with the public compact products (d1 and grad of every iteration
    are rtd_field_dose_influence_apply_compact / _apply_t_compact of w_full and of the evaluation's voxel gradient), on the bits."""
    rig = rig_of(scene(synth))
    if mixed:
        rig.set_mixed()
    rig.make_compact()
    w0 = np.zeros(rig.n, dtype=np.float32)
    opt = rig.lbfgs_ex(start=0.0, memory=3)
    ref = rig.value_restatement(w0, memory=3) if mixed else rig.restatement(w0, memory=3)
    d0 = rig.product(w0)
    moved = 0
    for k in range(12):
        d_in = d0
        out, d0 = step_terms(rig, opt, ref, k, d0, fresh=k == 0)
        check_products(rig, opt, out, d_in)
        moved += out["k"] >= 0
    assert moved >= 8, moved
    plain = rig.lbfgs_ex(start=0.0, memory=3, compact=False)
    plain.run(12)
    assert not np.array_equal(bits(plain.result()[1]), bits(opt.result()[1])), "the compact run has the plain run's history"


def test_compact_lifetimes(engine, synth):
    """Without a compact form: RTD_ERR_NOT_READY. After release_plain: creation and the run work, and equal the run before the release;
    rtd_optimizer_create_lbfgs_ex without the flag and rtd_optimizer_create_lbfgs answer RTD_ERR_NOT_READY. After the matrix has been
    computed again: rtd_optimizer_run answers RTD_ERR_NOT_READY before its first launch."""
    L = engine.lib()
    rig = LbfgsTermsRig(engine, hetero_scene(synth, 64, (0.0,), spots=3, layers=1))
    try:
        rig.set_mixed()
        h = rig.eng._h
        arr = (C.c_void_p * 1)(rig.fields[0]._h)
        out = C.c_void_p()
        ex = L.rtd_optimizer_create_lbfgs_ex
        assert ex(h, arr, 1, rig.obj._h, None, abi.RTD_LBFGS_COMPACT, C.byref(out)) == abi.RTD_ERR_NOT_READY and not out.value
        assert "compact" in L.rtd_last_error(h).decode()
        rig.make_compact()
        before = rig.lbfgs_ex(start=0.0)
        before.run(6)
        h_before = before.result()[1]
        rig.fields[0].dose_influence_compact(release_plain=True)
        after = rig.lbfgs_ex(start=0.0)
        after.run(6)
        assert np.array_equal(bits(after.result()[1]), bits(h_before))
        before.run(1)                                                 # (a compact optimiser made before the release runs on)
        assert before.result()[0]["iterations"] == 7
        assert ex(h, arr, 1, rig.obj._h, None, 0, C.byref(out)) == abi.RTD_ERR_NOT_READY and not out.value
        assert "release_plain" in L.rtd_last_error(h).decode()
        assert L.rtd_optimizer_create_lbfgs(h, arr, 1, rig.obj._h, None, C.byref(out)) in (abi.RTD_ERR_NOT_READY, abi.RTD_ERR_INVALID_ARG) and not out.value
        rig.fields[0].dose_influence()
        launched = after.result()[0]["iterations"]
        assert L.rtd_optimizer_run(h, after._h, 1) == abi.RTD_ERR_NOT_READY
        assert "computed again" in L.rtd_last_error(h).decode()
        assert after.result()[0]["iterations"] == launched
        rig.fields[0].dose_influence_compact()                        # (a new compact form of the new matrix is another matrix)
        assert L.rtd_optimizer_run(h, after._h, 1) == abi.RTD_ERR_NOT_READY
    finally:
        rig.close()


@pytest.mark.parametrize("compact", (False, True))
def test_resident(engine, rig_of, synth, compact):
    """The mixed objective, plain and compact: run(30) is three times run(10), and run(5) captured into a graph on a caller's stream
    and replayed once gives the bits of the direct call."""
    import torch
    rig = rig_of(scene(synth))
    rig.set_mixed()
    if compact:
        rig.make_compact()

    def same(a, b):
        ra, ha = a.result()
        rb, hb = b.result()
        assert ra == rb and np.array_equal(bits(ha), bits(hb)), (ra, rb)
        assert a.lbfgs_report() == b.lbfgs_report()
        for best in (False, True):
            assert np.array_equal(bits(rig.all_weights(a, best)), bits(rig.all_weights(b, best)))
        assert np.array_equal(bits(rig.volume(a.dose())), bits(rig.volume(b.dose())))
        la, lb = rig.line(a), rig.line(b)
        assert np.array_equal(bits(la["thr"]), bits(lb["thr"])) and np.array_equal(bits(la["eud"]), bits(lb["eud"]))
        return ra, ha
    a, b = rig.lbfgs_ex(start=0.0), rig.lbfgs_ex(start=0.0)
    a.run(30)
    for _ in range(3):
        b.run(10)
        b.run(0)
    ra, ha = same(a, b)
    assert ha.size == 30 and ha[-1] < ha[0]
    direct, captured = rig.lbfgs_ex(start=0.0), rig.lbfgs_ex(start=0.0)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    rig.eng.sync()
    rig.eng.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        direct.run(5)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            captured.run(5)
        g.replay()
    torch.cuda.synchronize()
    rd, hd = same(direct, captured)
    rig.eng.set_stream(None)
    assert hd.size == 5 and np.array_equal(bits(hd), bits(ha[:5]))


def test_refusals(engine, synth):
    L = engine.lib()
    rig = LbfgsTermsRig(engine, hetero_scene(synth, 64, (0.0,), spots=3, layers=1))
    try:
        rig.set_mixed()
        eng, h = rig.eng, rig.eng._h
        arr = (C.c_void_p * 1)(rig.fields[0]._h)
        out = C.c_void_p()
        ex = L.rtd_optimizer_create_lbfgs_ex
        for flags in (2, 4, 3, 0x80000000, 0xfffffffe):
            assert ex(h, arr, 1, rig.obj._h, None, flags, C.byref(out)) == abi.RTD_ERR_INVALID_ARG and not out.value, flags
        bad = lbfgs_options()
        bad.reserved[4] = 1
        assert ex(h, arr, 1, rig.obj._h, C.byref(bad), 0, C.byref(out)) == abi.RTD_ERR_INVALID_ARG and not out.value
        bad = lbfgs_options(memory=17)
        assert ex(h, arr, 1, rig.obj._h, C.byref(bad), 0, C.byref(out)) == abi.RTD_ERR_INVALID_ARG
        assert ex(h, None, 1, rig.obj._h, None, 0, C.byref(out)) == abi.RTD_ERR_INVALID_ARG
        assert ex(h, arr, 0, rig.obj._h, None, 0, C.byref(out)) == abi.RTD_ERR_INVALID_ARG
        fresh = eng.create_field(rig.fields[0]._beam, rig.dims)       # no matrix
        assert ex(h, (C.c_void_p * 1)(fresh._h), 1, rig.obj._h, None, 0, C.byref(out)) == abi.RTD_ERR_NOT_READY
        fresh.destroy()
        opt = rig.lbfgs_ex()
        plain_obj = eng.create_objective(rig.dims)
        plain_obj.add_roi(rig.ref.rois[0])
        plain_obj.add_term(R.SQ_DEVIATION, 0, 1.0, rig.level)
        spectral = eng.create_optimizer(rig.fields, plain_obj)
        lbuf = abi.RtdLbfgsLineBuffers()
        assert L.rtd_optimizer_lbfgs_line_buffers(h, spectral._h, C.byref(lbuf)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_lbfgs_line_buffers(h, opt._h, None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_lbfgs_line_buffers(h, None, C.byref(lbuf)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_lbfgs_line_buffers(h, opt._h, C.byref(lbuf)) == abi.RTD_OK
        assert lbuf.d0 == opt.dose() and lbuf.d1 == opt.lbfgs_buffers().trial_dose and lbuf.thresholds and lbuf.eud
        assert (lbuf.n_trials, lbuf.n_terms) == (6, 6) and not any(lbuf.reserved)
        rbe = eng.create_rbe(rig.dims, rbe_models.tissue("constant", 0.1, 0.05))
        assert L.rtd_optimizer_set_let_objective(h, opt._h, plain_obj._h) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_set_rbe(h, opt._h, rbe._h) == abi.RTD_ERR_INVALID_ARG
        v, p = (C.c_double * 1)(), C.c_void_p()
        assert L.rtd_optimizer_scenario_values(h, opt._h, v, None, None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_optimizer_scenario_dose(h, opt._h, 0, C.byref(p)) == abi.RTD_ERR_INVALID_ARG
        rbe.destroy()
        spectral.destroy()
        plain_obj.destroy()
        opt.run(3)
        rep, hist = opt.result()
        assert rep["iterations"] == 3 and np.all(np.diff(hist) <= 0)
        rig.obj.add_term(R.MEAN, 0, 1e-3, 0.0)                        # the objective changes: the optimiser can only be destroyed
        assert L.rtd_optimizer_run(h, opt._h, 1) == abi.RTD_ERR_NOT_READY
    finally:
        rig.close()
