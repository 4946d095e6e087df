"""rtd_optimizer_create_4d on the device (include/rtd.h "4D dose: phases warped and summed"): the resident iteration against a loop
driven from Python with the public calls, bit for bit; the batched path against RTD_4D_NO_BATCH; what the getters answer; the
one-phase identity case against the plain optimiser; capture; the stale-matrix refusal; the refusals. The scene is
tests/fourd_scenes.py's: three phases of the 96^3 phantom, a reference grid of its own, smooth random fields."""
import ctypes as C

import numpy as np
import pytest

import fourd_scenes as S
from gpu_plan_rigs import same
from gpu_support import bits, hetero_scene
from raytracedicom_amd import abi, fourd, rbe

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def rig(engine, synth):
    r = S.FourDRig(engine, synth)
    yield r
    r.close()


def test_run_equals_the_loop_driven_from_python(rig):
    """run(10) against apply per field and phase, warp_sum, Objective.eval, warp_dose_t_phases, apply_t, the float64 combine and the step
    rule of tests/optimizer_reference.py: history, weights and best weights bit for bit. The iteration descends; dose() is
    accumulate_phases of the three scenario_dose(p) volumes; scenario_values answers as a composite; the fields act."""
    opt = rig.optimizer()
    opt.run(10)
    ref = rig.python_loop(rig.obj, 10)
    rep, hist = rig.equals_loop(opt, ref)
    print("device history:", " ".join("%.6g" % x for x in hist))
    assert hist.size == 10 and rep["f_best"] <= hist[0] and min(ref.history) < ref.history[0]
    # the volumes
    doses = [rig.volume(opt.scenario_dose(p), rig.nvox).reshape(S.shape_of(rig.dims)) for p in range(3)]
    assert all(np.count_nonzero(d) > 1000 for d in doses) and not np.array_equal(doses[0], doses[2])
    pieces = [((w.dst_idx_to_src_idx, w.dst_idx_to_dvf_idx, np.array(w.disp_to_src_idx)), d) for w, d in zip(rig.warps, rig.dvfs)]
    want = rig.eng.accumulate_phases(doses, pieces, S.PHASE_WEIGHTS, rig.ref_dims)
    got = rig.volume(opt.dose(), rig.nref).reshape(want.shape)
    assert np.array_equal(bits(got), bits(want)) and np.count_nonzero(got) > 1000
    with pytest.raises(rig.engine.RtdError) as ei:
        opt.scenario_dose(3)
    assert ei.value.status == abi.RTD_ERR_INVALID_ARG
    vals, lams, worst = opt.scenario_values()
    assert np.array_equal(bits(vals), bits(np.full(3, rep["f_last"]))) and (lams == 1.0).all() and worst == 0
    # with the fields zeroed the history is another one: the warp did act
    flat = rig.optimizer(warps=rig.still)
    flat.run(10)
    assert not np.array_equal(bits(flat.result()[1]), bits(hist))
    rig.drop(flat)
    rig.drop(opt)


def test_batched_equals_the_per_phase_sequences(rig):
    a, b = rig.optimizer(), rig.optimizer(no_batch=True)
    a.run(10)
    b.run(10)
    rep, hist = same(rig, a, b)
    assert hist.size == 10
    for p in range(3):
        assert np.array_equal(bits(rig.volume(a.scenario_dose(p), rig.nvox)), bits(rig.volume(b.scenario_dose(p), rig.nvox)))
    assert np.array_equal(bits(rig.volume(a.dose(), rig.nref)), bits(rig.volume(b.dose(), rig.nref)))
    rig.drop(a)
    rig.drop(b)


def test_dvh_and_eud_terms(rig):
    obj = rig.dvh_eud_objective()
    for no_batch in (False, True):
        opt = rig.optimizer(obj=obj, no_batch=no_batch)
        opt.run(3)
        rep, hist = rig.equals_loop(opt, rig.python_loop(obj, 3))
        assert hist.size == 3 and np.isfinite(hist).all() and hist[0] > 0
        rig.drop(opt)


def test_thirty_is_three_times_ten_and_capture(rig):
    import torch
    a, b = rig.optimizer(), rig.optimizer()
    a.run(30)
    for _ in range(3):
        b.run(10)
        b.run(0)
    rep, hist = same(rig, a, b)
    assert hist.size == 30
    direct, captured = rig.optimizer(), rig.optimizer()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    rig.eng.sync()
    rig.eng.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        direct.run(3)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            captured.run(3)
        g.replay()
    torch.cuda.synchronize()
    rd, hd = direct.result()
    rg, hg = captured.result()
    rig.eng.set_stream(None)
    assert rd == rg and hd.size == 3 and np.array_equal(bits(hd), bits(hg)) and np.array_equal(bits(hd), bits(hist[:3]))
    for x, y in zip(rig.weights(direct), rig.weights(captured)):
        assert np.array_equal(bits(x), bits(y))
    for o in (a, b, direct, captured):
        rig.drop(o)


def test_one_identity_phase_against_the_plain_optimiser(rig):
    """One phase, the identity map, a zero field, weight 1.0, the objective on the phase grid: the forward warp is a copy (a row sum is
    never -0), so history[0] and dose() are the plain optimiser's bit for bit. Later entries may differ: the transposed rule quantises."""
    eng = rig.eng
    phase_dose = sum(m.matvec(rig.w0[a:b]) for m, a, b in zip(rig.smats[0], rig.offs, rig.offs[1:]))
    target = phase_dose > 0.5 * phase_dose.max()
    obj = eng.create_objective(rig.dims)
    rig.objs.append(obj)
    obj.add_roi(target)
    obj.add_term(abi.RTD_OBJ_SQ_DEVIATION, 0, 1.0, 1.1 * float(phase_dose[target].mean()))
    ident = fourd.phase_warps(eng, rig.phase_to_world, rig.phase_to_world, [np.zeros((3, 2, 2, 2), dtype=F)], (np.diag([95.0] * 3) @ np.diag(rig.scn.spacing), rig.phase_to_world[1]))
    try:
        m = ident[0].dst_idx_to_src_idx
        assert list(m.m) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(m.v) == [0, 0, 0]
        four = eng.create_4d_optimizer([rig.sfields[0]], ident, obj, [1.0])
        plain = eng.create_optimizer(rig.sfields[0], obj)
        rig.opts += [four, plain]
        four.run(3)
        plain.run(3)
        hf, hp = four.result()[1], plain.result()[1]
        print("4D:", hf, "plain:", hp)
        assert hf.size == 3 and np.array_equal(bits(hf[:1]), bits(hp[:1]))
        assert np.array_equal(bits(rig.volume(four.dose(), rig.nvox)), bits(rig.volume(plain.dose(), rig.nvox)))
        rig.drop(four)
        rig.drop(plain)
    finally:
        ident.free()


def test_a_recomputed_matrix_makes_run_refuse(rig):
    opt = rig.optimizer()
    opt.run(2)
    rep, hist = opt.result()
    w = [x.copy() for x in rig.weights(opt)]
    rig.eng.set_ct(np.roll(rig.scn.ct, S.SHIFTS[1], axis=0))          # (phase 1's CT: the matrix comes out as it was)
    rig.sfields[1][0].dose_influence()                                # computed again: the optimiser's note of it is stale
    with pytest.raises(rig.engine.RtdError) as ei:
        opt.run(1)
    assert ei.value.status == abi.RTD_ERR_NOT_READY
    rep2, hist2 = opt.result()
    assert rep2 == rep and np.array_equal(bits(hist2), bits(hist))
    for x, y in zip(rig.weights(opt), w):
        assert np.array_equal(bits(x), bits(y))
    rig.drop(opt)
    again = rig.optimizer()                                           # after destroy and re-create it runs
    again.run(2)
    assert np.array_equal(bits(again.result()[1]), bits(hist))
    rig.drop(again)


def test_refusals(rig, synth):
    eng, engine = rig.eng, rig.engine
    L = engine.lib()
    bare = eng.create_field(rig.scn.beams[0], rig.dims)               # no matrix
    other_grid = eng.create_field(rig.scn.beams[0], (96, 96, 95))
    small = eng.create_field(hetero_scene(synth, 96, (0.0,), spots=3).beams[0], rig.dims)
    recs = list(rig.warps)

    def record(**kw):
        r = abi.RtdWarp.from_buffer_copy(bytes(recs[1]))
        if "k" in kw:
            r.disp_to_src_idx[0] = kw["k"]
        if "dvf" in kw:
            r.dev_dvf = kw["dvf"]
        if "dims" in kw:
            r.dvf_dims[1] = kw["dims"]
        return r

    def raw(rows, warps, weights=None, n_phases=None, reserved0=0, reserved=0, null_warps=False, obj=None, null_out=False):
        fo = abi.Rtd4dOptions()
        fo.n_phases = len(rows) if n_phases is None else n_phases
        fo.reserved0 = reserved0
        fo.reserved[2] = reserved
        wa = (abi.RtdWarp * max(1, len(warps)))(*warps)
        if not null_warps:
            fo.warps = wa
        if weights is not None:
            wt = np.asarray(weights, dtype=F)
            fo.weights = abi.fptr(wt)
        flat = [f._h for fs in rows for f in fs]
        arr = (C.c_void_p * max(1, len(flat)))(*flat)
        out = C.c_void_p()
        st = L.rtd_optimizer_create_4d(eng._h, arr, len(rows[0]) if rows else 0, C.byref(fo), (rig.obj if obj is None else obj)._h, None,
                                       None if null_out else C.byref(out))
        assert not out.value, "a refused call left an optimiser behind"
        return st
    sf = rig.sfields
    empty = eng.create_objective(rig.ref_dims)
    try:
        invalid = {
            "no phases": lambda: raw(sf, recs, n_phases=0),
            "17 phases": lambda: raw(sf, recs, n_phases=17),
            "null warps": lambda: raw(sf, recs, null_warps=True),
            "a NaN in a warp's k": lambda: raw(sf, [recs[0], record(k=float("nan")), recs[2]]),
            "a null dev_dvf": lambda: raw(sf, [recs[0], record(dvf=None), recs[2]]),
            "a zero field dimension": lambda: raw(sf, [recs[0], record(dims=0), recs[2]]),
            "a zero weight": lambda: raw(sf, recs, weights=(0.5, 0.0, 0.5)),
            "a negative weight": lambda: raw(sf, recs, weights=(0.5, -0.25, 0.5)),
            "a NaN weight": lambda: raw(sf, recs, weights=(0.5, np.nan, 0.5)),
            "an infinite weight": lambda: raw(sf, recs, weights=(np.inf, 0.25, 0.5)),
            "reserved0": lambda: raw(sf, recs, reserved0=1),
            "a reserved word": lambda: raw(sf, recs, reserved=1),
            "a null result pointer": lambda: raw(sf, recs, null_out=True),
            "no fields": lambda: raw([[], [], []], recs),
            "17 fields": lambda: raw([(sf[0] * 9)[:17]], recs[:1]),
            "a field listed twice": lambda: raw([sf[0], sf[0], sf[2]], recs),
            "another spot-map shape": lambda: raw([sf[0], [small, sf[1][1]], sf[2]], recs),
            "another dose grid": lambda: raw([sf[0], [other_grid, sf[1][1]], sf[2]], recs),
            "an objective without terms": lambda: raw(sf, recs, obj=empty),
        }
        for what, call in invalid.items():
            assert call() == abi.RTD_ERR_INVALID_ARG, what
        assert raw([sf[0], [bare, sf[1][1]], sf[2]], recs) == abi.RTD_ERR_NOT_READY
        # a 4D optimiser takes neither a LET objective nor an RBE model, as a robust one
        opt = rig.optimizer()
        let_obj = eng.create_objective(rig.ref_dims)
        model = eng.create_rbe(rig.ref_dims, rbe.tissue("mcnamara", 0.5, 0.05))
        try:
            let_obj.add_roi(np.arange(10))
            let_obj.add_term(abi.RTD_OBJ_MEAN, 0, 1.0, 0.0)
            for call in (lambda: opt.set_let_objective(let_obj), lambda: opt.set_rbe(model)):
                with pytest.raises(engine.RtdError) as ei:
                    call()
                assert ei.value.status == abi.RTD_ERR_INVALID_ARG
            # ... and after all of it every object is usable
            opt.run(2)
            assert opt.result()[1].size == 2
        finally:
            rig.drop(opt)
            model.destroy()
            let_obj.destroy()
    finally:
        empty.destroy()
        for f in (bare, other_grid, small):
            f.destroy()
