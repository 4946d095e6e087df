"""What every entry point of a field's dose-influence matrix answers at every stage of the matrix's life ("What a
field's matrix is valid for"): no matrix, a matrix, prepared by the first product, LET values, a new table on the handle, LET values
again, the matrix computed again (with a plan set and an optimiser made before), release. At each stage every entry point is called
once and the pair (status, rtd_last_error text) is held against the tables below, whose texts are the engine's, written out here.

One field of the scene of tests/test_gpu_let.py::test_refusals (64^3, three spots, one layer) with a LET table, a second field that
never gets a matrix and a remote field. Nothing here depends on size."""
import ctypes as C

import numpy as np
import pytest

from gpu_support import hetero_scene, options
from raytracedicom_amd import abi, luts

pytestmark = pytest.mark.gpu

F = np.float32
OK, INVALID, NOT_READY = abi.RTD_OK, abi.RTD_ERR_INVALID_ARG, abi.RTD_ERR_NOT_READY

# The entry points in the order a pass calls them: what reads first, what prepares next, rtd_field_let_influence last (so its values
# show in the next pass). `fetch` is rtd_field_fetch "dij_batch".
ENTRIES = ("copy", "device", "fetch", "let_apply", "let_apply_t", "let_device", "apply", "apply_t", "apply_set", "apply_t_set", "prepare", "let_influence")
WHO = {"copy": "rtd_field_dose_influence_copy", "device": "rtd_field_dose_influence_device", "fetch": "rtd_field_fetch",
       "let_apply": "rtd_field_let_influence_apply", "let_apply_t": "rtd_field_let_influence_apply_t", "let_device": "rtd_field_let_influence_device",
       "apply": "rtd_field_dose_influence_apply", "apply_t": "rtd_field_dose_influence_apply_t", "apply_set": "rtd_field_dose_influence_apply_set",
       "apply_t_set": "rtd_field_dose_influence_apply_t_set", "prepare": "rtd_field_dose_influence_prepare", "let_influence": "rtd_field_let_influence"}
DOSE = ("copy", "device", "apply", "apply_t", "apply_set", "apply_t_set", "prepare", "let_influence")
LET = ("let_apply", "let_apply_t", "let_device")

NO_MATRIX = ": no dose-influence matrix (call rtd_field_dose_influence first)"
NO_LET = ": no LET-weighted matrix of the current matrix and table (call rtd_field_let_influence first)"
REMOTE = ": a remote field has no workspace"
NOT_THE_SETS = "rtd_planset_run: a field's matrix is not the one the plan set was created on (create a new set)"
NOT_THE_TABLES = ("rtd_optimizer_run: a field's LET-weighted matrix is not that of its matrix and the handle's table "
                  "(call rtd_field_let_influence again)")


def table(dose, let, fetch):
    """-> {entry: (status, text or None)}: the dose entry points answer `dose`, the LET ones `let` (a suffix behind the entry point's
    name, or None for RTD_OK), the fetch answers `fetch`."""
    t = {}
    for names, (st, suffix) in ((DOSE, dose), (LET, let)):
        for n in names:
            t[n] = (st, None if suffix is None else WHO[n] + suffix)
    t["fetch"] = fetch
    return t


FETCH_NONE = (NOT_READY, "rtd_field_fetch: no dose-influence matrix")
NONE_YET = table((NOT_READY, NO_MATRIX), (NOT_READY, NO_LET), FETCH_NONE)          # no matrix (and after release)
MATRIX = table((OK, None), (NOT_READY, NO_LET), (OK, None))                         # a matrix whose LET values are missing or stale
ALL_OK = table((OK, None), (OK, None), (OK, None))
ON_REMOTE = table((INVALID, REMOTE), (INVALID, REMOTE), FETCH_NONE)
ON_REMOTE["copy"] = (NOT_READY, WHO["copy"] + NO_MATRIX)                            # (tests the matrix first and never asks for remote)


def test_every_entry_point_at_every_stage(engine, synth):
    L = engine.lib()
    scn = hetero_scene(synth, 64, [0.0], spots=3, layers=1)
    b = scn.beams[0]
    let_table = luts.synth_let(synth)
    nvox, nspot, P = 64 ** 3, int(b.spotWeights.size), 2
    eng = engine.Engine(0)
    owned = []                                                        # destroyed in reverse order, in front of the engine
    try:
        eng.set_options(options(0.0))
        eng.set_luts(synth)
        eng.set_ct(scn.ct)
        eng.set_let_table(let_table)
        dVol, dSp = eng.device_alloc(4 * nvox * P), eng.device_alloc(4 * nspot * P)
        eng.device_zero(dVol, 4 * nvox * P)
        eng.to_device(dSp, np.ones(nspot * P, dtype=F))
        vol, sp = C.c_void_p(dVol), C.c_void_p(dSp)
        h = eng._h

        def error():
            return L.rtd_last_error(h).decode()

        def calls(fh):
            cp, ri, va, lv, nnz, need = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_size_t(0)
            colptr, rows, vals = np.empty(nspot + 1, dtype=np.int64), np.empty(nspot * nvox, dtype=np.int32), np.empty(nspot * nvox, dtype=F)
            vp = lambda a: a.ctypes.data_as(C.c_void_p)               # noqa: E731
            return {"copy": lambda: L.rtd_field_dose_influence_copy(h, fh, vp(colptr), vp(rows), vp(vals)),
                    "device": lambda: L.rtd_field_dose_influence_device(h, fh, C.byref(cp), C.byref(ri), C.byref(va), C.byref(nnz)),
                    "fetch": lambda: L.rtd_field_fetch(h, fh, b"dij_batch", None, 0, C.byref(need)),
                    "let_apply": lambda: L.rtd_field_let_influence_apply(h, fh, sp, vol, 1),
                    "let_apply_t": lambda: L.rtd_field_let_influence_apply_t(h, fh, vol, sp),
                    "let_device": lambda: L.rtd_field_let_influence_device(h, fh, C.byref(lv), C.byref(nnz)),
                    "apply": lambda: L.rtd_field_dose_influence_apply(h, fh, sp, vol, 1),
                    "apply_t": lambda: L.rtd_field_dose_influence_apply_t(h, fh, vol, sp),
                    "apply_set": lambda: L.rtd_field_dose_influence_apply_set(h, fh, sp, vol, P, P, 1),
                    "apply_t_set": lambda: L.rtd_field_dose_influence_apply_t_set(h, fh, vol, sp, P, P),
                    "prepare": lambda: L.rtd_field_dose_influence_prepare(h, fh),
                    "let_influence": lambda: L.rtd_field_let_influence(h, fh)}

        def walk(stage, fh, expected):
            """One pass: every entry point once, in ENTRIES' order."""
            c = calls(fh)
            for name in ENTRIES:
                st = c[name]()
                want, text = expected[name]
                assert st == want, (stage, name, st, error())
                if text is not None:
                    assert error() == text, (stage, name)
            eng.sync()
            eng.device_zero(dVol, 4 * nvox * P)                       # (the transposed products read it as g)

        def answer(stage, status, want, text=None):
            assert status == want, (stage, status, error())
            if text is not None:
                assert error() == text, stage

        def status_of(call):
            try:
                call()
            except engine.RtdError as e:
                return e.status
            return OK

        f, g, r = eng.create_field(b, scn.dims), eng.create_field(b, scn.dims), eng.create_field(b, scn.dims, remote=True)
        owned += [f, g, r]
        nnz = C.c_size_t(0)
        # the remote field: refused by name, behind the entry point's own pointer tests
        walk("remote", r._h, ON_REMOTE)
        answer("remote", L.rtd_field_dose_influence(h, r._h, C.c_float(0.0), C.byref(nnz)), INVALID, "rtd_field_dose_influence" + REMOTE)
        answer("remote", L.rtd_field_dose_influence_apply(h, r._h, None, vol, 1), INVALID, "rtd_field_dose_influence_apply: null device pointer")
        answer("remote", L.rtd_field_let_influence_apply_t(h, r._h, vol, None), INVALID, "rtd_field_let_influence_apply_t: null device pointer")
        answer("remote", L.rtd_field_dose_influence_device(h, r._h, None, None, None, None), INVALID, "rtd_field_dose_influence_device: null pointer")
        answer("remote", L.rtd_field_let_influence_device(h, r._h, None, None), INVALID, "rtd_field_let_influence_device: null pointer")
        # 1. no matrix (rtd_field_dose_influence_copy asks for the matrix before it looks at its pointers)
        walk("no matrix", f._h, NONE_YET)
        answer("no matrix", L.rtd_field_dose_influence_copy(h, f._h, None, None, None), NOT_READY, WHO["copy"] + NO_MATRIX)
        # 2., 3. a matrix; the first product prepares
        d = f.dose_influence()
        assert d.nnz > 0
        obj, let_obj = eng.create_objective(scn.dims), eng.create_objective(scn.dims)
        owned += [obj, let_obj]
        for o in (obj, let_obj):
            o.add_roi(np.bincount(d.indices, minlength=nvox) > 0)
            o.add_term(abi.RTD_OBJ_SQ_OVERDOSE, 0, 1.0, 0.0)
        variants = [[(abi.RTD_OBJ_SQ_OVERDOSE, 0, 1.0 + q, 0.0)] for q in range(P)]
        answer("matrix", L.rtd_field_dose_influence_copy(h, f._h, None, None, None), INVALID, "rtd_field_dose_influence_copy: null pointer")
        answer("matrix", status_of(lambda: eng.create_optimizer([f, g], obj)), NOT_READY, "rtd_optimizer_create: a field has no dose-influence matrix (call rtd_field_dose_influence first)")
        answer("matrix", status_of(lambda: eng.create_planset([f, g], obj, variants)), NOT_READY, "rtd_planset_create: a field has no dose-influence matrix (call rtd_field_dose_influence first)")
        answer("matrix", status_of(lambda: eng.create_optimizer([r], obj)), INVALID, "rtd_optimizer_create: a remote field has no matrix")
        opt = eng.create_optimizer([f], obj)
        owned.append(opt)
        answer("matrix", L.rtd_optimizer_set_let_objective(h, opt._h, let_obj._h), NOT_READY,
               "rtd_optimizer_set_let_objective: a field has no LET-weighted matrix (call rtd_field_let_influence first)")
        walk("matrix", f._h, MATRIX)
        # 4. LET values (the pass above ended with rtd_field_let_influence); a plan set and an optimiser with a LET objective
        walk("LET values", f._h, ALL_OK)
        ps = eng.create_planset([f], obj, variants)
        owned.append(ps)
        answer("LET values", L.rtd_optimizer_set_let_objective(h, opt._h, let_obj._h), OK)
        answer("LET values", L.rtd_optimizer_run(h, opt._h, 1), OK)
        answer("LET values", L.rtd_planset_run(h, ps._h, 1), OK)
        # 5., 6. a new table: the LET values are another table's until they are made again; without a table they cannot be made
        eng.set_let_table(let_table.copy())
        answer("new table", L.rtd_optimizer_run(h, opt._h, 1), NOT_READY, NOT_THE_TABLES)
        answer("new table", L.rtd_planset_run(h, ps._h, 1), OK)
        eng.set_let_table(None)
        answer("no table", L.rtd_field_let_influence(h, f._h), NOT_READY, "rtd_field_let_influence: no LET table (call rtd_set_let_table first)")
        eng.set_let_table(let_table)
        walk("new table", f._h, MATRIX)
        walk("LET values again", f._h, ALL_OK)
        answer("LET values again", L.rtd_optimizer_run(h, opt._h, 1), OK)
        # 7., 8. the matrix again: the LET values went with the old one, and the plan set made before is refused
        assert f.dose_influence().nnz == d.nnz
        answer("matrix again", L.rtd_planset_run(h, ps._h, 1), NOT_READY, NOT_THE_SETS)
        answer("matrix again", L.rtd_optimizer_run(h, opt._h, 1), NOT_READY, NOT_THE_TABLES)
        walk("matrix again", f._h, MATRIX)
        walk("matrix again, LET values", f._h, ALL_OK)
        answer("matrix again, LET values", L.rtd_planset_run(h, ps._h, 1), NOT_READY, NOT_THE_SETS)
        answer("matrix again, LET values", L.rtd_optimizer_run(h, opt._h, 1), OK)
        assert opt.result()[0]["iterations"] == 3 and ps.result(0)[0]["iterations"] == 2
        # the field that never got a matrix still has none
        walk("no matrix, second field", g._h, NONE_YET)
        # 9. release: the field object waits in the handle for a field of its shape; a call on the stale handle finds no matrix
        eng.sync()
        stale = C.c_void_p(f._h.value)
        f.release()
        walk("released", stale, NONE_YET)
        answer("released", L.rtd_planset_run(h, ps._h, 1), NOT_READY, NOT_THE_SETS)
        answer("released", L.rtd_optimizer_run(h, opt._h, 1), NOT_READY, NOT_THE_TABLES)
    finally:
        for o in reversed(owned):
            o.destroy()
        eng.close()
