#!/usr/bin/env python3
"""SHA-256 digests of ten iterations of every resident optimiser, for setting two builds of the engine against each other bit for bit.

On the 96^3 two-field rig of the optimiser tests (tests/gpu_plan_rigs.py, RobustRig: five scenarios) it runs ten iterations of a
plain optimiser, a robust one in both modes, batched and unbatched, a voxel-wise one, a plain one with a LET objective, a plain one
with an RBE model, and a plan set of three plans; each from the start weight 60 on every spot. Per run it hashes the bytes of the
final and the best weights, of the dose volume(s) and of the history (and of what else the run reports), and prints one JSON line.
Two builds agree when their lines are equal: `cmp` them, or diff the JSON. Also in the line: the chunk counts and entry counts
of the scenarios' matrices (the shapes the batched kernels meet).
Every GPU step runs in this one process under the time limit of the command that starts it.
Usage: python profiles/optimizer_digests.py [--lib=PATH_OF_ANOTHER_librtd_hip.so]"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's HIP runtime initialises first, as in bench.py)

from gpu_plan_rigs import MODES, RobustRig  # noqa: E402
from gpu_support import hetero_scene  # noqa: E402
from raytracedicom_amd import abi, engine, luts, rbe  # noqa: E402

K, START, PLANS = 10, 60.0, 3


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    for a in sys.argv[1:]:
        if a.startswith("--lib="):
            engine.LIB_PATH = os.path.abspath(a[len("--lib="):])
    torch.cuda.init()
    synth = luts.synth_luts()
    rig = RobustRig(engine, hetero_scene(synth, 96, (0.0, 90.0)))
    eng, out = rig.eng, {}
    extra = []
    try:
        def record(name, o, doses, **more):
            rep, hist = o.result()
            out[name] = dict(weights=sha(*rig.weights(o)), best_weights=sha(*rig.weights(o, best=True)), dose=sha(*[rig.volume(p) for p in doses]),
                             history=sha(hist), f_best=rep["f_best"], iterations=rep["iterations"], **more)

        o = rig.optimizer(start=START)
        o.run(K)
        record("plain", o, [o.dose()])
        for mode in MODES:
            for no_batch in (False, True):
                o = rig.robust(mode, start=START, no_batch=no_batch)
                o.run(K)
                vals, lams, worst = o.scenario_values()
                record("robust_mode%d%s" % (mode, "_nobatch" if no_batch else ""), o, [o.scenario_dose(s) for s in range(rig.S)],
                       scenario_values=sha(vals, lams), worst=int(worst))
        o = eng.create_voxelwise_optimizer(rig.sfields, rig.obj)
        rig.opts.append(o)
        rig.set_weights(o, START)
        o.run(K)
        record("voxelwise", o, [o.scenario_dose(s) for s in range(rig.S)])
        # LET values of the nominal fields; a LET objective (overdose of the LET-weighted dose wherever a field has a row), an RBE model
        eng.set_let_table(luts.synth_let(synth))
        for f in rig.fields:
            f.let_influence()
        has = sum(np.bincount(d.indices, minlength=rig.nvox) for d in rig.mats) > 0
        let_obj = eng.create_objective(rig.dims)
        extra.append(let_obj)
        let_obj.add_roi(has)
        let_obj.add_term(abi.RTD_OBJ_SQ_OVERDOSE, 0, 1e-3, 2.0 * rig.level)
        o = rig.optimizer(start=START)
        o.set_let_objective(let_obj)
        o.run(K)
        record("let", o, [o.dose(), o.let_dose()], values=sha(o.let_values()))
        model = eng.create_rbe(rig.dims, rbe.tissue("mcnamara", 10.0 * 0.05, 0.05))
        extra.append(model)
        o = rig.optimizer(start=START)
        o.set_rbe(model)
        o.run(K)
        record("rbe", o, [o.dose(), o.rbe_dose()])
        o.set_rbe(None)
        # a plan set: plan p weighs the overdose term 2^p times
        terms = [(abi.RTD_OBJ_SQ_DEVIATION, 0, 1.0, rig.level), (abi.RTD_OBJ_SQ_UNDERDOSE, 0, 5.0, 0.95 * rig.level),
                 (abi.RTD_OBJ_SQ_OVERDOSE, 1, 1.0, 0.3 * rig.level), (abi.RTD_OBJ_MEAN, 1, 1e-3 * rig.level, 0.0)]
        variants = [[(k, r, w * (2.0 ** p if k == abi.RTD_OBJ_SQ_OVERDOSE else 1.0), lv) for k, r, w, lv in terms] for p in range(PLANS)]
        ps = eng.create_planset(rig.fields, rig.obj, variants)
        rig.opts.append(ps)
        for p in range(PLANS):
            for i, s in enumerate(rig.shapes):
                d = rig.alloc(4 * int(np.prod(s)), zero=False)
                eng.to_device(d, np.full(s, START, dtype=np.float32))
                ps.set_weights(p, i, d)
        ps.run(K)
        res = [ps.result(p) for p in range(PLANS)]
        nf = len(rig.fields)
        out["planset_P%d" % PLANS] = dict(weights=sha(*[ps.weights(p, i) for p in range(PLANS) for i in range(nf)]),
                                          best_weights=sha(*[ps.weights(p, i, best=True) for p in range(PLANS) for i in range(nf)]),
                                          dose=sha(*[ps.dose(p) for p in range(PLANS)]), history=sha(*[h for _, h in res]), values=sha(ps.values()),
                                          f_best=[r["f_best"] for r, _ in res], iterations=[r["iterations"] for r, _ in res])
        shapes = dict(nnz=[[int(d.nnz) for d in ms] for ms in rig.smats],
                      chunks=[[int(sum(-(-int(n) // 2048) for n in np.diff(d.indptr))) for d in ms] for ms in rig.smats])
        print(json.dumps(dict(what="ten iterations of every resident optimiser on the 96^3 two-field rig: SHA-256 of weights, doses, histories",
                              K=K, start=START, scenario_shapes=shapes, digests=out)))
    finally:
        for o in rig.opts:                                                # (an optimiser goes before its objectives and its model)
            o.destroy()
        rig.opts = []
        for x in extra:
            x.destroy()
        rig.close()


if __name__ == "__main__":
    main()
