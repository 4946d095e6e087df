#!/usr/bin/env python3
"""Times the resident optimiser with EUD terms on the setting of profiles/optimizer_run.py and profiles/dvh_run.py (C3: 512^3
heterogeneous CT, 10x10 spots x 20 layers, 2 mm dose grid; a spherical target at the centre of the pattern's dose, the rest of the
field's dose box around it). Three numbers from one run, hipEvents on the engine's stream:
  products   apply + apply_t of the field alone (what an iteration cannot be cheaper than);
  plain      run(K) / K with the objective of section 12 (SQ_DEVIATION on the target, SQ_OVERDOSE on the rest): what the parent
             commit runs, and must not move;
  eud        run(K) / K with SQ_DEVIATION + SQ_MIN_EUD (a = -10, at 95 %) on the target and SQ_MAX_EUD (a = 8) on the rest at 0.8 of
             the gEUD the field's own weights give it.
Beside them eval alone with and without EUD terms and one rtd_objective_eud call (the two gEUDs above and the mean of the rest), each
/ K. Every GPU step runs in this one process under the time limit of the command that starts it. Prints one JSON line; with
rocprofv3 --kernel-trace --stats in front (a run of its own), the per-kernel split: k_eud_sum, k_eud_finish and k_obj_eval with and
without EUD terms.
Usage: python profiles/eud_run.py [K]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's HIP runtime initialises first, as in bench.py)

import optimizer_reference as R  # noqa: E402
from raytracedicom_amd import abi, engine, luts, scenarios  # noqa: E402
from profiles.dij_run import _two_mm  # noqa: E402
from profiles.gradient_run import _hip  # noqa: E402
from profiles.optimizer_run import _event_ms  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    K = int(args[0]) if args else 200
    torch.cuda.init()
    hip = _hip()
    es = luts.synth_luts()
    c3 = scenarios.hetero_ct(es, n=512, n_fields=1)
    beam, dims = _two_mm(c3.beams[0], 512)
    nvox, n = int(np.prod(dims)), int(np.prod(beam.spotWeights.shape))
    eng = engine.Engine(0)
    opt = abi.default_options()
    opt.ray_weight_cutoff = 0.0
    eng.set_options(opt)
    eng.set_luts(c3.luts)
    eng.set_ct(c3.ct)
    f = eng.create_field(beam, dims)
    nnz_c = C.c_size_t(0)
    eng._check(engine.lib().rtd_field_dose_influence(eng._h, f._h, C.c_float(0.0), C.byref(nnz_c)))
    f.dose_influence_prepare()
    _, info = f.finish()
    lo, hi = info["dose_box_min"], info["dose_box_max"]
    dD, dG = eng.device_alloc(4 * nvox), eng.device_alloc(4 * nvox)
    dW, dGrad = eng.device_alloc(4 * n), eng.device_alloc(4 * n)
    dV, dOut = eng.device_alloc(8 * 65), eng.device_alloc(8 * 64)
    eng.device_zero(dD, 4 * nvox)
    eng.device_zero(dG, 4 * nvox)
    eng.to_device(dW, np.ascontiguousarray(beam.spotWeights, dtype=np.float32))
    f.dose_influence_apply(dW, dD, init=True)
    dose0 = np.empty((dims[2], dims[1], dims[0]), dtype=np.float32)
    eng.to_host(dose0, dD)
    z, y, x = np.meshgrid(*[np.arange(d) for d in dose0.shape], indexing="ij")
    tot = float(dose0.sum(dtype=np.float64))
    c = [float((dose0 * a).sum(dtype=np.float64)) / tot for a in (z, y, x)]
    sphere = (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= 6.0 ** 2
    box = np.zeros(dose0.shape, dtype=bool)
    box[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    rest = box & ~sphere
    level = float(dose0[sphere].mean())
    plain, eud = eng.create_objective(dims), eng.create_objective(dims)
    for o in (plain, eud):
        o.add_roi(sphere.reshape(-1))
        o.add_roi(rest.reshape(-1))
        o.add_term(R.SQ_DEVIATION, 0, 1.0, level)
    plain.add_term(R.SQ_OVERDOSE, 1, 1.0, 0.3 * level)
    qs = [(0, level, -10.0), (1, level, 8.0), (1, level, 1.0)]
    e_rest = float(eud.eud(dD, qs)[1])
    eud.add_eud_term(abi.RTD_OBJ_SQ_MIN_EUD, 0, 5.0, 0.95 * level, -10.0)
    eud.add_eud_term(abi.RTD_OBJ_SQ_MAX_EUD, 1, 3.0, 0.8 * e_rest, 8.0)
    stream = eng.stream()
    out = {"what": "resident optimiser with EUD terms on C3, 2 mm dose grid; hipEvents around K calls / K", "K": K, "spots": n, "nnz": int(nnz_c.value),
           "dose_dims": list(dims), "target_voxels": int(sphere.sum()), "rest_voxels": int(rest.sum())}

    def pair():
        for _ in range(K):
            f.dose_influence_apply(dW, dD, init=True)
            f.dose_influence_apply_t(dG, dGrad)
    pair()
    eng.sync()
    pair_ms = _event_ms(hip, stream, pair) / K
    out["apply_plus_apply_t_ms"] = round(pair_ms, 4)
    for name, obj in (("plain", plain), ("eud", eud)):
        op = eng.create_optimizer([f], obj)
        op.run(3)                                                     # warm-up: every kernel loaded, the tables built
        eng.sync()
        ms = _event_ms(hip, stream, lambda: op.run(K)) / K
        rep, hist = op.result()
        f.dose_influence_apply(dW, dD, init=True)
        obj.eval(dD, dG, dV)
        eng.sync()
        ev = _event_ms(hip, stream, lambda: [obj.eval(dD, dG, dV) for _ in range(K)]) / K
        out[name] = {"resident_ms_per_iteration": round(ms, 4), "resident_over_products": round(ms / pair_ms, 3), "eval_ms": round(ev, 4),
                     "launches_per_eval": 4 if name == "eud" else 2, "f_first": float(hist[0]), "f_best": rep["f_best"],
                     "best_iteration": rep["best_iteration"], "iterations": rep["iterations"], "guarded": rep["guarded"]}
        if name == "eud":
            dose_best = eng.device_alloc(4 * nvox)
            wb = eng.device_alloc(4 * n)
            op.weights(0, wb, best=True)
            f.dose_influence_apply(wb, dose_best, init=True)
            e_t, e_r, mean_r = (float(v) for v in obj.eud(dose_best, qs))
            out[name].update({"level": level, "rest_gEUD8_of_own_weights_over_level": round(e_rest / level, 4),
                              "target_gEUD_minus10_over_level": round(e_t / level, 4), "rest_gEUD8_over_level": round(e_r / level, 4),
                              "rest_mean_over_level": round(mean_r / level, 4)})
            for p in (dose_best, wb):
                eng.device_free(p)
        op.destroy()
    eud.eud(dD, qs, dev_out=dOut)
    eng.sync()
    out["eud_3_queries_ms"] = round(_event_ms(hip, stream, lambda: [eud.eud(dD, qs, dev_out=dOut) for _ in range(K)]) / K, 4)
    out["eud_over_products"] = out["eud"]["resident_over_products"]
    for o in (plain, eud):
        o.destroy()
    f.destroy()
    for p in (dD, dG, dW, dGrad, dV, dOut):
        eng.device_free(p)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
