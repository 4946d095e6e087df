#!/usr/bin/env python3
"""Measures the constrained optimiser (rtd_optimizer_create_constrained) on C3 (512^3 heterogeneous CT, 10x10
spots x 20 layers) with the 2 mm dose grid and the scene of profiles/optimizer_run.py: a spherical target (SQ_DEVIATION), the rest of
the dose box (SQ_OVERDOSE and a MAX_DVH term), plus two hard constraints that the field's own weights satisfy strictly: MAX_DOSE on a
cord-like half shell beside the target at 1.02 of its largest dose under those weights, and MIN_DOSE on the target at 0.98 of its
smallest. The target's SQ_DEVIATION asks for 1.3 of its level, so the objective pulls against both. hipEvents on the engine's stream.
  iteration     run(K) / K of the plain spectral optimiser (the objective without constraints) and of the constrained one;
  kernels       K calls of rtd_objective_eval, _eval_constrained and _update_multipliers, per call, beside a device copy of the bytes
                k_con_eval moves (27 per union voxel: index, dose, CSR pointer, entry, mask, multiplier, g read and written);
  convergence   the violation of w_best and f_objective every inner block, beside the plain optimiser with a fixed SQ_OVERDOSE on
                the cord at weights 1, 100 and 10 000;
  inner         inner_iterations 10, 20 and 40 at the same K, and 20 with rho0 = f_0 / level^2 instead of the default 1.
Every GPU step runs in this one process under the time limit of the command that starts it. Writes profiles/r37_constrained_run.json
(or the path given with --out) and prints it.
Usage: python profiles/constrained_run.py [K] [--out=PATH]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's HIP runtime initialises first, as in bench.py)

from raytracedicom_amd import abi, engine, luts, scenarios  # noqa: E402
from profiles.dij_run import _two_mm  # noqa: E402
from profiles.gradient_run import _hip  # noqa: E402
from profiles.optimizer_run import _event_ms  # noqa: E402

SQ_DEVIATION, SQ_OVERDOSE = abi.RTD_OBJ_SQ_DEVIATION, abi.RTD_OBJ_SQ_OVERDOSE


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), os.path.join(ROOT, "profiles", "r37_constrained_run.json"))
    K = int(args[0]) if args else 200
    torch.cuda.init()
    hip = _hip()
    es = luts.synth_luts()
    c3 = scenarios.hetero_ct(es, n=512, n_fields=1)
    beam, dims = _two_mm(c3.beams[0], 512)
    nvox, shape = int(np.prod(dims)), beam.spotWeights.shape
    n = int(np.prod(shape))
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
    dD, dG, dW = eng.device_alloc(4 * nvox), eng.device_alloc(4 * nvox), eng.device_alloc(4 * n)
    eng.device_zero(dD, 4 * nvox)
    eng.device_zero(dG, 4 * nvox)
    w0 = np.ascontiguousarray(beam.spotWeights, dtype=np.float32)
    eng.to_device(dW, w0)
    f.dose_influence_apply(dW, dD, init=True)
    dose0 = np.empty((dims[2], dims[1], dims[0]), dtype=np.float32)
    eng.to_host(dose0, dD)
    z, y, x = np.meshgrid(*[np.arange(d) for d in dose0.shape], indexing="ij")
    tot = float(dose0.sum(dtype=np.float64))
    c = [float((dose0 * a).sum(dtype=np.float64)) / tot for a in (z, y, x)]
    r2 = (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2
    sphere = r2 <= 6.0 ** 2
    box = np.zeros(dose0.shape, dtype=bool)
    box[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    rest = box & ~sphere
    cord = rest & (r2 <= 10.0 ** 2) & (x > c[2])
    level = float(dose0[sphere].mean())
    cord_level, target_level = 1.02 * float(dose0[cord].max()), 0.98 * float(dose0[sphere].min())

    def objective(constraints, cord_weight=None):
        o = eng.create_objective(dims)
        o.add_term(SQ_DEVIATION, o.add_roi(sphere.reshape(-1)), 1.0, 1.3 * level)
        rr = o.add_roi(rest.reshape(-1))
        o.add_term(SQ_OVERDOSE, rr, 1.0, 0.3 * level)
        o.add_dvh_term(abi.RTD_OBJ_MAX_DVH, rr, 1.0, 0.5 * level, 0.05)
        rc = o.add_roi(cord.reshape(-1))
        if cord_weight is not None:
            o.add_term(SQ_OVERDOSE, rc, float(cord_weight), cord_level)
        if constraints:
            o.add_constraint(abi.RTD_CON_MAX_DOSE, rc, cord_level)
            o.add_constraint(abi.RTD_CON_MIN_DOSE, 0, target_level)
        return o

    con_obj, plain_obj = objective(True), objective(False)
    stream = eng.stream()
    dBest = eng.device_alloc(4 * n)

    def violation(op):
        """The largest violation of w_best's dose, in units of the level, and the terms' value there."""
        op.weights(0, dev_w_out=dBest, best=True)
        f.dose_influence_apply(dBest, dD, init=True)
        mx, _ = con_obj.constraint_violations(dD)
        vals = plain_obj.eval(dD, dG)
        return float(mx.max()) / level, float(vals[0])

    plain = eng.create_optimizer([f], plain_obj)
    plain.run(3)
    eng.sync()
    plain_ms = _event_ms(hip, stream, lambda: plain.run(K)) / K
    v_plain, f_plain = violation(plain)
    plain.destroy()

    def constrained(inner, k, trace=False, rho0=None):
        co = abi.default_constrained_options()
        co.inner_iterations = inner
        if rho0 is not None:
            co.rho0 = rho0
        op = eng.create_constrained_optimizer([f], con_obj, None, co)
        rows, ms = [], 0.0
        if trace:
            for _ in range(k // inner):
                op.run(inner)
                rows.append((op.result()[0]["iterations"],) + violation(op))
        else:
            op.run(inner + 3)                                         # warm-up across an outer update: every kernel loaded
            eng.sync()
            ms = _event_ms(hip, stream, lambda: op.run(k)) / k
        rep, outer = op.constraint_report()
        v, fo = violation(op)
        op.destroy()
        return {"inner_iterations": inner, "rho0": co.rho0, "ms_per_iteration": round(ms, 4), "violation_over_level": v, "f_objective_of_w_best": fo, "rho": rep["rho"],
                "outer_updates": rep["outer_updates"], "rho_increases": rep["rho_increases"],
                "trace": [{"iterations": int(i), "violation_over_level": a, "f_objective": b} for i, a, b in rows]}

    timed = constrained(20, K)
    traced = {str(i): constrained(i, K, trace=True) for i in (10, 20, 40)}
    f.dose_influence_apply(dW, dD, init=True)
    f0 = float(plain_obj.eval(dD, dG)[0])
    traced["20, rho0 = f_0 / level^2"] = constrained(20, K, trace=True, rho0=f0 / level ** 2)
    fixed = {}
    for wt in (1.0, 100.0, 10000.0):
        po = objective(False, cord_weight=wt)
        op = eng.create_optimizer([f], po)
        op.run(K)
        v, fo = violation(op)
        fixed[str(int(wt))] = {"violation_over_level": v, "f_objective_of_w_best": fo}
        op.destroy()
        po.destroy()
    # the kernels alone
    lay = con_obj.constraint_layout()
    dLam, dMu = eng.device_alloc(4 * max(1, lay.n_entries)), eng.device_alloc(8 * abi.RTD_CON_MAX_CONSTRAINTS)
    dVal, dCon, dViol = eng.device_alloc(8 * 65), eng.device_alloc(8 * 17), eng.device_alloc(16 * 16)
    for p, nb in ((dLam, 4 * max(1, lay.n_entries)), (dMu, 8 * 16)):
        eng.device_zero(p, nb)
    f.dose_influence_apply(dW, dD, init=True)
    con_obj.eval_constrained(dD, dLam, dMu, 1.0, dG, dVal, dCon)
    eng.sync()
    eval_ms = _event_ms(hip, stream, lambda: [plain_obj.eval(dD, dG, dVal) for _ in range(K)]) / K
    evalc_ms = _event_ms(hip, stream, lambda: [con_obj.eval_constrained(dD, dLam, dMu, 1.0, dG, dVal, dCon) for _ in range(K)]) / K
    update_ms = _event_ms(hip, stream, lambda: [con_obj.update_multipliers(dD, 1.0, dLam, dMu, 1e20, 0.0, dViol) for _ in range(K)]) / K
    nbytes = 27 * int(lay.n_union)
    src, dst = eng.device_alloc(nbytes), eng.device_alloc(nbytes)
    eng.device_zero(src, nbytes)

    def copies():
        for _ in range(K):
            hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), C.c_int(3), C.c_void_p(stream))   # 3: device to device
    copies()
    eng.sync()
    copy_ms = _event_ms(hip, stream, copies) / K
    eng.device_free(src)
    eng.device_free(dst)
    out = {"what": "constrained optimiser on C3, 2 mm dose grid; hipEvents around run(K) / K; violations of w_best in units of the target's level",
           "K": K, "spots": n, "nnz": int(nnz_c.value), "dose_dims": list(dims), "target_voxels": int(sphere.sum()), "cord_voxels": int(cord.sum()),
           "union_voxels": int(lay.n_union), "entries": int(lay.n_entries), "level": level,
           "plain_ms_per_iteration": round(plain_ms, 4), "constrained_ms_per_iteration": timed["ms_per_iteration"],
           "constrained_over_plain": round(timed["ms_per_iteration"] / plain_ms, 3),
           "plain_violation_over_level": v_plain, "plain_f_objective_of_w_best": f_plain,
           "eval_ms": round(eval_ms, 4), "eval_constrained_ms": round(evalc_ms, 4), "update_multipliers_ms": round(update_ms, 4),
           "copy_of_27_bytes_per_union_voxel_ms": round(copy_ms, 4), "timed": timed, "inner": traced, "fixed_sq_overdose_weight": fixed}
    for o in (con_obj, plain_obj):
        o.destroy()
    f.destroy()
    for p in (dD, dG, dW, dBest, dLam, dMu, dVal, dCon, dViol):
        eng.device_free(p)
    eng.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
