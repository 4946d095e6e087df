#!/usr/bin/env python3
"""Measures the constrained L-BFGS optimiser (rtd_optimizer_create_constrained_lbfgs) on the scene, plan and
constraints of profiles/constrained_run.py (C3, 2 mm dose grid; profiles/r37_constrained_run.json), with feasibility_tol = 1e-3 x level.
hipEvents on the engine's stream. The same file runs on a build without the new entry points (the parent commit) and then measures
only what that build has, so that the two references come from the parent's own code in the same session:
  iteration     run(K) / K of the constrained spectral optimiser, of rtd_optimizer_create_lbfgs_ex on the objective without the
                constraints, and (new build) of the constrained L-BFGS optimiser;
  line          K calls of rtd_objective_eval_constrained, per call, and (new build) of rtd_objective_constraint_trials with six trials;
  convergence   inner_iterations 5, 10 and 20, 200 iterations in runs of one inner block: after each block the largest violation in
                units of the level and the terms' value, of w_best for the spectral optimiser and of the current w for L-BFGS; the first
                block end from which the violation stays at or below feasibility_tol, and the milliseconds to there at the measured
                time per iteration.
Every GPU step runs in this one process under the time limit of the command that starts it. Writes the JSON to --out (default
profiles/r38_constrained_lbfgs_run.json) and prints it.
Usage: python profiles/constrained_lbfgs_run.py [K] [--out=PATH]"""
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
TOL_OVER_LEVEL = 1e-3


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), os.path.join(ROOT, "profiles", "r38_constrained_lbfgs_run.json"))
    K = int(args[0]) if args else 200
    has_new = hasattr(engine.Engine, "create_constrained_lbfgs_optimizer")
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
    dD, dD1, dG, dW, dCur = eng.device_alloc(4 * nvox), eng.device_alloc(4 * nvox), eng.device_alloc(4 * nvox), eng.device_alloc(4 * n), eng.device_alloc(4 * n)
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
    tol = TOL_OVER_LEVEL * level

    def objective(constraints):
        o = eng.create_objective(dims)
        o.add_term(SQ_DEVIATION, o.add_roi(sphere.reshape(-1)), 1.0, 1.3 * level)
        rr = o.add_roi(rest.reshape(-1))
        o.add_term(SQ_OVERDOSE, rr, 1.0, 0.3 * level)
        o.add_dvh_term(abi.RTD_OBJ_MAX_DVH, rr, 1.0, 0.5 * level, 0.05)
        rc = o.add_roi(cord.reshape(-1))
        if constraints:
            o.add_constraint(abi.RTD_CON_MAX_DOSE, rc, cord_level)
            o.add_constraint(abi.RTD_CON_MIN_DOSE, 0, target_level)
        return o

    con_obj, plain_obj = objective(True), objective(False)
    stream = eng.stream()

    def violation(op, best):
        """The largest violation of the dose of w_best or of the current w, in units of the level, and the terms' value there."""
        op.weights(0, dev_w_out=dCur, best=best)
        f.dose_influence_apply(dCur, dD, init=True)
        mx, _ = con_obj.constraint_violations(dD)
        vals = plain_obj.eval(dD, dG)
        return float(mx.max()) / level, float(vals[0])

    def options(inner):
        co = abi.default_constrained_options()
        co.inner_iterations = inner
        co.feasibility_tol = tol
        return co

    def timed(make, warm):
        op = make()
        op.run(warm)                                                  # warm-up across an outer update: every kernel loaded
        eng.sync()
        ms = _event_ms(hip, stream, lambda: op.run(K)) / K
        op.destroy()
        return ms

    def traced(make, inner, best, ms_per_iteration):
        op = make(inner)
        rows = []
        for _ in range(K // inner):
            op.run(inner)
            rows.append((op.result()[0]["iterations"],) + violation(op, best))
        rep, _ = op.constraint_report()
        extra = op.lbfgs_report() if not best else {}
        op.destroy()
        first = None
        for i in range(len(rows) - 1, -1, -1):                        # the first block end from which the violation stays within tol
            if rows[i][1] > TOL_OVER_LEVEL:
                break
            first = i
        return {"inner_iterations": inner, "rho": rep["rho"], "outer_updates": rep["outer_updates"], "rho_increases": rep["rho_increases"],
                "feasible_from_iteration": None if first is None else int(rows[first][0]),
                "feasible_from_ms": None if first is None else round(rows[first][0] * ms_per_iteration, 3),
                "f_objective_there": None if first is None else rows[first][2], "f_objective_after_%d" % K: rows[-1][2],
                "violation_over_level_after_%d" % K: rows[-1][1],
                "steps": {k: extra[k] for k in ("unit_steps", "backtracked_steps", "halvings", "stalls", "resets")} if extra else None,
                "trace": [{"iterations": int(i), "violation_over_level": a, "f_objective": b} for i, a, b in rows]}

    spectral_ms = timed(lambda: eng.create_constrained_optimizer([f], con_obj, None, options(20)), 23)
    lbfgs_ms = timed(lambda: eng.create_lbfgs_optimizer_ex([f], plain_obj), 3)
    out = {"what": "constrained L-BFGS on C3, 2 mm dose grid, the plan and constraints of r37; hipEvents around run(K) / K; violations in units of the target's level; "
                   "feasibility_tol = 1e-3 x level; convergence sampled at the end of every inner block",
           "build_has_constrained_lbfgs": has_new, "K": K, "spots": n, "nnz": int(nnz_c.value), "dose_dims": list(dims), "level": level,
           "spectral_constrained_ms_per_iteration": round(spectral_ms, 4), "lbfgs_ex_unconstrained_ms_per_iteration": round(lbfgs_ms, 4)}
    out["spectral"] = {str(i): traced(lambda inner: eng.create_constrained_optimizer([f], con_obj, None, options(inner)), i, True, spectral_ms) for i in (5, 10, 20)}
    # the line search's constraint half
    lay = con_obj.constraint_layout()
    dLam, dMu = eng.device_alloc(4 * max(1, lay.n_entries)), eng.device_alloc(8 * abi.RTD_CON_MAX_CONSTRAINTS)
    dVal, dCon, dPsi = eng.device_alloc(8 * 65), eng.device_alloc(8 * 17), eng.device_alloc(2 * 8 * 8 * 16)
    for p, nb in ((dLam, 4 * max(1, lay.n_entries)), (dMu, 8 * 16)):
        eng.device_zero(p, nb)
    f.dose_influence_apply(dW, dD, init=True)
    eng.to_device(dCur, (1.1 * w0).astype(np.float32))
    f.dose_influence_apply(dCur, dD1, init=True)
    con_obj.eval_constrained(dD, dLam, dMu, 1.0, dG, dVal, dCon)
    eng.sync()
    evalc_ms = _event_ms(hip, stream, lambda: [con_obj.eval_constrained(dD, dLam, dMu, 1.0, dG, dVal, dCon) for _ in range(K)]) / K
    eval_ms = _event_ms(hip, stream, lambda: [plain_obj.eval(dD, dG, dVal) for _ in range(K)]) / K
    out.update(union_voxels=int(lay.n_union), entries=int(lay.n_entries), eval_ms=round(eval_ms, 4), eval_constrained_ms=round(evalc_ms, 4),
               six_eval_constrained_ms=round(6 * evalc_ms, 4), six_constraint_shares_ms=round(6 * (evalc_ms - eval_ms), 4))
    if has_new:
        con_obj.constraint_trials(dD, dD1, 6, dLam, dMu, 1.0, dPsi, dPsi + 8 * 8 * 16)
        eng.sync()
        trials_ms = _event_ms(hip, stream, lambda: [con_obj.constraint_trials(dD, dD1, 6, dLam, dMu, 1.0, dPsi, dPsi + 8 * 8 * 16) for _ in range(K)]) / K
        new_ms = timed(lambda: eng.create_constrained_lbfgs_optimizer([f], con_obj, None, options(20)), 23)
        out.update(constraint_trials_6_ms=round(trials_ms, 4), constrained_lbfgs_ms_per_iteration=round(new_ms, 4),
                   constrained_lbfgs_over_spectral=round(new_ms / spectral_ms, 3), constrained_lbfgs_over_lbfgs_ex=round(new_ms / lbfgs_ms, 3))
        out["lbfgs"] = {str(i): traced(lambda inner: eng.create_constrained_lbfgs_optimizer([f], con_obj, None, options(inner)), i, False, new_ms) for i in (5, 10, 20)}
    for o in (con_obj, plain_obj):
        o.destroy()
    f.destroy()
    for p in (dD, dD1, dG, dW, dCur, dLam, dMu, dVal, dCon, dPsi):
        eng.device_free(p)
    eng.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("spectral", "lbfgs")}))
    for kind in ("spectral", "lbfgs"):
        for i, r in out.get(kind, {}).items():
            print(kind, i, json.dumps({k: v for k, v in r.items() if k != "trace"}))


if __name__ == "__main__":
    main()
