#!/usr/bin/env python3
"""Times the L-BFGS optimiser of rtd_optimizer_create_lbfgs_ex on an objective with DVH and EUD terms, on the plain and on the compact
matrix, beside the spectral optimiser on the same objective: C3 (512^3 heterogeneous CT, 10x10 spots x 20 layers), 2 mm dose grid,
the DVH objective of profiles/dvh_run.py (SQ_DEVIATION and MIN_DVH 98 % on the sphere, MAX_DVH 25 % on the rest of the dose box) plus
the SQ_MAX_EUD term (a = 8) of profiles/eud_run.py on the rest. One process, hipEvents on the engine's stream:
  (a) ms per iteration of the spectral optimiser, run(K) / K (its code is the parent's), and its f_best after K iterations;
  (b) ms per iteration of L-BFGS (m = 8, 6 trials), plain and compact, the iteration whose objective first reaches (a)'s f_best and
      the time to get there, with the counters of the run;
  (c) the K-wide line search at 6 trials: 6 separate rtd_objective_eval calls on 6 trial volumes (the design it replaces), beside
      (b) - (a) on the plain matrix, which holds the whole line search AND the L-BFGS vector kernels (an upper bound of its cost);
  (d) ms per iteration of rtd_optimizer_create_lbfgs and of _create_lbfgs_ex (flags 0) on the plain objective of profiles/lbfgs_run.py.
Prints one JSON line. Usage: python profiles/lbfgs_terms_run.py [K]"""
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
    dD, dW, dG = eng.device_alloc(4 * nvox), eng.device_alloc(4 * n), eng.device_alloc(4 * nvox)
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
    sphere = (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= 6.0 ** 2
    box = np.zeros(dose0.shape, dtype=bool)
    box[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    rest = box & ~sphere
    level = float(dose0[sphere].mean())
    plain, terms = eng.create_objective(dims), eng.create_objective(dims)
    for o in (plain, terms):
        o.add_roi(sphere.reshape(-1))
        o.add_roi(rest.reshape(-1))
        o.add_term(R.SQ_DEVIATION, 0, 1.0, level)
    plain.add_term(R.SQ_OVERDOSE, 1, 1.0, 0.3 * level)
    e_rest = float(terms.eud(dD, [(1, level, 8.0)])[0])
    terms.add_dvh_term(abi.RTD_OBJ_MIN_DVH, 0, 5.0, 0.95 * level, 0.98)
    terms.add_dvh_term(abi.RTD_OBJ_MAX_DVH, 1, 3.0, 0.3 * level, 0.25)
    terms.add_eud_term(abi.RTD_OBJ_SQ_MAX_EUD, 1, 3.0, 0.8 * e_rest, 8.0)
    stream = eng.stream()

    def timed(make):
        """Two optimisers of one kind: one warms every kernel up and is thrown away, the other runs K iterations from the start
        weights under the events, so that its history is the history of K iterations from w0."""
        warm = make()
        warm.run(3)
        eng.sync()
        warm.destroy()
        op = make()
        op.run(0)
        eng.sync()
        ms = _event_ms(hip, stream, lambda: op.run(K)) / K
        return op, ms
    lo_opt = abi.default_lbfgs_options()
    lo_opt.memory, lo_opt.max_halvings = 8, 5
    n_trials = 1 + lo_opt.max_halvings
    out = {"what": "L-BFGS with DVH and EUD terms (m = 8, 6 trials), plain and compact, beside the spectral optimiser on the same objective; C3, 2 mm "
                   "dose grid; hipEvents around run(K) / K of each, all from the field's own weights",
           "K": K, "spots": n, "nnz": int(nnz_c.value), "dose_dims": list(dims), "target_voxels": int(sphere.sum()), "rest_voxels": int(rest.sum())}
    # (d) the plain objective: create_lbfgs beside create_lbfgs_ex with flags 0
    old, old_ms = timed(lambda: eng.create_lbfgs_optimizer([f], plain, lo_opt))
    new, new_ms = timed(lambda: eng.create_lbfgs_optimizer_ex([f], plain, lo_opt))
    out["plain_objective_create_lbfgs_ms_per_iteration"] = round(old_ms, 4)
    out["plain_objective_create_lbfgs_ex_ms_per_iteration"] = round(new_ms, 4)
    out["plain_objective_same_history"] = bool(np.array_equal(old.result()[1].view(np.uint64), new.result()[1].view(np.uint64)))
    old.destroy()
    new.destroy()
    # (a) the spectral optimiser on the objective with DVH and EUD terms
    spectral, spectral_ms = timed(lambda: eng.create_optimizer([f], terms))
    srep, shist = spectral.result()
    out.update(spectral_ms_per_iteration=round(spectral_ms, 4), f_first=float(shist[0]), spectral_f_best=srep["f_best"],
               spectral_best_iteration=srep["best_iteration"], spectral_rises=int((np.diff(shist) > 0).sum()), spectral_ms_for_K=round(K * spectral_ms, 4))
    spectral.destroy()
    # (c) 6 separate evaluations on 6 trial volumes d0 + 2^-k (d1 - d0), d1 the dose of half the weights
    d1 = (0.5 * dose0.astype(np.float64)).astype(np.float32)
    vols = []
    for k in range(n_trials):
        r = d1 if k == 0 else (dose0.astype(np.float64) + 0.5 ** k * (d1.astype(np.float64) - dose0.astype(np.float64))).astype(np.float32)
        p = eng.device_alloc(4 * nvox)
        eng.to_device(p, np.ascontiguousarray(r))
        vols.append(p)
    dV = eng.device_alloc(8 * (1 + abi.RTD_OBJ_MAX_TERMS))

    def evals():
        for _ in range(K):
            for p in vols:
                terms.eval(p, dG, dV)
    evals()
    eng.sync()
    out["separate_evals_ms_per_line_search"] = round(_event_ms(hip, stream, evals) / K, 4)
    # (b) L-BFGS on that objective, plain and compact
    for name, compact in (("plain", False), ("compact", True)):
        if compact:
            f.dose_influence_compact()
        op, ms = timed(lambda: eng.create_lbfgs_optimizer_ex([f], terms, lo_opt, compact=compact))
        rep, hist = op.result()
        lb = op.lbfgs_report()
        reached = np.flatnonzero(hist <= srep["f_best"])
        first = int(reached[0]) if reached.size else None
        out["lbfgs_" + name] = {"ms_per_iteration": round(ms, 4), "over_spectral": round(ms / spectral_ms, 3), "f_best": rep["f_best"],
                                "best_iteration": rep["best_iteration"], "rises": int((np.diff(hist) > 0).sum()),
                                "first_iteration_at_spectral_f_best": first, "ms_to_spectral_f_best": None if first is None else round(first * ms, 4),
                                "unit_steps": lb["unit_steps"], "backtracked_steps": lb["backtracked_steps"], "halvings": lb["halvings"],
                                "resets": lb["resets"], "stalls": lb["stalls"], "pairs": lb["pairs"], "guarded": rep["guarded"],
                                "history_every_20": [float(v) for v in hist[::20]]}
        op.destroy()
    out["line_search_and_vector_kernels_ms_upper_bound"] = round(out["lbfgs_plain"]["ms_per_iteration"] - spectral_ms, 4)
    out["spectral_history_every_20"] = [float(v) for v in shist[::20]]
    for o in (plain, terms):
        o.destroy()
    f.destroy()
    for p in [dD, dW, dG, dV] + vols:
        eng.device_free(p)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
