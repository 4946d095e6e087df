#!/usr/bin/env python3
"""Times the resident L-BFGS optimiser (rtd_optimizer_create_lbfgs) beside the spectral one (rtd_optimizer_create) on C3 (512^3
heterogeneous CT, 10x10 spots x 20 layers) with the 2 mm dose grid and the objective of profiles/optimizer_run.py: a spherical target
at the centre of the spot pattern's dose (SQ_DEVIATION) and the rest of the field's dose box as SQ_OVERDOSE. One process, hipEvents
on the engine's stream:
  (a) ms per iteration of the spectral optimiser, run(K) / K (the reference);
  (b) ms per iteration of L-BFGS at m = 8, K_trials = 6, run(K) / K;
  (c) the spectral f_best after K iterations, and the L-BFGS iteration (and time at (b)) whose objective first reaches it;
  (d) unit steps, backtracked steps, resets and stalls of the L-BFGS run.
Every GPU step runs in this one process under the time limit of the command that starts it. Prints one JSON line; with
rocprofv3 --kernel-trace --stats in front, the per-kernel split of both iterations.
Usage: python profiles/lbfgs_run.py [K]"""
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
    dD, dW = eng.device_alloc(4 * nvox), eng.device_alloc(4 * n)
    eng.device_zero(dD, 4 * nvox)
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
    obj = eng.create_objective(dims)
    obj.add_term(R.SQ_DEVIATION, obj.add_roi(sphere.reshape(-1)), 1.0, level)
    obj.add_term(R.SQ_OVERDOSE, obj.add_roi(rest.reshape(-1)), 1.0, 0.3 * level)
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
    spectral, spectral_ms = timed(lambda: eng.create_optimizer([f], obj))
    lbfgs, lbfgs_ms = timed(lambda: eng.create_lbfgs_optimizer([f], obj, lo_opt))
    srep, shist = spectral.result()
    lrep, lhist = lbfgs.result()
    lb = lbfgs.lbfgs_report()
    reached = np.flatnonzero(lhist <= srep["f_best"])
    first = int(reached[0]) if reached.size else None
    out = {"what": "L-BFGS (m = 8, 6 trial steps) beside the spectral optimiser on C3, 2 mm dose grid; hipEvents around run(K) / K of each, "
                   "both from the field's own weights",
           "K": K, "spots": n, "nnz": int(nnz_c.value), "dose_dims": list(dims), "target_voxels": int(sphere.sum()), "overdose_voxels": int(rest.sum()),
           "spectral_ms_per_iteration": round(spectral_ms, 4), "lbfgs_ms_per_iteration": round(lbfgs_ms, 4),
           "lbfgs_over_spectral": round(lbfgs_ms / spectral_ms, 3),
           "f_first": float(shist[0]), "spectral_f_best": srep["f_best"], "spectral_best_iteration": srep["best_iteration"],
           "spectral_rises": int((np.diff(shist) > 0).sum()),
           "lbfgs_f_best": lrep["f_best"], "lbfgs_best_iteration": lrep["best_iteration"], "lbfgs_rises": int((np.diff(lhist) > 0).sum()),
           "lbfgs_first_iteration_at_spectral_f_best": first,
           "lbfgs_ms_to_spectral_f_best": None if first is None else round(first * lbfgs_ms, 4),
           "spectral_ms_for_K": round(K * spectral_ms, 4),
           "unit_steps": lb["unit_steps"], "backtracked_steps": lb["backtracked_steps"], "halvings": lb["halvings"], "resets": lb["resets"],
           "stalls": lb["stalls"], "pairs": lb["pairs"], "guarded": lrep["guarded"],
           "lbfgs_history_every_20": [float(v) for v in lhist[::20]], "spectral_history_every_20": [float(v) for v in shist[::20]]}
    for o in (spectral, lbfgs):
        o.destroy()
    obj.destroy()
    f.destroy()
    for p in (dD, dW):
        eng.device_free(p)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
