#!/usr/bin/env python3
"""Times the resident spot-weight optimiser (rtd_optimizer_run) on C3 (512^3 heterogeneous CT, 10x10 spots x 20 layers) with the
2 mm dose grid: a spherical target at the centre of the spot pattern's dose (SQ_DEVIATION) and the rest of the field's dose box as
SQ_OVERDOSE. Three numbers from one run, hipEvents on the engine's stream:
  resident   run(K) / K;
  products   apply + apply_t of the same field (what an iteration cannot be cheaper than);
  host loop  the same K iterations driven from the host the way the dose-influence tests drive a descent: dose volume down, objective
             and voxel gradient in numpy, gradient volume up, apply_t, spot gradient down, step in numpy, weights up (wall clock / K).
Every GPU step runs in this one process under the time limit of the command that starts it. Prints one JSON line; with
rocprofv3 --kernel-trace --stats in front, the per-kernel split of the iteration.
Usage: python profiles/optimizer_run.py [K]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's HIP runtime initialises first, as in bench.py)

import optimizer_reference as R  # noqa: E402
from raytracedicom_amd import abi, engine, luts, scenarios  # noqa: E402
from profiles.dij_run import _two_mm  # noqa: E402
from profiles.gradient_run import _hip  # noqa: E402


def _event_ms(hip, stream, call):
    e0, e1, v = C.c_void_p(), C.c_void_p(), C.c_float()
    hip.hipEventCreate(C.byref(e0)); hip.hipEventCreate(C.byref(e1))
    hip.hipEventRecord(e0, C.c_void_p(stream))
    call()
    hip.hipEventRecord(e1, C.c_void_p(stream))
    hip.hipEventSynchronize(e1)
    hip.hipEventElapsedTime(C.byref(v), e0, e1)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    return float(v.value)


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
    dD, dG = eng.device_alloc(4 * nvox), eng.device_alloc(4 * nvox)
    dW, dGrad = eng.device_alloc(4 * n), eng.device_alloc(4 * n)
    eng.device_zero(dD, 4 * nvox)
    eng.device_zero(dG, 4 * nvox)
    w0 = np.ascontiguousarray(beam.spotWeights, dtype=np.float32)
    eng.to_device(dW, w0)
    f.dose_influence_apply(dW, dD, init=True)
    dose0 = np.empty((dims[2], dims[1], dims[0]), dtype=np.float32)
    eng.to_host(dose0, dD)
    # the target: a sphere of 12 mm radius (6 voxels) at the dose-weighted centre of the pattern's own dose; the rest of the dose box
    z, y, x = np.meshgrid(*[np.arange(d) for d in dose0.shape], indexing="ij")
    tot = float(dose0.sum(dtype=np.float64))
    c = [float((dose0 * a).sum(dtype=np.float64)) / tot for a in (z, y, x)]
    sphere = (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= 6.0 ** 2
    box = np.zeros(dose0.shape, dtype=bool)
    box[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    rest = box & ~sphere
    level = float(dose0[sphere].mean())
    obj, ref = eng.create_objective(dims), R.ReferenceObjective(nvox)
    for o in (obj, ref):
        o.add_term(R.SQ_DEVIATION, o.add_roi(sphere.reshape(-1)), 1.0, level)
        o.add_term(R.SQ_OVERDOSE, o.add_roi(rest.reshape(-1)), 1.0, 0.3 * level)
    op = eng.create_optimizer([f], obj)
    stream = eng.stream()
    op.run(3)                                                         # warm-up: every kernel loaded
    eng.sync()
    resident_ms = _event_ms(hip, stream, lambda: op.run(K)) / K
    rep, hist = op.result()

    def pair():
        for _ in range(K):
            f.dose_influence_apply(dW, dD, init=True)
            f.dose_influence_apply_t(dG, dGrad)
    pair_ms = _event_ms(hip, stream, pair) / K
    # the host-driven loop: the same iteration, the vectors and the objective on the host
    host = R.ReferenceOptimizer(ref, None, None, w0)
    vol, grad = np.empty(nvox, dtype=np.float32), np.empty(n, dtype=np.float32)

    def host_iteration():
        eng.to_device(dW, host.w)
        f.dose_influence_apply(dW, dD, init=True)
        eng.to_host(vol, dD)                                          # volume down
        values, g, _ = ref.eval(vol)
        eng.to_device(dG, g.astype(np.float32))                       # voxel gradient up
        f.dose_influence_apply_t(dG, dGrad)
        eng.to_host(grad, dGrad)
        host.advance(float(values[0]), grad)
    for _ in range(2):
        host_iteration()
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(K):
        host_iteration()
    eng.sync()
    host_ms = 1e3 * (time.perf_counter() - t0) / K
    out = {"what": "resident optimiser on C3, 2 mm dose grid; hipEvents around run(K) / K, around K x (apply + apply_t) / K, and the wall "
                   "clock of the same iteration driven from the host / K",
           "K": K, "spots": n, "nnz": int(nnz_c.value), "dose_dims": list(dims), "target_voxels": int(sphere.sum()), "overdose_voxels": int(rest.sum()),
           "resident_ms_per_iteration": round(resident_ms, 4), "apply_plus_apply_t_ms": round(pair_ms, 4),
           "resident_over_products": round(resident_ms / pair_ms, 3), "host_driven_ms_per_iteration": round(host_ms, 3),
           "host_over_resident": round(host_ms / resident_ms, 1),
           "f_first": float(hist[0]), "f_best": rep["f_best"], "best_iteration": rep["best_iteration"], "iterations": rep["iterations"],
           "guarded": rep["guarded"], "host_loop_f_best": host.f_best}
    op.destroy()
    obj.destroy()
    f.destroy()
    for p in (dD, dG, dW, dGrad):
        eng.device_free(p)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
