#!/usr/bin/env python3
"""Times the voxel-wise worst-case optimiser (rtd_optimizer_create_voxelwise) in the setting of profiles/robust_run.py: C3 (512^3
heterogeneous CT, one field of 10x10 spots x 20 layers), 2 mm dose grid, a spherical target (SQ_DEVIATION) and the rest of the dose
box (SQ_OVERDOSE), with S = 9 scenarios: nominal, the patient displaced by +-3 mm along each gantry axis, and the stopping-power table
scaled by 0.965 and 1.035. hipEvents on the engine's stream around run(K), per configuration and repetition:
  expected            rtd_optimizer_create_robust, EXPECTED, batched over the scenario axis: all S forward and transposed products,
                      2 S evaluation launches and the decision (the iteration this one is held against);
  voxelwise           rtd_optimizer_create_voxelwise, batched: the same products for the active scenarios, one composite evaluation
                      (a clear and two launches) and the decision;
  voxelwise_no_batch  the same with RTD_ROBUST_NO_BATCH.
The configurations are interleaved within a repetition. `--expected` stops after the EXPECTED optimiser and needs nothing of the
voxel-wise interface, so that the same file times the parent build of the library. Prints one JSON line; with rocprofv3 --kernel-trace
--stats in front, the per-kernel split (k_obj_eval_voxelwise among them).
Usage: python profiles/voxelwise_run.py [K] [--expected] [--reps=N]"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's HIP runtime initialises first, as in bench.py)

import optimizer_reference as R  # noqa: E402
from raytracedicom_amd import abi, engine, luts, robust, scenarios  # noqa: E402
from profiles.dij_run import _two_mm  # noqa: E402
from profiles.gradient_run import _hip  # noqa: E402
from profiles.optimizer_run import _event_ms  # noqa: E402

SHIFT_MM, FACTORS = 3.0, (0.965, 1.035)


def _matrix(eng, beam, dims):
    f = eng.create_field(beam, dims)
    nnz = C.c_size_t(0)
    eng._check(engine.lib().rtd_field_dose_influence(eng._h, f._h, C.c_float(0.0), C.byref(nnz)))
    f.dose_influence_prepare()
    return f, int(nnz.value)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    K = int(args[0]) if args else 200
    expected_only = "--expected" in sys.argv
    reps = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("--reps=")), 4)
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
    f0, nnz0 = _matrix(eng, beam, dims)
    _, info = f0.finish()
    lo, hi = info["dose_box_min"], info["dose_box_max"]
    dD, dW = eng.device_alloc(4 * nvox), eng.device_alloc(4 * n)
    eng.device_zero(dD, 4 * nvox)
    w0 = np.ascontiguousarray(beam.spotWeights, dtype=np.float32)
    eng.to_device(dW, w0)
    f0.dose_influence_apply(dW, dD, init=True)
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
    fields, nnz = [[f0]], [nnz0]
    shifts = [tuple(SHIFT_MM * s * (a == k) for a in range(3)) for k in range(3) for s in (1.0, -1.0)]
    for beams in robust.scenario_beams([beam], shifts):
        f, m = _matrix(eng, beams[0], dims)
        fields.append([f]); nnz.append(m)
    for factor in FACTORS:
        eng.set_luts(robust.range_scaled_luts(c3.luts, factor))
        f, m = _matrix(eng, beam, dims)
        fields.append([f]); nnz.append(m)
    eng.set_luts(c3.luts)

    def make(no_batch=False):
        if no_batch:
            os.environ["RTD_ROBUST_NO_BATCH"] = "1"
        try:
            return eng.create_voxelwise_optimizer(fields, obj)
        finally:
            os.environ.pop("RTD_ROBUST_NO_BATCH", None)
    configs = {"expected": lambda: eng.create_robust_optimizer(fields, obj, abi.RTD_ROBUST_EXPECTED)}
    if not expected_only:
        configs["voxelwise"] = lambda: make()
        configs["voxelwise_no_batch"] = lambda: make(True)
    opts = {k: mk() for k, mk in configs.items()}
    for o in opts.values():
        o.run(3)                                                      # warm-up: every kernel loaded
    eng.sync()
    ms = {k: [] for k in opts}
    for _ in range(reps):
        for k, o in opts.items():
            ms[k].append(_event_ms(hip, stream, lambda o=o: o.run(K)) / K)
    out = {"what": "voxel-wise worst-case optimiser on C3, 2 mm dose grid, S scenarios; hipEvents around run(K) / K per configuration, interleaved",
           "K": K, "reps": reps, "scenarios": len(fields), "spots": n, "nnz": nnz, "dose_dims": list(dims),
           "matrix_bytes": [16 * m for m in nnz], "volume_bytes": 4 * nvox, "volumes": 2 * len(fields),
           "ms_per_iteration": {k: [round(v, 4) for v in vs] for k, vs in ms.items()},
           "median_ms": {k: round(statistics.median(vs), 4) for k, vs in ms.items()}}
    for k, o in opts.items():
        rep, hist = o.result()
        out.setdefault("f_first", {})[k] = float(hist[0])
        out.setdefault("f_best", {})[k] = rep["f_best"]
        out.setdefault("guarded", {})[k] = rep["guarded"]
        v, lam, worst = o.scenario_values()
        out.setdefault("lambdas", {})[k] = [float(t) for t in lam]
        out.setdefault("worst", {})[k] = worst
    if "voxelwise_no_batch" in opts:
        a, b = opts["voxelwise"].result()[1], opts["voxelwise_no_batch"].result()[1]
        out["batched_equals_unbatched"] = bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
    for o in opts.values():
        o.destroy()
    obj.destroy()
    for fs in fields:
        fs[0].destroy()
    for p in (dD, dW):
        eng.device_free(p)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
