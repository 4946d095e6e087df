#!/usr/bin/env python3
"""Times the robust and the voxel-wise optimiser on the compact dose-influence matrix (rtd_optimizer_create_robust_compact,
rtd_optimizer_create_voxelwise_compact) beside their plain siblings, in the setting of profiles/robust_run.py: C3 (512^3 heterogeneous
CT, one field of 10x10 spots x 20 layers), 2 mm dose grid, a spherical target (SQ_DEVIATION) and the rest of the dose box
(SQ_OVERDOSE). Nine fields are computed once: nominal, the patient displaced by +-3 mm along each gantry axis, the stopping-power table
scaled by 0.965 and 1.035 (raytracedicom_amd/robust.py). S = 9 uses all of them, S = 5 the nominal one, +-3 mm along x and the two
range factors. Per S and configuration, hipEvents on the engine's stream around run(K) of a fresh optimiser (after a warm-up
optimiser of 3 iterations), `reps` times, the configurations interleaved within a repetition:
  expected, worst_case, voxelwise                      the plain optimisers, launches batched over the scenario axis;
  expected_no_batch                                    the plain EXPECTED one with RTD_ROBUST_NO_BATCH;
  compact_expected, compact_worst_case, compact_voxelwise, compact_expected_no_batch, compact_worst_case_no_batch
                                                       the same on the compact forms.
Every run starts from the fields' own weights, so f_best after K iterations stands beside the plain optimiser's from the same start.
The bytes are those rtd_field_dose_influence_compact_info reports, summed over the S fields. `--parent` keeps to the calls an older
build of the library has (the plain configurations), so that the same file times the parent commit's build.
Prints one JSON line. Usage: python profiles/robust_compact_run.py [K] [--parent] [--reps=N]"""
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
SETS = {5: (0, 1, 2, 7, 8), 9: tuple(range(9))}


def _matrix(eng, beam, dims):
    f = eng.create_field(beam, dims)
    nnz = C.c_size_t(0)
    eng._check(engine.lib().rtd_field_dose_influence(eng._h, f._h, C.c_float(0.0), C.byref(nnz)))
    f.dose_influence_prepare()
    return f, int(nnz.value)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    K = int(args[0]) if args else 200
    parent = "--parent" in sys.argv
    reps = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("--reps=")), 3)
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
    eng.to_device(dW, np.ascontiguousarray(beam.spotWeights, dtype=np.float32))
    f0.dose_influence_apply(dW, dD, init=True)
    dose0 = np.empty((dims[2], dims[1], dims[0]), dtype=np.float32)
    eng.to_host(dose0, dD)
    z, y, x = np.meshgrid(*[np.arange(d) for d in dose0.shape], indexing="ij")
    tot = float(dose0.sum(dtype=np.float64))
    c = [float((dose0 * a).sum(dtype=np.float64)) / tot for a in (z, y, x)]
    sphere = (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= 6.0 ** 2
    box = np.zeros(dose0.shape, dtype=bool)
    box[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    level = float(dose0[sphere].mean())
    obj = eng.create_objective(dims)
    obj.add_term(R.SQ_DEVIATION, obj.add_roi(sphere.reshape(-1)), 1.0, level)
    obj.add_term(R.SQ_OVERDOSE, obj.add_roi((box & ~sphere).reshape(-1)), 1.0, 0.3 * level)
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
    infos = []
    if not parent:
        for fs in fields:
            fs[0].dose_influence_compact()
            infos.append(fs[0].dose_influence_compact_info())

    def no_batch(create):
        os.environ["RTD_ROBUST_NO_BATCH"] = "1"
        try:
            return create()
        finally:
            os.environ.pop("RTD_ROBUST_NO_BATCH", None)
    out = {"what": "robust and voxel-wise optimisers on C3, 2 mm dose grid, plain and compact matrices; hipEvents around run(K) / K of a fresh "
                   "optimiser per configuration and repetition, interleaved",
           "K": K, "reps": reps, "spots": n, "dose_dims": list(dims), "nnz": nnz, "volume_bytes": 4 * nvox, "sets": []}
    EXP, WC = abi.RTD_ROBUST_EXPECTED, abi.RTD_ROBUST_WORST_CASE
    for S, which in SETS.items():
        sf = [fields[k] for k in which]
        configs = {"expected": lambda: eng.create_robust_optimizer(sf, obj, EXP),
                   "worst_case": lambda: eng.create_robust_optimizer(sf, obj, WC),
                   "voxelwise": lambda: eng.create_voxelwise_optimizer(sf, obj),
                   "expected_no_batch": lambda: no_batch(lambda: eng.create_robust_optimizer(sf, obj, EXP))}
        if not parent:
            configs.update({"compact_expected": lambda: eng.create_robust_compact_optimizer(sf, obj, EXP),
                            "compact_worst_case": lambda: eng.create_robust_compact_optimizer(sf, obj, WC),
                            "compact_voxelwise": lambda: eng.create_voxelwise_compact_optimizer(sf, obj),
                            "compact_expected_no_batch": lambda: no_batch(lambda: eng.create_robust_compact_optimizer(sf, obj, EXP)),
                            "compact_worst_case_no_batch": lambda: no_batch(lambda: eng.create_robust_compact_optimizer(sf, obj, WC))})
        for mk in configs.values():                                   # warm-up: every kernel loaded
            o = mk()
            o.run(3)
            eng.sync()
            o.destroy()
        ms = {k: [] for k in configs}
        last = {}
        for _ in range(reps):
            for k, mk in configs.items():
                o = mk()
                o.run(0)
                eng.sync()
                ms[k].append(_event_ms(hip, stream, lambda o=o: o.run(K)) / K)
                rep, hist = o.result()
                last[k] = {"f_first": float(hist[0]), "f_best": rep["f_best"], "f_last": rep["f_last"], "guarded": rep["guarded"],
                           "history_bits": hist.view(np.uint64).tolist()}
                o.destroy()
        rec = {"scenarios": S, "fields": list(which),
               "ms_per_iteration": {k: [round(v, 4) for v in vs] for k, vs in ms.items()},
               "median_ms": {k: round(statistics.median(vs), 4) for k, vs in ms.items()},
               "f_first": {k: v["f_first"] for k, v in last.items()}, "f_best": {k: v["f_best"] for k, v in last.items()},
               "f_last": {k: v["f_last"] for k, v in last.items()}, "guarded": {k: v["guarded"] for k, v in last.items()},
               "plain_bytes": sum(16 * nnz[k] for k in which)}
        rec["batched_equals_unbatched"] = {"plain_expected": last["expected"]["history_bits"] == last["expected_no_batch"]["history_bits"]}
        if not parent:
            rec["compact_bytes"] = sum(infos[k]["compact_bytes"] for k in which)
            rec["plain_bytes_reported"] = sum(infos[k]["plain_bytes"] for k in which)
            rec["row_bits"] = sorted({infos[k]["row_bits"] for k in which})
            for k in ("expected", "worst_case"):
                rec["batched_equals_unbatched"]["compact_" + k] = last["compact_" + k]["history_bits"] == last["compact_" + k + "_no_batch"]["history_bits"]
            rec["compact_over_plain"] = {k: round(rec["median_ms"]["compact_" + k] / rec["median_ms"][k], 4) for k in ("expected", "worst_case", "voxelwise")}
        out["sets"].append(rec)
    obj.destroy()
    for fs in fields:
        fs[0].destroy()
    for p in (dD, dW):
        eng.device_free(p)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
