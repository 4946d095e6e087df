#!/usr/bin/env python3
"""Times the 4D block (include/rtd.h "4D dose: phases warped and summed").
Warps: n^3 -> n^3 (default 256) through fields of (n/4)^3 nodes with smooth displacements of up to 3 voxels, one field per phase, at
P = 1, 4, 10 and 16 phases:
  sum         rtd_dose_warp_sum against the sequence of P rtd_dose_warp calls (phase 0 written, the others accumulated);
  transposed  rtd_dose_warp_t_phases against the sequence of P rtd_dose_warp_t calls, each on its slice;
  copy        a device-to-device copy of the destination's bytes, beside them: not code under test.
Each is hipEvents around the call(s) on the handle's stream, the median of 7 after one warm-up, the two sides alternated inside one loop;
the fused results are compared with the sequences' bit for bit.
Optimiser: C3's field on the 2 mm dose grid (the bench field's matrix), P fields of the same beam as the phases, the fields above on
the 2 mm grid: one iteration of the 4D optimiser batched, under RTD_4D_NO_BATCH, and beside P iterations of the plain optimiser.
Usage: python profiles/fourd_run.py [N] [--reps R] [--iters K] [--out FILE]     (FILE default profiles/r31_fourd_run.json)"""
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
from raytracedicom_amd import abi, engine, fourd, luts, scenarios  # noqa: E402
from profiles.dij_run import _two_mm  # noqa: E402
from profiles.gradient_run import _hip  # noqa: E402
from profiles.optimizer_run import _event_ms  # noqa: E402
from profiles.warp_run import smooth_field  # noqa: E402

PHASES = (1, 4, 10, 16)


def phase_fields(nf, spacing, P):
    """One smooth field per phase, the amplitude growing with the phase up to 3 voxels (phase 0 is not the identity either)."""
    return [np.roll(smooth_field(nf, spacing, 3.0 * (p + 1) / P), p, axis=1 + p % 3) for p in range(P)]


def median(ts):
    return round(float(np.median(ts)), 4)


def warps_part(n, reps, hip):
    nf, spacing = n // 4, 2.0
    dims = (n, n, n)
    grid = (np.eye(3) * spacing, np.zeros(3))
    other = (np.eye(3) * spacing, np.array([0.6, -0.5, 0.25]))          # the phases' grid: the same spacing, shifted by a fraction of a voxel
    field_grid = (np.eye(3) * spacing * (n - 1) / (nf - 1), np.zeros(3))
    nbytes = 4 * n ** 3
    P_max = max(PHASES)
    rows = []
    with engine.Engine(0) as eng:
        stream = eng.stream()
        recs = fourd.phase_warps(eng, grid, other, phase_fields(nf, spacing, P_max), field_grid)
        rng = np.random.default_rng(1)
        srcs = [eng.device_alloc(nbytes) for _ in range(P_max)]
        for s in srcs:
            eng.to_device(s, (rng.random((n, n, n), dtype=np.float32) * np.float32(70.0)).astype(np.float32))
        outs = [eng.device_alloc(nbytes) for _ in range(P_max)]
        outs_seq = [eng.device_alloc(nbytes) for _ in range(P_max)]
        d_a, d_b = eng.device_alloc(nbytes), eng.device_alloc(nbytes)
        one = eng.warp_t_workspace_bytes(dims)
        d_ws = eng.device_alloc(one * P_max)
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

        def fetch(p):
            a = np.empty(n ** 3, dtype=np.uint32)
            eng.to_host(a.view(np.float32), p)
            return a
        for P in PHASES:
            r, w = list(recs)[:P], [np.float32(1.0 / P)] * P

            def fused_sum():
                eng.warp_sum_device(srcs[:P], dims, r, w, d_a, dims)

            def seq_sum():
                for p in range(P):
                    eng.warp_dose_device(srcs[p], dims, r[p], d_b, dims, scale=w[p], accumulate=1 if p else 0)

            def fused_t():
                eng.warp_dose_t_phases_device(d_a, dims, r, w, outs[:P], dims, d_ws, one * P)

            def seq_t():
                for p in range(P):
                    eng.warp_dose_t_device(d_a, dims, r[p], outs_seq[p], dims, d_ws + p * one, one, scale=w[p])

            def copy():
                assert hip.hipMemcpyAsync(d_b, d_a, nbytes, 3, stream) == 0                # hipMemcpyDeviceToDevice
            fused_sum()
            seq_sum()
            sum_equal = bool((fetch(d_a) == fetch(d_b)).all())        # (before the copy overwrites d_b)
            t = {k: [] for k in ("sum", "sum_sequence", "transposed", "transposed_sequence", "copy")}
            for i in range(reps + 1):
                for k, call in (("sum", fused_sum), ("sum_sequence", seq_sum), ("transposed", fused_t), ("transposed_sequence", seq_t), ("copy", copy)):
                    ms = _event_ms(hip, stream, call)
                    if i:
                        t[k].append(ms)
            t_equal = all(bool((fetch(outs[p]) == fetch(outs_seq[p])).all()) for p in range(P))
            row = {"phases": P, "bits_equal": {"sum": sum_equal, "transposed": t_equal}}
            row.update({k + "_ms": median(v) for k, v in t.items()})
            row["min_max_ms"] = {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}
            row["sum_over_sequence"] = round(row["sum_ms"] / row["sum_sequence_ms"], 4)
            row["transposed_over_sequence"] = round(row["transposed_ms"] / row["transposed_sequence_ms"], 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
        eng.sync()
        recs.free()
        for p in srcs + outs + outs_seq + [d_a, d_b, d_ws]:
            eng.device_free(p)
    return {"n": n, "field": nf, "reps": reps, "rows": rows}


def optimizer_part(K, reps, hip):
    es = luts.synth_luts()
    c3 = scenarios.hetero_ct(es, n=512, n_fields=1)
    beam, dims = _two_mm(c3.beams[0], 512)
    eng = engine.Engine(0)
    opt = abi.default_options()
    opt.ray_weight_cutoff = 0.0
    eng.set_options(opt)
    eng.set_luts(c3.luts)
    eng.set_ct(c3.ct)
    P_max = max(PHASES)
    fields = []
    nnz = C.c_size_t(0)
    for _ in range(P_max):
        f = eng.create_field(beam, dims)
        eng._check(engine.lib().rtd_field_dose_influence(eng._h, f._h, C.c_float(0.0), C.byref(nnz)))
        f.dose_influence_prepare()
        fields.append(f)
    nvox, n = int(np.prod(dims)), int(np.prod(beam.spotWeights.shape))
    dW, dD = eng.device_alloc(4 * n), eng.device_alloc(4 * nvox)
    eng.to_device(dW, np.ascontiguousarray(beam.spotWeights, dtype=np.float32))
    fields[0].dose_influence_apply(dW, dD, init=True)
    dose0 = np.empty((dims[2], dims[1], dims[0]), dtype=np.float32)
    eng.to_host(dose0, dD)
    z, y, x = np.meshgrid(*[np.arange(d) for d in dose0.shape], indexing="ij")
    tot = float(dose0.sum(dtype=np.float64))
    c = [float((dose0 * a).sum(dtype=np.float64)) / tot for a in (z, y, x)]
    sphere = (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= 6.0 ** 2
    rest = (dose0 > 0) & ~sphere
    level = float(dose0[sphere].mean())
    obj = eng.create_objective(dims)
    obj.add_roi(sphere.reshape(-1))
    obj.add_roi(rest.reshape(-1))
    obj.add_term(R.SQ_DEVIATION, 0, 1.0, level)
    obj.add_term(R.SQ_OVERDOSE, 1, 1.0, 0.3 * level)
    stream = eng.stream()
    spacing = 2.0
    grid = (np.eye(3) * spacing, np.zeros(3))
    nf = dims[0] // 4
    field_grid = (np.eye(3) * spacing * (dims[0] - 1) / (nf - 1), np.zeros(3))
    recs = fourd.phase_warps(eng, grid, grid, phase_fields(nf, spacing, P_max), field_grid)
    plain = eng.create_optimizer([fields[0]], obj)
    plain.run(3)
    eng.sync()
    rows = []
    for P in PHASES:
        os.environ.pop("RTD_4D_NO_BATCH", None)
        batched = eng.create_4d_optimizer([[f] for f in fields[:P]], list(recs)[:P], obj)
        os.environ["RTD_4D_NO_BATCH"] = "1"                           # (read when the optimiser is made)
        sequence = eng.create_4d_optimizer([[f] for f in fields[:P]], list(recs)[:P], obj)
        os.environ.pop("RTD_4D_NO_BATCH", None)
        t = {"batched": [], "no_batch": [], "plain": []}
        for i in range(reps + 1):
            for k, o in (("batched", batched), ("no_batch", sequence), ("plain", plain)):
                ms = _event_ms(hip, stream, lambda: o.run(K)) / K
                if i:
                    t[k].append(ms)
        hb, hs = batched.result()[1], sequence.result()[1]
        row = {"phases": P, "batched_ms_per_iteration": median(t["batched"]), "no_batch_ms_per_iteration": median(t["no_batch"]),
               "plain_ms_per_iteration": median(t["plain"]), "histories_equal": bool(np.array_equal(hb.view(np.uint64), hs.view(np.uint64)))}
        row["min_max_ms"] = {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}
        row["phases_times_plain_ms"] = round(P * row["plain_ms_per_iteration"], 4)
        row["batched_over_no_batch"] = round(row["batched_ms_per_iteration"] / row["no_batch_ms_per_iteration"], 4)
        row["batched_over_phases_times_plain"] = round(row["batched_ms_per_iteration"] / row["phases_times_plain_ms"], 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
        batched.destroy()
        sequence.destroy()
    plain.destroy()
    obj.destroy()
    recs.free()
    for f in fields:
        f.destroy()
    for p in (dW, dD):
        eng.device_free(p)
    eng.close()
    return {"K": K, "reps": reps, "spots": n, "nnz": int(nnz.value), "dose_dims": list(dims), "rows": rows}


def main():
    flags = sys.argv[1:]
    n = int(flags[0]) if flags and not flags[0].startswith("--") else 256
    reps = int(flags[flags.index("--reps") + 1]) if "--reps" in flags else 7
    K = int(flags[flags.index("--iters") + 1]) if "--iters" in flags else 50
    out_path = flags[flags.index("--out") + 1] if "--out" in flags else os.path.join(ROOT, "profiles", "r31_fourd_run.json")
    torch.cuda.init()
    hip = _hip()
    result = {"what": "the fused phase warps against the per-phase sequences (medians of %d after a warm-up, alternated), and one iteration of the "
                      "4D optimiser batched, under RTD_4D_NO_BATCH and beside P plain iterations, on C3's 2 mm matrix" % reps,
              "warps": warps_part(n, reps, hip), "optimizer": optimizer_part(K, reps, hip)}
    text = json.dumps(result, indent=1)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print("written", out_path, flush=True)


if __name__ == "__main__":
    main()
