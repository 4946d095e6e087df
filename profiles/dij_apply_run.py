#!/usr/bin/env python3
"""Times the products with the resident dose-influence matrix (rtd_field_dose_influence_prepare / _apply / _apply_t) with hipEvents
on the engine's stream, on C3 (512^3 heterogeneous CT, 10x10 spots x 20 layers) with a 2 mm dose grid and, if the device has the
memory free, on its native grid; inputs resident, ray_weight_cutoff = 0, threshold 0. In the same run: the forward
(rtd_field_compute) and the gradient (rtd_field_spot_gradient) of the same field — the only other way to the same two vectors on
the device. Reports bytes streamed (8 per entry) / time as a fraction of 8 TB/s, what prepare costs, and for the 2 mm case the
row-length histogram. Prints one JSON line; with rocprofv3 --kernel-trace --stats in front, the per-kernel split.
Usage: python profiles/dij_apply_run.py [K] [--no-native]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's HIP runtime initialises first, as in bench.py)

from raytracedicom_amd import abi, engine, luts, scenarios  # noqa: E402
from profiles.dij_run import _two_mm  # noqa: E402
from profiles.gradient_run import _hip  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
NATIVE_BYTES_NEEDED = 120e9      # 31 GB each for CSC, staging (up to 2x while it grows) and companion, plus workspace: an estimate


class Timer:
    def __init__(self, hip, stream):
        self.hip, self.s = hip, C.c_void_p(stream)
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        hip.hipEventCreate(C.byref(self.e0)); hip.hipEventCreate(C.byref(self.e1))

    def ms(self, call, steps, warmup=3):
        for _ in range(warmup):
            call()
        out = []
        for _ in range(steps):
            self.hip.hipEventRecord(self.e0, self.s)
            call()
            self.hip.hipEventRecord(self.e1, self.s)
            self.hip.hipEventSynchronize(self.e1)
            v = C.c_float()
            self.hip.hipEventElapsedTime(C.byref(v), self.e0, self.e1)
            out.append(v.value)
        return {"median": round(float(np.median(out)), 4), "min": round(float(np.min(out)), 4), "max": round(float(np.max(out)), 4)}

    def close(self):
        self.hip.hipEventDestroy(self.e0); self.hip.hipEventDestroy(self.e1)


def run(name, scn, beam, dims, steps, hip, histogram):
    torch.cuda.synchronize()
    eng = engine.Engine(0)
    opt = abi.default_options()
    opt.ray_weight_cutoff = 0.0
    eng.set_options(opt)
    eng.set_luts(scn.luts)
    eng.set_ct(scn.ct)
    n = dims[0] * dims[1] * dims[2]
    n_spots = int(beam.spotWeights.size)
    d, dg = eng.device_alloc(4 * n), eng.device_alloc(4 * n)
    dw, dout = eng.device_alloc(4 * n_spots), eng.device_alloc(4 * n_spots)
    rng = np.random.default_rng(1)
    eng.to_device(dg, rng.random((dims[2], dims[1], dims[0]), dtype=np.float32) - np.float32(0.5))
    eng.to_device(dw, np.ascontiguousarray(beam.spotWeights, dtype=np.float32))
    eng.device_zero(d, 4 * n)
    f = eng.create_field(beam, dims)
    tm = Timer(hip, eng.stream())
    forward = tm.ms(lambda: f.compute(d), steps)
    _, info = f.finish()
    gradient = tm.ms(lambda: f.spot_gradient(dg, dout), steps)
    t0 = time.perf_counter()
    dij = f.dose_influence() if histogram else None                  # (the host copy only where the histogram is wanted)
    if dij is None:
        nnz_c = C.c_size_t(0)
        eng._check(engine.lib().rtd_field_dose_influence(eng._h, f._h, C.c_float(0.0), C.byref(nnz_c)))
    matrix_s = time.perf_counter() - t0
    nnz = f.dose_influence_device()[3]
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.perf_counter()
    f.dose_influence_prepare()                                        # synchronous
    prepare_ms = 1e3 * (time.perf_counter() - t0)
    prepare_bytes = free0 - torch.cuda.mem_get_info()[0]
    apply_init = tm.ms(lambda: f.dose_influence_apply(dw, d, init=True), steps)
    apply_add = tm.ms(lambda: f.dose_influence_apply(dw, d, init=False), steps)
    apply_t = tm.ms(lambda: f.dose_influence_apply_t(dg, dout), steps)

    def pair():
        f.dose_influence_apply(dw, d, init=True)
        f.dose_influence_apply_t(dg, dout)
    both = tm.ms(pair, steps)
    lo, hi = info["dose_box_min"], info["dose_box_max"]
    box_voxels = int(np.prod([max(hi[i] - lo[i] + 1, 0) for i in range(3)]))
    frac = lambda t: round(8.0 * nnz / (1e-3 * t["median"]) / PEAK_BYTES_PER_S, 4)   # noqa: E731
    out = {"case": name, "dose_dims": list(dims), "spots": n_spots, "nnz": int(nnz), "dose_box_voxels": box_voxels,
           "entry_bytes_streamed_per_product": int(8 * nnz),
           "matrix_s_host_clock": round(matrix_s, 3), "prepare_ms_host_clock": round(prepare_ms, 2), "prepare_device_bytes": int(prepare_bytes),
           "apply_init_ms": apply_init, "apply_add_ms": apply_add, "apply_t_ms": apply_t, "apply_plus_apply_t_ms": both,
           "forward_ms": forward, "gradient_ms": gradient,
           "forward_plus_gradient_ms_median": round(forward["median"] + gradient["median"], 4),
           "speedup_of_the_pair": round((forward["median"] + gradient["median"]) / both["median"], 2),
           "apply_fraction_of_8TBps": frac(apply_init), "apply_t_fraction_of_8TBps": frac(apply_t), "steps": steps}
    if dij is not None:
        rows = np.bincount(dij.indices, minlength=n)
        rows = rows[rows > 0]
        edges = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 1 << 30]
        out["row_length_histogram"] = {"%d..%d" % (a, b - 1) if b < (1 << 30) else ">=%d" % a: int(((rows >= a) & (rows < b)).sum())
                                       for a, b in zip(edges, edges[1:])}
        out["rows_with_entries"] = int(rows.size)
        out["row_length_mean_median_max"] = [round(float(rows.mean()), 1), int(np.median(rows)), int(rows.max())]
        cols = np.diff(dij.indptr)
        out["column_length_mean_max_empty"] = [round(float(cols.mean()), 1), int(cols.max()), int((cols == 0).sum())]
        del dij
    tm.close()
    f.destroy()
    for p in (d, dg, dw, dout):
        eng.device_free(p)
    eng.close()
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    steps = int(args[0]) if args else 20
    torch.cuda.init()
    hip = _hip()
    es = luts.synth_luts()
    c3 = scenarios.hetero_ct(es, n=512, n_fields=1)
    b2, dims2 = _two_mm(c3.beams[0], 512)
    res = [run("C3 2mm dose grid", c3, b2, dims2, steps, hip, histogram=True)]
    free, total = torch.cuda.mem_get_info()
    native = {"case": "C3 native grid", "device_bytes_free": int(free), "device_bytes_total": int(total), "bytes_wanted": int(NATIVE_BYTES_NEEDED)}
    if "--no-native" in sys.argv:
        native["status"] = "not run: switched off"
    elif free < NATIVE_BYTES_NEEDED:
        native["status"] = "not run: memory"
    else:
        native.update(run("C3 native grid", c3, c3.beams[0], c3.dims, steps, hip, histogram=False))
        native["status"] = "run"
    res.append(native)
    print(json.dumps({"what": "products with the resident dose-influence matrix; hipEvents on the engine's stream, median / min / max ms over "
                              "`steps` calls after 3 warm-up calls; fractions are 8 bytes per entry / median time / 8 TB/s",
                      "dij_apply": res}))


if __name__ == "__main__":
    main()
