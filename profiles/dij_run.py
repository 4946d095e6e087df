#!/usr/bin/env python3
"""Times rtd_field_dose_influence (the dose-influence matrix) with hipEvents around the call, on C3 (512^3 heterogeneous CT, 10x10
spots x 20 layers) on a 2 mm dose grid and on its native grid, and on C2 (256^3 water cube, 33x33 spots x 20 layers); inputs
resident, ray_weight_cutoff = 0, threshold 0. Records batches, nnz, bytes of the CSC, ms, ms per batch and one cold forward of the
field. Prints one JSON line; with rocprofv3 --kernel-trace --stats in front, the per-kernel split. Usage: python profiles/dij_run.py [K]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (torch's HIP runtime initialises first, as in bench.py)

from raytracedicom_amd import abi, engine, luts, scenarios  # noqa: E402
from profiles.gradient_run import _hip  # noqa: E402


def _two_mm(b, n):
    """The beam's dose grid coarsened to 2 mm (voxel 256 / n mm): dose index = ct index * (voxel / 2) + (voxel / 2 - 1) / 2."""
    r = (256.0 / n) / 2.0
    t = b.gantryToDoseIdx
    g = scenarios.Float3AffineTransform(r * t.m, r * t.v + 0.5 * (r - 1.0))
    return b.replace(gantryToDoseIdx=g), (128, 128, 128)


def run(name, scn, beam, dims, steps, hip):
    torch.cuda.synchronize()
    eng = engine.Engine(0)
    opt = abi.default_options()
    opt.ray_weight_cutoff = 0.0
    eng.set_options(opt)
    eng.set_luts(scn.luts)
    eng.set_ct(scn.ct)
    n = dims[0] * dims[1] * dims[2]
    d = eng.device_alloc(4 * n)
    f = eng.create_field(beam, dims)
    eng.device_zero(d, 4 * n)
    f.compute(d)
    t, info = f.finish()
    cold = t["total_ms"]
    eng.device_zero(d, 4 * n)
    f.compute(d)
    warm = f.finish()[0]["total_ms"]
    L = engine.lib()
    nnz = C.c_size_t(0)
    s = C.c_void_p(eng.stream())
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip.hipEventCreate(C.byref(e0)); hip.hipEventCreate(C.byref(e1))
    ms = []
    for _ in range(steps):
        hip.hipEventRecord(e0, s)
        eng._check(L.rtd_field_dose_influence(eng._h, f._h, C.c_float(0.0), C.byref(nnz)))
        hip.hipEventRecord(e1, s)
        hip.hipEventSynchronize(e1)
        v = C.c_float()
        hip.hipEventElapsedTime(C.byref(v), e0, e1)
        ms.append(v.value)
    batch = f.fetch("dij_batch")
    nb = int(batch.max()) + 1
    n_spots = int(batch.size)
    ms.sort()
    out = {"case": name, "dose_dims": list(dims), "spots": n_spots, "empty_columns": int((batch < 0).sum()), "batches": nb,
           "spots_per_batch_max": int(max((batch == k).sum() for k in range(nb))) if nb else 0,
           "nnz": int(nnz.value), "csc_bytes": int(8 * (n_spots + 1) + 8 * nnz.value),
           "ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_per_batch": ms[len(ms) // 2] / max(nb, 1),
           "forward_cold_ms": cold, "forward_warm_ms": warm, "max_radius": info["max_radius"], "steps": steps}
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    f.destroy()
    eng.device_free(d)
    eng.close()
    return out


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    hip = _hip()
    es = luts.synth_luts()
    res = []
    c3 = scenarios.hetero_ct(es, n=512, n_fields=1)
    b2, dims2 = _two_mm(c3.beams[0], 512)
    res.append(run("C3 2mm dose grid", c3, b2, dims2, steps, hip))
    res.append(run("C3 native grid", c3, c3.beams[0], c3.dims, steps, hip))
    del c3
    c2 = scenarios.water_cube(es, n=256, n_layers=20)
    res.append(run("C2", c2, c2.beams[0], c2.dims, steps, hip))
    print(json.dumps({"dij": res}))


if __name__ == "__main__":
    main()
