#!/usr/bin/env python3
"""Times rtd_field_spot_gradient (the transposed dose path) with hipEvents on the engine's stream, at C3 (512^3 heterogeneous CT,
10x10 spots x 20 layers) and C2 (the reference's 256^3 water cube, 33x33 spots x 20 layers), inputs resident, after one forward
compute of the field; ray_weight_cutoff = 0 (what an optimiser uses). Prints one JSON line; with rocprofv3 --kernel-trace --stats in
front, the per-kernel split. Usage: python profiles/gradient_run.py [K]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from raytracedicom_amd import abi, engine, luts, scenarios


def _hip():
    h = C.CDLL("libamdhip64.so")                                     # the runtime the engine is linked against
    for n in ("hipEventCreate", "hipEventRecord", "hipEventSynchronize", "hipEventElapsedTime", "hipEventDestroy"):
        getattr(h, n).restype = C.c_int
    h.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    h.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    h.hipEventSynchronize.argtypes = [C.c_void_p]
    h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    h.hipEventDestroy.argtypes = [C.c_void_p]
    return h


def run(name, scn, steps, hip):
    eng = engine.Engine(0)
    opt = abi.default_options()
    opt.ray_weight_cutoff = 0.0
    eng.set_options(opt)
    eng.set_luts(scn.luts)
    eng.set_ct(scn.ct)
    n = scn.n_voxels
    d, dg = eng.device_alloc(4 * n), eng.device_alloc(4 * n)
    b = scn.beams[0]
    dout = eng.device_alloc(4 * b.spotWeights.size)
    eng.to_device(dg, np.random.default_rng(1).random(scn.ct.shape, dtype=np.float32))
    f = eng.create_field(b, scn.dims)
    fwd = []
    for _ in range(3):                                               # forward, for the comparison (the last one is the gradient's)
        eng.device_zero(d, 4 * n)
        f.compute(d)
        t, info = f.finish()
        fwd.append(t["total_ms"])
    for _ in range(3):
        f.spot_gradient(dg, dout)
    eng.sync()
    s = C.c_void_p(eng.stream())
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip.hipEventCreate(C.byref(e0)); hip.hipEventCreate(C.byref(e1))
    ms = []
    for _ in range(steps):
        hip.hipEventRecord(e0, s)
        f.spot_gradient(dg, dout)
        hip.hipEventRecord(e1, s)
        hip.hipEventSynchronize(e1)
        v = C.c_float()
        hip.hipEventElapsedTime(C.byref(v), e0, e1)
        ms.append(v.value)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    W, H, L = info["ray_dims"]
    out = {"workload": name, "ray_grid": [W, H, L], "live_steps": info["live_steps"], "max_radius": info["max_radius"],
           "uniform_sigma": info["uniform_sigma"], "gradient_ms_median": round(float(np.median(ms)), 4),
           "gradient_ms_min": round(float(np.min(ms)), 4), "gradient_ms_mean": round(float(np.mean(ms)), 4),
           "forward_ms_one_field": round(float(np.median(fwd)), 4), "steps": steps}
    f.destroy()
    for p in (d, dg, dout):
        eng.device_free(p)
    eng.close()
    return out


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    torch.cuda.init()
    hip = _hip()
    es = luts.synth_luts()
    res = {"what": "rtd_field_spot_gradient, hipEvents around the call on the engine's stream (transfer^T, fill^T + superposition^T, "
                   "reduce, conv^T), after a forward compute of the field; ray_weight_cutoff = 0; target 1.2 ms per C3 field",
           "c3": run("C3: 512^3 heterogeneous CT, 10x10 spots x 20 layers", scenarios.hetero_ct(es, n=512), steps, hip),
           "c2": run("C2: reference water cube 256^3, 33x33 spots x 20 layers", scenarios.water_cube(es, n=256, n_layers=20), steps, hip)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
