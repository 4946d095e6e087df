#!/usr/bin/env python3
"""Times rtd_field_project_target and rtd_field_select_spots with hipEvents on the engine's stream, on C3 (512^3 heterogeneous CT, 10x10
spots x 20 layers, 512 steps: 512 x 96 x 88 samples to project) with a sphere target of 40 mm radius at the isocentre on the field's own
dose grid, next to one warm forward of the same field in the same run; ray_weight_cutoff = 0. project is a synchronous call (it returns
the summary): its figure holds the launch, the copy of the record and the wait. select is timed as launches only, at zero margins and
at (lateral 6, proximal 2, distal 5) mm, and once more with the count. Writes profiles/r14_target_run.json and prints the same JSON
line; with rocprofv3 --kernel-trace --stats in front, the per-kernel split. Usage: python profiles/target_run.py [K]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: F401,E402  (torch's HIP runtime initialises first, as in bench.py)

from raytracedicom_amd import abi, engine, luts, scenarios  # noqa: E402
from profiles.gradient_run import _hip  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "r14_target_run.json")
MARGINS = ((0.0, 0.0, 0.0), (6.0, 2.0, 5.0))    # (lateral, proximal, distal) mm


def _sphere(n, radius_mm):
    """uint8 [Z][Y][X] on the C3 grid (voxel 256 / n mm, origin (-128, -128, -106)): voxel centres within radius_mm of the isocentre."""
    voxel = 256.0 / n
    ax = np.arange(n, dtype=np.float32) * np.float32(voxel)
    x, y, z = (ax - 128.0)[None, None, :], (ax - 128.0)[None, :, None], (ax - 106.0)[:, None, None]
    return ((x * x + y * y + z * z) <= radius_mm * radius_mm).astype(np.uint8)


def _stats(ms):
    ms = sorted(ms)
    return {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    hip = _hip()
    es = luts.synth_luts()
    scn = scenarios.hetero_ct(es, n=512, n_fields=1)
    beam, dims = scn.beams[0], scn.dims
    mask = _sphere(512, 40.0)
    torch.cuda.synchronize()
    eng = engine.Engine(0)
    opt = abi.default_options()
    opt.ray_weight_cutoff = 0.0
    eng.set_options(opt)
    eng.set_luts(es)
    eng.set_ct(scn.ct)
    n = scn.n_voxels
    d_dose, d_mask, d_sel = eng.device_alloc(4 * n), eng.device_alloc(n), eng.device_alloc(beam.spotWeights.size)
    eng.to_device(d_mask, mask)
    f = eng.create_field(beam, dims)
    fwd = []
    for _ in range(3):                                               # the last one is warm: trace and plan reused
        eng.device_zero(d_dose, 4 * n)
        f.compute(d_dose)
        t, info = f.finish()
        fwd.append(t["total_ms"])
    L = engine.lib()
    s = C.c_void_p(eng.stream())
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip.hipEventCreate(C.byref(e0)); hip.hipEventCreate(C.byref(e1))

    def timed(call, reps):
        ms = []
        for _ in range(reps):
            hip.hipEventRecord(e0, s)
            call()
            hip.hipEventRecord(e1, s)
            hip.hipEventSynchronize(e1)
            v = C.c_float()
            hip.hipEventElapsedTime(C.byref(v), e0, e1)
            ms.append(v.value)
        return ms

    ti = abi.RtdTargetInfo()
    project = lambda: eng._check(L.rtd_field_project_target(eng._h, f._h, C.c_void_p(d_mask), C.byref(ti)))  # noqa: E731
    project()                                                         # the first call allocates
    out = {"case": "C3 native grid, sphere r = 40 mm at the isocentre", "ray_dims": info["ray_dims"], "steps": int(beam.tracerSteps),
           "spots": int(beam.spotWeights.size), "mask_voxels": int(mask.sum()), "reps": steps,
           "forward_first_ms": fwd[0], "forward_warm_ms": fwd[-1], "project": _stats(timed(project, steps)), "target": ti.as_dict(), "select": []}
    for lateral, proximal, distal in MARGINS:
        o = abi.RtdTargetOptions()
        o.lateral_margin_mm, o.proximal_margin_mm, o.distal_margin_mm = lateral, proximal, distal
        cnt = C.c_uint32(0)
        launch = lambda: eng._check(L.rtd_field_select_spots(eng._h, f._h, C.byref(o), C.c_void_p(d_sel), None))  # noqa: E731
        counted = lambda: eng._check(L.rtd_field_select_spots(eng._h, f._h, C.byref(o), C.c_void_p(d_sel), C.byref(cnt)))  # noqa: E731
        launch()
        rec = {"margins_mm": [lateral, proximal, distal], "launches_only": _stats(timed(launch, steps)), "with_count": _stats(timed(counted, steps)),
               "n_selected": int(cnt.value)}
        out["select"].append(rec)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    f.destroy()
    for p in (d_dose, d_mask, d_sel):
        eng.device_free(p)
    eng.close()
    line = json.dumps({"target": out})
    with open(OUT, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
