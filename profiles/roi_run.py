#!/usr/bin/env python3
"""Times rtd_roi_rasterize on two structures:
  large   elliptical contours of 2000 points on 300 planes, on a 512 x 512 x 300 grid (one plane per slice);
  small   contours of 64 points on 20 planes in the middle of the same grid.
Per structure: kernel_ms, the hipEvents the call itself records around its kernels (scan, count, the two scan steps, emit); wall_ms, the
wall clock around the whole synchronous call (transform and planes on the host, allocations, copies, kernels, the wait); fill_mask_ms,
hipEvents around one rtd_roi_fill_mask launch. One warm-up call, then N timed ones: median, min and max. The baseline is the scanline
of the restatement vectorised with numpy (per plane: the crossings of every row sorted, the columns between them filled), on the same
input on this machine's CPU, checked for equality with the device's list. Prints one JSON line.
Usage: python profiles/roi_run.py [N]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's HIP runtime initialises first, as in bench.py)

import roi_reference as R  # noqa: E402
from raytracedicom_amd import engine  # noqa: E402
from profiles.gradient_run import _hip  # noqa: E402
from profiles.optimizer_run import _event_ms  # noqa: E402


def numpy_scanline(dims, m, v, contours, thickness):
    """The rule of include/rtd.h by rows instead of by voxels: per row the crossings xc of the plane's edges, c = clamp(ceil(xc), 0, nx)
    counted into a difference array, a suffix parity over it. Equal to roi_reference.rasterize."""
    nx, ny, nz = dims
    planes = R.planes_of(m, v, contours)
    take = R.assign_slices([p[0] for p in planes], nz, R.slab_of(m, thickness))
    rows = np.arange(ny, dtype=np.float64)
    masks = {}
    vol = np.zeros((nz, ny, nx), dtype=bool)
    for k in range(nz):
        p = int(take[k])
        if p < 0:
            continue
        if p not in masks:
            au, av, bu, bv = R.edges_of(planes[p][1])
            cross = (av[None, :] <= rows[:, None]) != (bv[None, :] <= rows[:, None])
            jj, ee = np.nonzero(cross)
            t = (rows[jj] - av[ee]) / (bv[ee] - av[ee])
            xc = au[ee] + t * (bu[ee] - au[ee])
            c = np.clip(np.ceil(xc), 0, nx).astype(np.int64)
            diff = np.zeros((ny, nx + 1), dtype=np.int64)
            np.add.at(diff, (jj, c), 1)
            above = diff[:, ::-1].cumsum(axis=1)[:, ::-1]             # above[j][b] = crossings with c >= b
            masks[p] = (above[:, 1:] & 1).astype(bool)                # voxel i is flipped by the crossings with c > i
        vol[k] = masks[p]
    return np.flatnonzero(vol).astype(np.int32)


def spread(ms):
    ms = sorted(ms)
    return {"median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    N = int(args[0]) if args else 7
    torch.cuda.init()
    hip = _hip()
    dims = (512, 512, 300)
    m, v = R.IDENTITY
    rng = np.random.default_rng(0)
    large = [R.circle(256.3 + 5.0 * rng.random(), 250.7 + 5.0 * rng.random(), 150.0 + 40.0 * np.sin(0.02 * k), 2000, float(k), ry=110.0 + 30.0 * np.cos(0.03 * k))
             for k in range(300)]
    small = [R.circle(300.2, 200.4, 9.0 + 0.3 * k, 64, float(140 + k), ry=7.0) for k in range(20)]
    out = {"what": "rtd_roi_rasterize; kernel_ms = hipEvents around its kernels, wall_ms = the whole call", "N": N, "dims": list(dims)}
    eng = engine.Engine(0)
    mask = torch.empty(int(np.prod(dims)), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for name, contours in (("large", large), ("small", small)):
        eng.rasterize_roi(dims, (m, v), contours, 1.0).close()        # warm-up: the kernels loaded
        kern, wall, vox, info = [], [], None, None
        for _ in range(N):
            t0 = time.perf_counter()
            roi = eng.rasterize_roi(dims, (m, v), contours, 1.0)
            wall.append(1e3 * (time.perf_counter() - t0))
            kern.append(roi.kernel_ms())
            if vox is None:
                vox, info = roi.voxels(), roi.info
                roi.fill_mask(mask)
                eng.sync()
                fill = [_event_ms(hip, eng.stream(), lambda: roi.fill_mask(mask)) for _ in range(N)]
            roi.close()
        t0 = time.perf_counter()
        ref = numpy_scanline(dims, m, v, contours, 1.0)
        numpy_ms = 1e3 * (time.perf_counter() - t0)
        out[name] = {"contours": len(contours), "points": int(sum(len(c) for c in contours)), "n_voxels": info["n_voxels"],
                     "slices_covered": info["n_slices_covered"], "kernel_ms": spread(kern), "wall_ms": spread(wall), "fill_mask_ms": spread(fill),
                     "numpy_scanline_ms": round(numpy_ms, 1), "equal_to_numpy": bool(np.array_equal(vox, ref)),
                     "launches": {"rasterize": 5 if info["n_voxels"] else 4, "fill_mask": 1}}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
