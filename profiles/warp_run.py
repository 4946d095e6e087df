#!/usr/bin/env python3
"""Times deformable dose warping on the device (rtd_dose_warp, rtd_dose_warp_t) on n^3 -> n^3 (default 512) through a field of
(n/4)^3 nodes (4-voxel field spacing) whose displacements are smooth and a few voxels large, the shape of a breathing-phase
registration. Beside them, on the same stream:
  resample   rtd_dose_resample with the warp's affine map alone: the forward kernel without its field level;
  copy       a device-to-device copy of the destination's bytes between two events: not code under test, and neither direction can be
             faster than moving those bytes once.
The transposed call is timed launch by launch (rtd_dose_warp_t_kernel_ms: memset of the workspace, maximum, scatter, finish), once
with the scatter that merges a block's contributions in an LDS tile and once with plain atomics (a handle made under
RTD_WARP_T_PLAIN); the two results are compared bit for bit. Every time is the smallest and the median of the repeats after one warm-up call.
Usage: python profiles/warp_run.py [N] [--reps R] [--out FILE]     (FILE default profiles/r26_warp_run.json)"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def hip_runtime():
    """The HIP runtime the engine library has loaded (the same copy: events and copies must come from the runtime that owns the stream)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            L = C.CDLL(line.split()[-1])
            L.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
            L.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
            L.hipEventSynchronize.argtypes = [C.c_void_p]
            L.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
            L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
            return L
    sys.exit("the engine library has not loaded a HIP runtime")


def smooth_field(nf, spacing_mm, amplitude_voxels):
    """[3][nf][nf][nf] float32 in mm: one period of a sine per axis and component, out of phase with each other."""
    i = np.arange(nf, dtype=np.float64) / (nf - 1)
    z, y, x = np.meshgrid(i, i, i, indexing="ij")
    a = amplitude_voxels * spacing_mm
    return np.stack([a * np.sin(2 * np.pi * (y + 0.3 * z)) * np.cos(np.pi * x), a * np.sin(2 * np.pi * (z + 0.2 * x) + 1.0),
                     0.6 * a * np.cos(2 * np.pi * (x + y) + 2.0)]).astype(np.float32)


def stats(ts):
    return {"min": float(min(ts)), "median": float(np.median(ts))}


def main():
    flags = sys.argv[1:]
    n = int(flags[0]) if flags and not flags[0].startswith("--") else 512
    reps = int(flags[flags.index("--reps") + 1]) if "--reps" in flags else 7
    out_path = flags[flags.index("--out") + 1] if "--out" in flags else os.path.join(ROOT, "profiles", "r26_warp_run.json")
    from raytracedicom_amd import abi, engine, grids
    nf, spacing = n // 4, 2.0
    dims, fdims = (n, n, n), (nf, nf, nf)
    grid = (np.eye(3) * spacing, np.zeros(3))
    other = (np.eye(3) * spacing, np.array([0.6, -0.5, 0.25]))          # the source grid: the same spacing, shifted by a fraction of a voxel
    field_grid = (np.eye(3) * spacing * (n - 1) / (nf - 1), np.zeros(3))
    maps = grids.warp_maps(grid, other, field_grid)
    dvf = smooth_field(nf, spacing, 3.0)
    rng = np.random.default_rng(1)
    nbytes = 4 * n ** 3
    result = {"n": n, "field": nf, "reps": reps, "max_displacement_voxels": float(np.abs(dvf).max() / spacing)}
    with engine.Engine(0) as eng:
        hip = hip_runtime()
        stream = eng.stream()
        ev = [C.c_void_p(), C.c_void_p()]
        for e in ev:
            assert hip.hipEventCreate(C.byref(e)) == 0
        d_dvf, d_src, d_dst, d_other = (eng.device_alloc(b) for b in (dvf.nbytes, nbytes, nbytes, nbytes))
        nws = eng.warp_t_workspace_bytes(dims)
        d_ws = eng.device_alloc(nws)
        eng.to_device(d_dvf, dvf)
        eng.to_device(d_src, (rng.random((n, n, n), dtype=np.float32) * np.float32(70.0)).astype(np.float32))
        eng.device_zero(d_other, nbytes)
        warp = abi.make_warp(*maps, d_dvf, fdims)
        fw, rs, cp = [], [], []
        for i in range(reps + 1):
            eng.warp_dose_device(d_src, dims, warp, d_dst, dims)
            t_fw = eng.warp_kernel_ms()
            eng.resample_dose_device(d_src, dims, maps[0], d_dst, dims)
            t_rs = eng.resample_kernel_ms()
            assert hip.hipEventRecord(ev[0], stream) == 0
            assert hip.hipMemcpyAsync(d_dst, d_other, nbytes, 3, stream) == 0              # hipMemcpyDeviceToDevice
            assert hip.hipEventRecord(ev[1], stream) == 0 and hip.hipEventSynchronize(ev[1]) == 0
            ms = C.c_float(0)
            assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
            if i:
                fw.append(t_fw)
                rs.append(t_rs)
                cp.append(float(ms.value))
        result.update(forward_ms=stats(fw), resample_ms=stats(rs), copy_ms=stats(cp))
        # the transposed call: the gradient is the warped dose (d_dst after a forward call), pushed back into d_other
        eng.warp_dose_device(d_src, dims, warp, d_dst, dims)
        eng.sync()
        results = {}
        for name, plain in (("tile", False), ("plain", True)):
            os.environ.pop("RTD_WARP_T_PLAIN", None)
            if plain:
                os.environ["RTD_WARP_T_PLAIN"] = "1"                  # (read when the handle is made)
            with engine.Engine(0) as e2:
                os.environ.pop("RTD_WARP_T_PLAIN", None)
                rows = []
                for i in range(reps + 1):
                    e2.warp_dose_t_device(d_dst, dims, warp, d_other, dims, d_ws, nws)
                    t = e2.warp_t_kernel_ms()
                    if i:
                        rows.append(t)
                rows = np.array(rows)
                result["transposed_%s_ms" % name] = {k: stats(rows[:, j]) for j, k in enumerate(("memset", "maximum", "scatter", "finish"))}
                result["transposed_%s_ms" % name]["total"] = stats(rows.sum(axis=1))
                got = np.empty((n, n, n), dtype=np.float32)
                e2.to_host(got, d_other)
                results[name] = got
        result["plain_and_tile_bits_equal"] = bool((results["tile"].view(np.uint32) == results["plain"].view(np.uint32)).all())
        result["transposed_nonzero_share"] = float(np.count_nonzero(results["tile"]) / results["tile"].size)
        eng.sync()
        for p in (d_dvf, d_src, d_dst, d_other, d_ws):
            eng.device_free(p)
    med = lambda k: result[k]["median"]
    result["forward_over_resample"] = med("forward_ms") / med("resample_ms")
    result["forward_over_copy"] = med("forward_ms") / med("copy_ms")
    for name in ("tile", "plain"):
        result["transposed_%s_over_copy" % name] = result["transposed_%s_ms" % name]["total"]["median"] / med("copy_ms")
    result["scatter_plain_over_tile"] = result["transposed_plain_ms"]["scatter"]["median"] / result["transposed_tile_ms"]["scatter"]["median"]
    text = json.dumps(result, indent=1)
    print(text, flush=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
