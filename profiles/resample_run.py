#!/usr/bin/env python3
"""Times dose resampling on the device (rtd_dose_resample) onto an n^3 destination (default 512) and, beside each case, a
device-to-device copy of the destination's bytes on the same stream between two events: the copy is the yardstick, because it is not
code under test and a resampling that writes every destination voxel once cannot be faster than moving those bytes.
  shift     n^3 -> n^3 at a half-voxel shift on every axis (every voxel blends 8 nodes);
  up3       (n/3)^3 at 3 mm -> n^3 at 1 mm, float32 source;
  up3_u16   the same from the uint16 pixels of an RT Dose file (src_scale);
  rot17     n^3 -> n^3 turned by 17 degrees about z through the centre (rows of the destination cross rows of the source).
Per case one JSON line: resample_ms (rtd_dose_resample_kernel_ms) and copy_ms, each the smallest and the median of the repeats after
one warm-up call, their ratio (median over median), and the destination bytes per second of the resampling.
Usage: python profiles/resample_run.py [N] [--reps R]"""
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


def cases(n):
    third = n // 3
    a = np.deg2rad(17.0)
    rot = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    c = np.full(3, (n - 1) / 2.0)
    return (("shift", n, np.float32, np.eye(3), np.full(3, 0.5)),
            ("up3", third, np.float32, np.eye(3) / 3.0, np.array([0.1, 0.2, 0.3])),
            ("up3_u16", third, np.uint16, np.eye(3) / 3.0, np.array([0.1, 0.2, 0.3])),
            ("rot17", n, np.float32, rot, c - rot @ c))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    flags = sys.argv[1:]
    n = int(args[0]) if args else 512
    reps = int(flags[flags.index("--reps") + 1]) if "--reps" in flags else 7
    from raytracedicom_amd import engine
    rng = np.random.default_rng(1)
    with engine.Engine(0) as eng:
        hip = hip_runtime()
        stream = eng.stream()
        ev = [C.c_void_p(), C.c_void_p()]
        for e in ev:
            assert hip.hipEventCreate(C.byref(e)) == 0
        dst_bytes = 4 * n ** 3
        d_dst, d_other = eng.device_alloc(dst_bytes), eng.device_alloc(dst_bytes)
        eng.device_zero(d_other, dst_bytes)
        for name, sn, dtype, m, v in cases(n):
            src = (rng.random((sn, sn, sn), dtype=np.float32) * np.float32(70.0)).astype(np.float32)
            kw = {}
            if dtype == np.uint16:
                src, kw = np.rint(src * (65535 / 70.0)).astype(np.uint16), dict(src_type=1, src_scale=70.0 / 65535)
            d_src = eng.device_alloc(src.nbytes)
            eng.to_device(d_src, src)
            rs, cp = [], []
            for i in range(reps + 1):
                eng.resample_dose_device(d_src, (sn, sn, sn), (m, v), d_dst, (n, n, n), **kw)
                t = eng.resample_kernel_ms()
                assert hip.hipEventRecord(ev[0], stream) == 0
                assert hip.hipMemcpyAsync(d_dst, d_other, dst_bytes, 3, stream) == 0          # hipMemcpyDeviceToDevice
                assert hip.hipEventRecord(ev[1], stream) == 0 and hip.hipEventSynchronize(ev[1]) == 0
                ms = C.c_float(0)
                assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
                if i:
                    rs.append(t)
                    cp.append(float(ms.value))
            eng.sync()
            eng.device_free(d_src)
            row = {"case": name, "src": [sn] * 3, "dst": [n] * 3, "src_type": np.dtype(dtype).name, "reps": reps,
                   "resample_ms_min": min(rs), "resample_ms_median": float(np.median(rs)), "copy_ms_min": min(cp), "copy_ms_median": float(np.median(cp)),
                   "ratio_to_copy": float(np.median(rs) / np.median(cp)), "dst_gb_per_s": dst_bytes / (float(np.median(rs)) * 1e-3) / 1e9}
            print(json.dumps(row), flush=True)
        eng.device_free(d_dst)
        eng.device_free(d_other)


if __name__ == "__main__":
    main()
