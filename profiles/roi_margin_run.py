#!/usr/bin/env python3
"""Times the derived ROIs on a 512 x 512 x 300 grid at 1 x 1 x 2.5 mm:
  target_expand_5        an ellipsoidal target of 60 x 60 x 60 mm expanded by 5 mm;
  target_expand_7_3      the same by 7 mm with the +x and +z sides at 3 mm;
  body_contract_5        a body-sized ellipsoid (400 x 300 x 700 mm) contracted by 5 mm;
  body_expand_30         the same expanded by 30 mm;
  ring_5_20              expand(20) without expand(5) of the target: two margins and a combine;
  combine                the body without the target's 5 mm expansion;
  from_mask              the body from its byte mask.
Per case: kernel_ms, the hipEvents each call records around its own kernels (summed over the calls of the case); wall_ms, the wall
clock around the synchronous calls (tables, allocations, kernels, the wait for the total, the emit). One warm-up, then N timed runs:
median, min and max. Beside them the margins under RTD_ROI_MARGIN_NAIVE in a fresh child process (one warm-up and 3 runs, 1 run where
the warm-up took more than 5 s), and the SHA-256 of every voxel list compared between the two processes. Prints one JSON line.
Usage: python profiles/roi_margin_run.py [N]"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's HIP runtime initialises first, as in bench.py)

from raytracedicom_amd import engine  # noqa: E402

DIMS = (512, 512, 300)
SPACING = (1.0, 1.0, 2.5)


def ellipsoid(centre, semi_mm):
    """uint8 [Z][Y][X] on the device: voxel centres inside the ellipsoid (centre in voxels, semi-axes in mm)."""
    ax = [torch.arange(n, device="cuda", dtype=torch.float32) for n in DIMS]
    r = (((ax[0] - centre[0]) * SPACING[0] / semi_mm[0]) ** 2)[None, None, :] + (((ax[1] - centre[1]) * SPACING[1] / semi_mm[1]) ** 2)[None, :, None] \
        + (((ax[2] - centre[2]) * SPACING[2] / semi_mm[2]) ** 2)[:, None, None]
    return (r <= 1.0).to(torch.uint8).contiguous()


def spread(ms):
    ms = sorted(ms)
    return {"median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}


def ring(roi, inner, outer):
    a, b = roi.expand(outer, SPACING), roi.expand(inner, SPACING)
    out = a.subtract(b)
    ms = a.kernel_ms() + b.kernel_ms() + out.kernel_ms()
    a.close()
    b.close()
    return out, ms


def cases(eng, masks, margins_only):
    """name -> a function that runs the case once and returns (the result Roi, the kernel ms of its calls)."""
    target, body = eng.roi_from_mask(masks["target"]), eng.roi_from_mask(masks["body"])
    grown = target.expand(5.0, SPACING)

    def one(call):
        def run():
            r = call()
            return r, r.kernel_ms()
        return run
    out = {"target_expand_5": one(lambda: target.expand(5.0, SPACING)),
           "target_expand_7_3": one(lambda: target.expand((7.0, 3.0, 7.0, 7.0, 7.0, 3.0), SPACING)),
           "body_contract_5": one(lambda: body.contract(5.0, SPACING)),
           "body_expand_30": one(lambda: body.expand(30.0, SPACING)),
           "ring_5_20": lambda: ring(target, 5.0, 20.0)}
    if not margins_only:
        out["combine"] = one(lambda: body.subtract(grown))
        out["from_mask"] = one(lambda: eng.roi_from_mask(masks["body"]))
    return out, (target, body, grown)


def measure(n_runs, margins_only, adaptive):
    eng = engine.Engine(0)
    masks = {"target": ellipsoid((300.0, 200.0, 150.0), (30.0, 30.0, 30.0)), "body": ellipsoid((256.0, 256.0, 150.0), (200.0, 150.0, 350.0))}
    torch.cuda.synchronize()
    todo, keep = cases(eng, masks, margins_only)
    res = {}
    for name, run in todo.items():
        t0 = time.perf_counter()
        r, _ = run()                                                   # warm-up: the kernels loaded
        warm = 1e3 * (time.perf_counter() - t0)
        vox = r.voxels()
        info = r.info
        digest = hashlib.sha256(vox.tobytes()).hexdigest()
        r.close()
        n = 1 if adaptive and warm > 5000.0 else n_runs
        kern, wall = [], []
        for _ in range(n):
            t0 = time.perf_counter()
            r, ms = run()
            wall.append(1e3 * (time.perf_counter() - t0))
            kern.append(ms)
            r.close()
        res[name] = {"n_voxels": info["n_voxels"], "box_lo": info["box_lo"], "box_hi": info["box_hi"], "sha256": digest, "runs": n,
                     "kernel_ms": spread(kern), "wall_ms": spread(wall)}
        print("%s: kernel %s wall %s" % (name, res[name]["kernel_ms"], res[name]["wall_ms"]), file=sys.stderr, flush=True)
    for r in keep:
        r.close()
    eng.close()
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--child" in sys.argv:
        torch.cuda.init()
        json.dump(measure(3, True, True), open(args[0], "w"))
        return
    N = int(args[0]) if args else 7
    torch.cuda.init()
    out = {"what": "rtd_roi_margin / _combine / _from_mask; kernel_ms = hipEvents around the kernels of the calls, wall_ms = the whole calls",
           "N": N, "dims": list(DIMS), "spacing_mm": list(SPACING), "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
           "state": "one process on a shared machine, profiler off, clocks as found; the spread of the runs is given with every median"}
    out["separable"] = measure(N, False, False)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "naive.json")
        env = dict(os.environ, RTD_ROI_MARGIN_NAIVE="1")
        subprocess.run([sys.executable, os.path.abspath(__file__), path, "--child"], check=True, env=env, cwd=ROOT)
        out["naive"] = json.load(open(path))
    out["equal_lists"] = {k: v["sha256"] == out["separable"][k]["sha256"] for k, v in out["naive"].items()}
    out["naive_over_separable_kernel_ms"] = {k: round(v["kernel_ms"]["median"] / out["separable"][k]["kernel_ms"]["median"], 1) for k, v in out["naive"].items()}
    for part in ("separable", "naive"):
        for v in out[part].values():
            v["sha256"] = v["sha256"][:16]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
