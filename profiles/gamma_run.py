#!/usr/bin/env python3
"""Times the gamma index on the device (rtd_dose_gamma) on an n^3 grid at 1 mm: the Gaussian blob of tests/gamma_scenes.py scaled with
the grid (sigma 0.1875 n mm, so about a quarter of the voxels lie above the 10 % threshold) against a copy with 2 % multiplicative
noise. Per configuration (dd / dta, samples per grid step) one JSON line:
  brick_ms   rtd_dose_gamma_kernel_ms of k_gamma_search: the smallest and the median of the repeats after one warm-up call;
  naive_ms   the same of k_gamma_naive, from a child process started with RTD_GAMMA_NAIVE=1 (the switch is read by rtd_create);
  oracle_s   wall clock of the CPU oracle's search with the machine's threads (interp = 1 only; --no-oracle leaves it out);
  gsamples_per_s   n_evaluated (2 k r + 1)^3 samples of the definition over brick_ms: samples the pruning skips count as done.
The counts of the two kernels (and of the oracle) are compared and a difference is an error. Every GPU step runs under the time limit
of the command that starts this script.
--scale S multiplies the evaluated dose by S: with S = 3 every voxel fails by so much that no sample can be pruned, and gsamples_per_s
is the rate at which samples are really visited.
Usage: python profiles/gamma_run.py N [--no-oracle] [--reps R] [--only dd:dta:interp] [--scale S]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

CONFIGS = ((0.01, 1.0, 1), (0.01, 1.0, 2), (0.03, 3.0, 1), (0.03, 3.0, 2))


SCALE = 1.0     # --scale S: the evaluated dose is S times the noisy copy (S = 3: no sample can be pruned, every voxel fails)


def pair(n, amp=0.02, seed=7):
    x = np.arange(n, dtype=np.float32)
    gx = np.exp(-((x - 0.45 * n) ** 2) / (2 * (0.1875 * n) ** 2))
    gy = np.exp(-((x - 0.55 * n) ** 2) / (2 * (0.1875 * n) ** 2))
    gz = np.exp(-((x - 0.50 * n) ** 2) / (2 * (0.1875 * n) ** 2))
    ref = (2.0 * gz[:, None, None] * gy[None, :, None] * gx[None, None, :]).astype(np.float32)
    rng = np.random.default_rng(seed)
    ev = ref * (1 + amp * rng.standard_normal(ref.shape, dtype=np.float32))
    return ref, (np.float32(SCALE) * ev).astype(np.float32)


def time_configs(n, configs, reps):
    """-> {config: (ms per repeat, n_evaluated, n_passed, bits of max_gamma)} with this process' handle."""
    from raytracedicom_amd import abi, engine
    ref, ev = pair(n)
    out = {}
    with engine.Engine(0) as eng:
        d_ref, d_ev, d_res = eng.device_alloc(ref.nbytes), eng.device_alloc(ev.nbytes), eng.device_alloc(32)
        eng.to_device(d_ref, ref)
        eng.to_device(d_ev, ev)
        for dd, dta, k in configs:
            ms = []
            for i in range(reps + 1):
                eng.gamma_device(d_ref, d_ev, (n, n, n), (1.0, 1.0, 1.0), d_res, dd=dd, dta=dta, interp=k)
                t = eng.gamma_kernel_ms()
                if i:
                    ms.append(t)
            raw = np.empty(32, dtype=np.uint8)
            eng.to_host(raw, d_res)
            res = abi.RtdGammaResult.from_buffer_copy(raw.tobytes())
            out["%g:%g:%d" % (dd, dta, k)] = (ms, int(res.n_evaluated), int(res.n_passed), int(np.float32(res.max_gamma).view(np.uint32)))
        for p in (d_ref, d_ev, d_res):
            eng.device_free(p)
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    flags = sys.argv[1:]
    n = int(args[0])
    reps = int(flags[flags.index("--reps") + 1]) if "--reps" in flags else 3
    global SCALE
    if "--scale" in flags:
        SCALE = float(flags[flags.index("--scale") + 1])
    configs = CONFIGS
    if "--only" in flags:
        dd, dta, k = flags[flags.index("--only") + 1].split(":")
        configs = ((float(dd), float(dta), int(k)),)
    if "--child" in flags:                                            # the RTD_GAMMA_NAIVE leg: the timings as one JSON line
        print(json.dumps(time_configs(n, configs, reps)))
        return
    brick = time_configs(n, configs, reps)
    child_args = [sys.executable, os.path.abspath(__file__), str(n), "--child", "--reps", str(max(1, reps - 1))]
    for f in ("--only", "--scale"):
        if f in flags:
            child_args += [f, flags[flags.index(f) + 1]]
    p = subprocess.run(child_args, capture_output=True, text=True, env=dict(os.environ, RTD_GAMMA_NAIVE="1"))
    if p.returncode != 0:
        sys.exit("the RTD_GAMMA_NAIVE leg failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    naive = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    ref = ev = None
    for dd, dta, k in configs:
        key = "%g:%g:%d" % (dd, dta, k)
        ms, n_eval, n_pass, gbits = brick[key]
        nms, *ncounts = naive[key]
        if [n_eval, n_pass, gbits] != ncounts:
            sys.exit("%s: the brick kernel and the naive kernel differ: %r vs %r" % (key, (n_eval, n_pass, gbits), ncounts))
        r = int(np.ceil(np.float32(1.5) * np.float32(dta)))
        row = {"n": n, "scale": SCALE, "dd": dd, "dta_mm": dta, "radius": r, "interp": k, "n_evaluated": n_eval, "pass_rate": n_pass / max(n_eval, 1),
               "brick_ms_min": min(ms), "brick_ms_median": float(np.median(ms)), "naive_ms_min": min(nms), "naive_ms_median": float(np.median(nms)),
               "gsamples_per_s": n_eval * (2 * k * r + 1) ** 3 / (min(ms) * 1e-3) / 1e9}
        if k == 1 and "--no-oracle" not in flags:
            from oracle import oracle
            if ref is None:
                ref, ev = pair(n)
            t0 = time.perf_counter()
            rate, on, og = oracle.gamma_pass_rate(ref, ev, (1.0, 1.0, 1.0), dd, dta, 0.10)
            row["oracle_s"] = time.perf_counter() - t0
            row["oracle_threads"] = oracle.max_threads()
            if (on, round(rate * on), int(np.float32(og).view(np.uint32))) != (n_eval, n_pass, gbits):
                sys.exit("%s: the engine and the oracle differ: %r vs %r" % (key, (n_eval, n_pass, gbits), (on, rate, og)))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
