#!/usr/bin/env python3
"""Times the products with the compact dose-influence matrix (rtd_field_dose_influence_compact / _apply_compact / _apply_t_compact)
beside the plain ones (rtd_field_dose_influence_apply / _apply_t) in one process, on C3 (512^3 heterogeneous CT, 10x10 spots x 20
layers) with the 2 mm dose grid and, if the device has the memory free, on its native grid; inputs resident, ray_weight_cutoff = 0,
threshold 0. hipEvents on the engine's stream, the median of `steps` calls after 3 warm-up calls, as profiles/dij_apply_run.py.
Per case: the plain pair; for every forward tree (G lanes per row, E entries per lane and trip) the build's time on the host clock, the
bytes both forms keep, and the compact pair; then, at the default tree and on the 2 mm case, an iteration of
rtd_optimizer_create_compact beside rtd_optimizer_create and the objective of each after K iterations from the same start (the
objective of profiles/lbfgs_run.py), and the device memory in use before and after release_plain.
Prints one JSON line. Usage: python profiles/dij_compact_run.py [steps] [K] [--no-native]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's HIP runtime initialises first, as in bench.py)

import optimizer_reference as R  # noqa: E402
from raytracedicom_amd import abi, engine, luts, scenarios  # noqa: E402
from profiles.dij_apply_run import Timer  # noqa: E402
from profiles.dij_run import _two_mm  # noqa: E402
from profiles.gradient_run import _hip  # noqa: E402
from profiles.optimizer_run import _event_ms  # noqa: E402

TREES = ((16, 1), (16, 2), (16, 4), (32, 1), (32, 2), (32, 4))
DEFAULT = (16, 4)
NATIVE_BYTES_NEEDED = 150e9      # the plain form's 120 GB estimate of profiles/dij_apply_run.py plus the compact form beside it


def run(name, scn, beam, dims, steps, K, hip, optimise):
    torch.cuda.synchronize()
    eng = engine.Engine(0)
    opt = abi.default_options()
    opt.ray_weight_cutoff = 0.0
    eng.set_options(opt)
    eng.set_luts(scn.luts)
    eng.set_ct(scn.ct)
    nvox = dims[0] * dims[1] * dims[2]
    n_spots = int(beam.spotWeights.size)
    d, dg = eng.device_alloc(4 * nvox), eng.device_alloc(4 * nvox)
    dw, dout = eng.device_alloc(4 * n_spots), eng.device_alloc(4 * n_spots)
    rng = np.random.default_rng(1)
    eng.to_device(dg, rng.random((dims[2], dims[1], dims[0]), dtype=np.float32) - np.float32(0.5))
    eng.to_device(dw, np.ascontiguousarray(beam.spotWeights, dtype=np.float32))
    eng.device_zero(d, 4 * nvox)
    f = eng.create_field(beam, dims)
    nnz_c = C.c_size_t(0)
    t0 = time.perf_counter()
    eng._check(engine.lib().rtd_field_dose_influence(eng._h, f._h, C.c_float(0.0), C.byref(nnz_c)))
    matrix_s = time.perf_counter() - t0
    f.dose_influence_prepare()
    tm = Timer(hip, eng.stream())
    out = {"case": name, "dose_dims": list(dims), "spots": n_spots, "nnz": int(nnz_c.value), "matrix_s_host_clock": round(matrix_s, 3), "steps": steps}
    out["plain_apply_ms"] = tm.ms(lambda: f.dose_influence_apply(dw, d, init=True), steps)
    out["plain_apply_t_ms"] = tm.ms(lambda: f.dose_influence_apply_t(dg, dout), steps)
    trees = []
    for G, E in TREES + (DEFAULT,):                                  # (the default last: it is the form that stays)
        os.environ["RTD_DIJC_LANES"], os.environ["RTD_DIJC_PER"] = str(G), str(E)
        t0 = time.perf_counter()
        f.dose_influence_compact()
        build_ms = 1e3 * (time.perf_counter() - t0)
        info = f.dose_influence_compact_info()
        trees.append({"lanes_per_row": G, "entries_per_lane": E, "build_ms_host_clock": round(build_ms, 2), "row_bits": info["row_bits"],
                      "row_entries": info["row_entries"], "compact_bytes": info["compact_bytes"], "plain_bytes": info["plain_bytes"],
                      "apply_ms": tm.ms(lambda: f.dose_influence_apply_compact(dw, d, init=True), steps),
                      "apply_t_ms": tm.ms(lambda: f.dose_influence_apply_t_compact(dg, dout), steps)})
    del os.environ["RTD_DIJC_LANES"], os.environ["RTD_DIJC_PER"]
    out["trees"] = trees[:-1]
    out["default_tree"] = trees[-1]
    out["plain_apply_ms_again"] = tm.ms(lambda: f.dose_influence_apply(dw, d, init=True), steps)   # (the plain twin's own run-to-run spread)
    out["plain_apply_t_ms_again"] = tm.ms(lambda: f.dose_influence_apply_t(dg, dout), steps)
    if optimise:
        _, info = f.finish()
        lo, hi = info["dose_box_min"], info["dose_box_max"]
        f.dose_influence_apply(dw, d, init=True)
        dose0 = np.empty((dims[2], dims[1], dims[0]), dtype=np.float32)
        eng.to_host(dose0, d)
        z, y, x = np.meshgrid(*[np.arange(k) for k in dose0.shape], indexing="ij")
        tot = float(dose0.sum(dtype=np.float64))
        c = [float((dose0 * a).sum(dtype=np.float64)) / tot for a in (z, y, x)]
        sphere = (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= 6.0 ** 2
        box = np.zeros(dose0.shape, dtype=bool)
        box[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
        level = float(dose0[sphere].mean())
        obj = eng.create_objective(dims)
        obj.add_term(R.SQ_DEVIATION, obj.add_roi(sphere.reshape(-1)), 1.0, level)
        obj.add_term(R.SQ_OVERDOSE, obj.add_roi((box & ~sphere).reshape(-1)), 1.0, 0.3 * level)

        def timed(make):
            warm = make()
            warm.run(3)
            eng.sync()
            warm.destroy()
            op = make()
            op.run(0)
            eng.sync()
            ms = _event_ms(hip, eng.stream(), lambda: op.run(K)) / K
            rep, hist = op.result()
            op.destroy()
            return ms, rep, hist
        pm, prep, phist = timed(lambda: eng.create_optimizer([f], obj))
        cm, crep, chist = timed(lambda: eng.create_compact_optimizer([f], obj))
        out["optimizer"] = {"K": K, "plain_ms_per_iteration": round(pm, 4), "compact_ms_per_iteration": round(cm, 4),
                            "f_first": [float(phist[0]), float(chist[0])], "plain_f_last": prep["f_last"], "compact_f_last": crep["f_last"],
                            "plain_f_best": prep["f_best"], "compact_f_best": crep["f_best"]}
        obj.destroy()
    eng.sync()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    f.dose_influence_compact(release_plain=True)
    eng.sync()
    info = f.dose_influence_compact_info()
    out["release_plain"] = {"device_bytes_freed": int(torch.cuda.mem_get_info()[0] - free0), "released_bytes": info["released_bytes"],
                            "compact_bytes": info["compact_bytes"],
                            "apply_ms": tm.ms(lambda: f.dose_influence_apply_compact(dw, d, init=True), steps),
                            "apply_t_ms": tm.ms(lambda: f.dose_influence_apply_t_compact(dg, dout), steps)}
    tm.close()
    f.destroy()
    for p in (d, dg, dw, dout):
        eng.device_free(p)
    eng.close()
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    steps = int(args[0]) if args else 20
    K = int(args[1]) if len(args) > 1 else 200
    torch.cuda.init()
    hip = _hip()
    es = luts.synth_luts()
    c3 = scenarios.hetero_ct(es, n=512, n_fields=1)
    b2, dims2 = _two_mm(c3.beams[0], 512)
    res = [run("C3 2mm dose grid", c3, b2, dims2, steps, K, hip, optimise=True)]
    free, total = torch.cuda.mem_get_info()
    native = {"case": "C3 native grid", "device_bytes_free": int(free), "device_bytes_total": int(total), "bytes_wanted": int(NATIVE_BYTES_NEEDED)}
    if "--no-native" in sys.argv:
        native["status"] = "not run: switched off"
    elif free < NATIVE_BYTES_NEEDED:
        native["status"] = "not run: memory"
    else:
        native.update(run("C3 native grid", c3, c3.beams[0], c3.dims, steps, K, hip, optimise=False))
        native["status"] = "run"
    res.append(native)
    print(json.dumps({"what": "products with the compact dose-influence matrix beside the plain ones; hipEvents on the engine's stream, median / min / "
                              "max ms over `steps` calls after 3 warm-up calls; build times on the host clock",
                      "dij_compact": res}))


if __name__ == "__main__":
    main()
