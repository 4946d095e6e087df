#!/usr/bin/env python3
"""Times the LET path (rtd_field_water_depth, the two value passes of rtd_field_let_influence, rtd_field_let_influence_apply /
_apply_t) with hipEvents on the engine's stream, on the matrix of profiles/r22_dij_run_new.json's first case: C3 (512^3
heterogeneous CT, 10x10 spots x 20 layers) with a 2 mm dose grid, ray_weight_cutoff = 0, threshold 0, luts.synth_let as the table.
In the same process: apply / apply_t with the dose values (the same kernels on an array of the same size), and a device-to-device
copy that moves the bytes a value pass must move (per entry 8 read + 4 written for each of the CSC pass and the row-major pass, plus
the depth box: a copy of half that many bytes reads and writes that many).
Prints one JSON line; with rocprofv3 --kernel-trace --stats in front, the per-kernel split (k_let_depth, k_let_values_csc,
k_let_values_rows).
Usage: python profiles/let_run.py [K]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's HIP runtime initialises first, as in bench.py)

from raytracedicom_amd import abi, engine, luts, scenarios  # noqa: E402
from profiles.dij_apply_run import Timer  # noqa: E402
from profiles.dij_run import _two_mm  # noqa: E402
from profiles.gradient_run import _hip  # noqa: E402

HIP_MEMCPY_DEVICE_TO_DEVICE = 3


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    steps = int(args[0]) if args else 20
    torch.cuda.init()
    hip = _hip()
    es = luts.synth_luts()
    c3 = scenarios.hetero_ct(es, n=512, n_fields=1)
    beam, dims = _two_mm(c3.beams[0], 512)
    torch.cuda.synchronize()
    eng = engine.Engine(0)
    opt = abi.default_options()
    opt.ray_weight_cutoff = 0.0
    eng.set_options(opt)
    eng.set_luts(es)
    eng.set_ct(c3.ct)
    eng.set_let_table(luts.synth_let(es))
    n = dims[0] * dims[1] * dims[2]
    n_spots = int(beam.spotWeights.size)
    d, dg = eng.device_alloc(4 * n), eng.device_alloc(4 * n)
    dw, dout = eng.device_alloc(4 * n_spots), eng.device_alloc(4 * n_spots)
    rng = np.random.default_rng(1)
    eng.to_device(dg, rng.random((dims[2], dims[1], dims[0]), dtype=np.float32) - np.float32(0.5))
    eng.to_device(dw, np.ascontiguousarray(beam.spotWeights, dtype=np.float32))
    eng.device_zero(d, 4 * n)
    f = eng.create_field(beam, dims)
    nnz_c = C.c_size_t(0)
    eng._check(engine.lib().rtd_field_dose_influence(eng._h, f._h, C.c_float(0.0), C.byref(nnz_c)))
    nnz = int(nnz_c.value)
    f.dose_influence_prepare()
    _, info = f.finish()
    lo, hi = info["dose_box_min"], info["dose_box_max"]
    box_voxels = int(np.prod([max(hi[i] - lo[i] + 1, 0) for i in range(3)]))
    tm = Timer(hip, eng.stream())
    f.let_influence()                                                 # (allocates its three buffers: launches only from here on)
    eng.sync()
    depth = tm.ms(lambda: f.water_depth(d), steps)
    influence = tm.ms(f.let_influence, steps)                         # depth over the row box + the two value passes
    pass_bytes = 2 * 12 * nnz + 4 * box_voxels                        # what the three launches of let_influence must move
    half = pass_bytes // 2
    src, dst = eng.device_alloc(half), eng.device_alloc(half)
    eng.device_zero(src, half)
    stream = C.c_void_p(eng.stream())
    copy = tm.ms(lambda: hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(half), HIP_MEMCPY_DEVICE_TO_DEVICE, stream), steps)
    eng.device_free(src)
    eng.device_free(dst)
    eng.device_zero(d, 4 * n)
    apply = tm.ms(lambda: f.dose_influence_apply(dw, d, init=True), steps)
    let_apply = tm.ms(lambda: f.let_apply(dw, d, init=True), steps)
    apply_t = tm.ms(lambda: f.dose_influence_apply_t(dg, dout), steps)
    let_apply_t = tm.ms(lambda: f.let_apply_t(dg, dout), steps)
    apply_again = tm.ms(lambda: f.dose_influence_apply(dw, d, init=True), steps)      # the run-to-run spread of the same call
    apply_t_again = tm.ms(lambda: f.dose_influence_apply_t(dg, dout), steps)
    out = {"what": "LET path on the C3 2 mm matrix; hipEvents on the engine's stream, median / min / max ms over `steps` calls after 3 warm-up "
                   "calls. let_influence = k_let_depth over the row box + k_let_values_csc + k_let_values_rows (rocprofv3 --kernel-trace --stats "
                   "splits them); device_copy moves the same number of bytes (half of them read, half written)",
           "case": "C3 2mm dose grid", "dose_dims": list(dims), "spots": n_spots, "nnz": nnz, "dose_box_voxels": box_voxels,
           "let_influence_bytes": int(pass_bytes), "water_depth_ms": depth, "let_influence_ms": influence, "device_copy_ms": copy,
           "let_influence_over_copy": round(influence["median"] / copy["median"], 3),
           "apply_ms": apply, "let_apply_ms": let_apply, "apply_again_ms": apply_again,
           "apply_t_ms": apply_t, "let_apply_t_ms": let_apply_t, "apply_t_again_ms": apply_t_again, "steps": steps}
    tm.close()
    f.destroy()
    for p in (d, dg, dw, dout):
        eng.device_free(p)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
