#!/usr/bin/env python3
"""Times the variable-RBE path (rtd_rbe_dose, rtd_rbe_backward, an optimiser iteration with and without rtd_optimizer_set_rbe) with
hipEvents on the engine's stream, on the matrix of profiles/let_run.py: C3 (512^3 heterogeneous CT, 10x10 spots x 20 layers) with a
2 mm dose grid, ray_weight_cutoff = 0, threshold 0, luts.synth_let as the table, McNamara with two tissues. The two kernels on the
matrix's row box and on the whole grid; beside each a device-to-device copy that moves the same number of bytes (forward 9 read + 4
written per voxel, backward 13 + 8: a copy of half that many bytes reads and writes that many). The 2 mm grid is 128^3 and fits the
caches, so the same pair is timed once more on a synthetic 512^3 grid with three classes. The optimiser's objective is SQ_OVERDOSE on
the voxels of the row box.
Prints one JSON line.
Usage: python profiles/rbe_run.py [K]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's HIP runtime initialises first, as in bench.py)

from raytracedicom_amd import abi, engine, luts, rbe, scenarios  # noqa: E402
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
    f = eng.create_field(beam, dims)
    nnz_c = C.c_size_t(0)
    eng._check(engine.lib().rtd_field_dose_influence(eng._h, f._h, C.c_float(0.0), C.byref(nnz_c)))
    f.dose_influence_prepare()
    f.let_influence()
    _, info = f.finish()
    lo, hi = info["dose_box_min"], info["dose_box_max"]
    box_voxels = int(np.prod([max(hi[i] - lo[i] + 1, 0) for i in range(3)]))
    vols = [eng.device_alloc(4 * n) for _ in range(6)]
    dD, dN, dG, dR, dA, dB = vols
    dw = eng.device_alloc(4 * int(beam.spotWeights.size))
    eng.to_device(dw, np.ascontiguousarray(beam.spotWeights, dtype=np.float32))
    for p in vols:
        eng.device_zero(p, 4 * n)
    f.dose_influence_apply(dw, dD, init=True)
    f.let_apply(dw, dN, init=True)
    eng.to_device(dG, np.random.default_rng(1).random(n, dtype=np.float32) - np.float32(0.5))
    model = eng.create_rbe(dims, rbe.tissue("mcnamara", 0.5, 0.05))
    late = model.add_tissue(rbe.tissue("mcnamara", 0.1, 0.05))
    zz, yy, xx = np.meshgrid(np.arange(lo[2], hi[2] + 1), np.arange(lo[1], hi[1] + 1), np.arange(lo[0], hi[0] + 1), indexing="ij")
    box_idx = ((zz * dims[1] + yy) * dims[0] + xx).reshape(-1).astype(np.int32)
    model.assign(box_idx[::3], late)                                   # (lanes of a wave differ in class)
    tm = Timer(hip, eng.stream())
    stream = C.c_void_p(eng.stream())
    out = {"what": "variable-RBE path on the C3 2 mm matrix; hipEvents on the engine's stream, median / min / max ms over `steps` calls after 3 "
                   "warm-up calls. copy_*: a device-to-device copy that moves the same number of bytes as the kernel beside it (half of them "
                   "read, half written). optimizer_*: one rtd_optimizer_run iteration, SQ_OVERDOSE on the voxels of the row box",
           "case": "C3 2mm dose grid", "dose_dims": list(dims), "nnz": int(nnz_c.value), "dose_box_voxels": box_voxels, "grid_voxels": n, "steps": steps}
    for name, box, nv in (("box", (lo, hi), box_voxels), ("grid", None, n)):
        fwd = tm.ms(lambda: model.dose(dD, dN, dR, box=box), steps)
        bwd = tm.ms(lambda: model.backward(dD, dN, dG, dA, dB, box=box), steps)
        res = {"voxels": nv, "rbe_dose_ms": fwd, "rbe_backward_ms": bwd}
        for kname, per_voxel, t in (("rbe_dose", 13, fwd), ("rbe_backward", 21, bwd)):
            half = max(per_voxel * nv // 2, 4)
            src, dst = eng.device_alloc(half), eng.device_alloc(half)
            eng.device_zero(src, half)
            cp = tm.ms(lambda: hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(half), HIP_MEMCPY_DEVICE_TO_DEVICE, stream), steps)
            eng.device_free(src)
            eng.device_free(dst)
            res["copy_%s_ms" % kname] = cp
            res["%s_bytes" % kname] = per_voxel * nv
            res["%s_over_copy" % kname] = round(t["median"] / cp["median"], 3)
        out[name] = res
    # the same two kernels where the volumes no longer fit a cache: a synthetic 512^3 grid (no field), three classes
    big_dims = (512, 512, 512)
    nb = 512 ** 3
    gen = torch.Generator(device="cuda").manual_seed(3)
    td = 80.0 * torch.rand(nb, device="cuda", generator=gen)
    tn = td * 20.0 * torch.rand(nb, device="cuda", generator=gen)
    tg = torch.rand(nb, device="cuda", generator=gen) - 0.5
    tr, ta, tb = (torch.zeros(nb, device="cuda") for _ in range(3))
    big = eng.create_rbe(big_dims, rbe.tissue("mcnamara", 0.5, 0.05))
    for t, step in ((rbe.tissue("carabe", 0.1, 0.05), 3), (rbe.tissue("wedenberg", 0.15, 0.05), 7)):
        big.assign(np.arange(0, nb, step, dtype=np.int32), big.add_tissue(t))
    torch.cuda.synchronize()
    fwd = tm.ms(lambda: big.dose(td.data_ptr(), tn.data_ptr(), tr.data_ptr()), steps)
    bwd = tm.ms(lambda: big.backward(td.data_ptr(), tn.data_ptr(), tg.data_ptr(), ta.data_ptr(), tb.data_ptr()), steps)
    res = {"voxels": nb, "rbe_dose_ms": fwd, "rbe_backward_ms": bwd}
    del tg, ta, tb
    for kname, per_voxel, t in (("rbe_dose", 13, fwd), ("rbe_backward", 21, bwd)):
        half = per_voxel * nb // 2
        src, dst = eng.device_alloc(half), eng.device_alloc(half)
        eng.device_zero(src, half)
        cp = tm.ms(lambda: hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(half), HIP_MEMCPY_DEVICE_TO_DEVICE, stream), steps)
        eng.device_free(src)
        eng.device_free(dst)
        res["copy_%s_ms" % kname] = cp
        res["%s_bytes" % kname] = per_voxel * nb
        res["%s_over_copy" % kname] = round(t["median"] / cp["median"], 3)
        res["%s_tb_per_s" % kname] = round(per_voxel * nb / (t["median"] * 1e-3) / 1e12, 3)
    out["synthetic_512"] = res
    big.destroy()
    del td, tn, tr
    obj = eng.create_objective(dims)
    obj.add_roi(np.sort(box_idx))
    obj.add_term(abi.RTD_OBJ_SQ_OVERDOSE, 0, 1.0, 0.0)
    plain, with_model = eng.create_optimizer([f], obj), eng.create_optimizer([f], obj)
    with_model.set_rbe(model)
    eng.sync()
    out["optimizer_iteration_ms"] = tm.ms(lambda: plain.run(1), steps)
    out["optimizer_iteration_rbe_ms"] = tm.ms(lambda: with_model.run(1), steps)
    out["optimizer_iteration_again_ms"] = tm.ms(lambda: plain.run(1), steps)    # the run-to-run spread of the same call
    tm.close()
    for o in (plain, with_model):
        o.destroy()
    obj.destroy()
    model.destroy()
    f.destroy()
    for p in vols + [dw]:
        eng.device_free(p)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
