#!/usr/bin/env python3
"""Times a plan set (rtd_planset_run) on C3 (512^3 heterogeneous CT, 10x10 spots x 20 layers) with the 2 mm dose grid and the objective
of profiles/optimizer_run.py: a spherical target at the centre of the spot pattern's dose (SQ_DEVIATION) and the rest of the field's
dose box as SQ_OVERDOSE. For P = 1, 2, 4, 8, 16 plans (plan p: the overdose weight times 2^p), hipEvents on the engine's stream:
  set        run(K) / K of the set, three repeats;
  products   apply_set + apply_t_set of the same field at the set's stride, three repeats (what an iteration cannot be cheaper than);
and once, in the same process, the plain optimiser's run(K) / K and apply + apply_t (three repeats each): P times the plain
iteration is what P separate runs cost.
Prints one JSON line; with rocprofv3 --kernel-trace --stats in front, the per-kernel split of the iteration.
With --summary PARENT.jsonl NEW.jsonl PLANSET.json (lines of profiles/optimizer_run.py from the parent commit's build and from this
one, and a line of this script) it runs nothing: it prints the record that sets the set's figures against P times the parent's plain
iteration, with every ratio, margin and spread.
Usage: python profiles/planset_run.py [K] | --summary PARENT.jsonl NEW.jsonl PLANSET.json"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's HIP runtime initialises first, as in bench.py)

import optimizer_reference as R  # noqa: E402
from raytracedicom_amd import abi, engine, luts, scenarios  # noqa: E402
from profiles.dij_run import _two_mm  # noqa: E402
from profiles.gradient_run import _hip  # noqa: E402
from profiles.optimizer_run import _event_ms  # noqa: E402

PLANS = (1, 2, 4, 8, 16)
REPEATS = 3


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    K = int(args[0]) if args else 100
    torch.cuda.init()
    hip = _hip()
    es = luts.synth_luts()
    c3 = scenarios.hetero_ct(es, n=512, n_fields=1)
    beam, dims = _two_mm(c3.beams[0], 512)
    nvox, n = int(np.prod(dims)), int(np.prod(beam.spotWeights.shape))
    eng = engine.Engine(0)
    opt = abi.default_options()
    opt.ray_weight_cutoff = 0.0
    eng.set_options(opt)
    eng.set_luts(c3.luts)
    eng.set_ct(c3.ct)
    f = eng.create_field(beam, dims)
    nnz_c = C.c_size_t(0)
    eng._check(engine.lib().rtd_field_dose_influence(eng._h, f._h, C.c_float(0.0), C.byref(nnz_c)))
    f.dose_influence_prepare()
    _, info = f.finish()
    lo, hi = info["dose_box_min"], info["dose_box_max"]
    S = max(PLANS)
    dD, dG = eng.device_alloc(4 * nvox * S), eng.device_alloc(4 * nvox * S)
    dW, dGrad = eng.device_alloc(4 * n * S), eng.device_alloc(4 * n * S)
    for p, size in ((dD, nvox), (dG, nvox), (dGrad, n)):
        eng.device_zero(p, 4 * size * S)
    w0 = np.ascontiguousarray(beam.spotWeights, dtype=np.float32)
    eng.to_device(dW, w0)
    f.dose_influence_apply(dW, dD, init=True)
    dose0 = np.empty((dims[2], dims[1], dims[0]), dtype=np.float32)
    eng.to_host(dose0, dD)
    z, y, x = np.meshgrid(*[np.arange(d) for d in dose0.shape], indexing="ij")
    tot = float(dose0.sum(dtype=np.float64))
    c = [float((dose0 * a).sum(dtype=np.float64)) / tot for a in (z, y, x)]
    sphere = (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= 6.0 ** 2
    box = np.zeros(dose0.shape, dtype=bool)
    box[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    rest = box & ~sphere
    level = float(dose0[sphere].mean())
    terms = [(R.SQ_DEVIATION, 0, 1.0, level), (R.SQ_OVERDOSE, 1, 1.0, 0.3 * level)]
    obj = eng.create_objective(dims)
    obj.add_roi(sphere.reshape(-1))
    obj.add_roi(rest.reshape(-1))
    for t in terms:
        obj.add_term(*t)
    stream = eng.stream()
    # the plain optimiser and the plain products, in this process
    op = eng.create_optimizer([f], obj)
    op.run(3)
    eng.sync()
    plain_ms = [round(_event_ms(hip, stream, lambda: op.run(K)) / K, 4) for _ in range(REPEATS)]

    def pair():
        for _ in range(K):
            f.dose_influence_apply(dW, dD, init=True)
            f.dose_influence_apply_t(dG, dGrad)
    plain_pair_ms = [round(_event_ms(hip, stream, pair) / K, 4) for _ in range(REPEATS)]
    op.destroy()
    rows = []
    for P in PLANS:
        variants = [[terms[0], (terms[1][0], terms[1][1], terms[1][2] * 2.0 ** p, terms[1][3])] for p in range(P)]
        ps = eng.create_planset([f], obj, variants)
        ps.run(3)                                                     # warm-up: every kernel loaded
        eng.sync()
        set_ms = [round(_event_ms(hip, stream, lambda: ps.run(K)) / K, 4) for _ in range(REPEATS)]
        rep, hist = ps.result(P - 1)
        eng.device_zero(dG, 4 * nvox * S)

        def pair_set():
            for _ in range(K):
                f.dose_influence_apply_set(dW, dD, P, P, init=True)
                f.dose_influence_apply_t_set(dG, dGrad, P, P)
        eng.to_device(dW, np.repeat(w0.reshape(-1), P))               # (plan-minor: every plan the field's own weights)
        pair_set()                                                    # (warm-up, and the handle's scratch at this stride)
        eng.sync()
        pair_ms = [round(_event_ms(hip, stream, pair_set) / K, 4) for _ in range(REPEATS)]
        ps.destroy()
        rows.append({"plans": P, "set_ms_per_iteration": set_ms, "apply_set_plus_apply_t_set_ms": pair_ms,
                     "plans_times_plain_ms": round(P * min(plain_ms), 4), "set_over_plans_times_plain": round(min(set_ms) / (P * min(plain_ms)), 4),
                     "ms_per_plan": round(min(set_ms) / P, 4), "iterations": rep["iterations"], "guarded": rep["guarded"], "f_best_last_plan": rep["f_best"]})
    out = {"what": "plan set on C3, 2 mm dose grid: hipEvents around run(K) / K of the set and around K x (apply_set + apply_t_set) / K, per number "
                   "of plans, three repeats each; beside the plain optimiser's run(K) / K and K x (apply + apply_t) / K in the same process",
           "K": K, "spots": n, "nnz": int(nnz_c.value), "dose_dims": list(dims), "target_voxels": int(sphere.sum()), "overdose_voxels": int(rest.sum()),
           "plain_resident_ms_per_iteration": plain_ms, "plain_apply_plus_apply_t_ms": plain_pair_ms, "sets": rows}
    obj.destroy()
    f.destroy()
    for p in (dD, dG, dW, dGrad):
        eng.device_free(p)
    eng.close()
    print(json.dumps(out))


def summary(parent_path, new_path, planset_path):
    """The set against P plain runs of the parent's build: smallest against smallest, the margin taken from the set's largest repeat."""
    par = [json.loads(l)["resident_ms_per_iteration"] for l in open(parent_path) if l.strip()]
    new = [json.loads(l)["resident_ms_per_iteration"] for l in open(new_path) if l.strip()]
    ps = json.load(open(planset_path))
    rows = []
    for r in ps["sets"]:
        P, s = r["plans"], r["set_ms_per_iteration"]
        rows.append({"plans": P, "set_ms_per_iteration": s, "set_spread_ms": round(max(s) - min(s), 4),
                     "plans_times_parent_plain_ms": round(P * min(par), 4), "plans_times_parent_plain_spread_ms": round(P * (max(par) - min(par)), 4),
                     "ratio_smallest_over_smallest": round(min(s) / (P * min(par)), 4),
                     "ratio_largest_set_over_smallest_plain": round(max(s) / (P * min(par)), 4), "margin_ms": round(P * min(par) - max(s), 4),
                     "faster_than_plans_plain_runs": max(s) < P * min(par)})
    out = {"what": "the plan set against P plain optimiser runs on C3, 2 mm dose grid: the figures of %s beside P times resident_ms_per_iteration of "
                   "profiles/optimizer_run.py from the parent commit's tree with its build (%s), and the same script from this tree (%s); one session "
                   "on one machine" % (os.path.basename(planset_path), os.path.basename(parent_path), os.path.basename(new_path)),
           "plain_parent_ms": par, "plain_parent_spread_ms": round(max(par) - min(par), 4), "plain_new_ms": new,
           "plain_new_spread_ms": round(max(new) - min(new), 4), "plain_moved_beyond_spread": not (min(new) <= max(par) and min(par) <= max(new)), "sets": rows}
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--summary":
        summary(*sys.argv[2:])
    else:
        main()
