#!/usr/bin/env python3
"""Times, with hipEvents around compute + transfer, the first (cold: traced and planned) compute of the C3 field (512^3 heterogeneous
CT, 10x10 spots x 20 layers, inputs resident) and the computes after it, which reuse the field's trace and plan; and the same with
RTD_NO_TRACE_REUSE in the environment of the field's creation (every compute traces). Each compute is finished before the next is
launched (the reuse needs a finished compute), so these are latencies of one plan on a drained stream, not bench.py's pipelined
steps. Prints one JSON line. Usage: python profiles/trace_reuse_run.py [K]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (torch's HIP runtime initialises first, as in bench.py)

from raytracedicom_amd import abi, engine, luts, scenarios  # noqa: E402
from profiles.gradient_run import _hip  # noqa: E402


def run(eng, scn, d, steps, hip, no_reuse):
    if no_reuse:
        os.environ["RTD_NO_TRACE_REUSE"] = "1"
    try:
        f = eng.create_field(scn.beams[0], scn.dims)
    finally:
        os.environ.pop("RTD_NO_TRACE_REUSE", None)
    s = C.c_void_p(eng.stream())
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip.hipEventCreate(C.byref(e0)); hip.hipEventCreate(C.byref(e1))
    ms, total, reused = [], [], []
    for _ in range(steps + 1):
        eng.sync()
        hip.hipEventRecord(e0, s)
        f.compute_bev()
        f.transfer_init(d)
        hip.hipEventRecord(e1, s)
        hip.hipEventSynchronize(e1)
        v = C.c_float()
        hip.hipEventElapsedTime(C.byref(v), e0, e1)
        t, _ = f.finish()
        ms.append(v.value)
        total.append(t["total_ms"])
        reused.append(int(f.fetch("trace_reused")[0]))
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    f.destroy()
    later, later_total = sorted(ms[1:]), sorted(total[1:])
    return {"first_ms": ms[0], "first_total_ms": total[0], "later_ms_median": later[len(later) // 2], "later_ms_min": later[0],
            "later_total_ms_median": later_total[len(later_total) // 2], "trace_reused": reused, "steps": steps}


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    hip = _hip()
    es = luts.synth_luts()
    scn = scenarios.hetero_ct(es, n=512, n_fields=1)
    torch.cuda.synchronize()
    eng = engine.Engine(0)
    eng.set_options(abi.default_options())
    eng.set_luts(es)
    eng.set_ct(scn.ct)
    d = eng.device_alloc(4 * scn.n_voxels)
    eng.device_zero(d, 4 * scn.n_voxels)
    out = {"case": "C3", "reuse": run(eng, scn, d, steps, hip, False), "no_reuse": run(eng, scn, d, steps, hip, True)}
    eng.device_free(d)
    eng.close()
    print(json.dumps({"trace_reuse": out}))


if __name__ == "__main__":
    main()
