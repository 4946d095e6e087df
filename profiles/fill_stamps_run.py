"""Clock stamps of k_fill's blocks on the bench field (RTD_FILL_DEBUG=1) over four computes of one field — walked, recorded and
replayed, replayed, replayed: ticks per block and per batch of 8 steps, by role (0 the sigma walk or its replay, 1 the dose walk).
A replaying compute has a block per step segment of a walk (RTD_FILL_SEG_STEPS; the stamp's word 3 holds the segment above bit 40
and 1 in bit 0 for a block whose segment lies behind its layer's steps). The clocks of different XCDs do not agree, so what a launch
spans is taken per CU (first start to last end of the blocks the CU ran): the mean and the longest span over the CUs, the block ticks
a CU ran per tick of its span, and for the CU that ended last which block ended it and when that block had started.
Run from the root of the tree whose build is to be measured (profiles/r20_fill_stamps_*.txt); tools/fill_dbg.py has the per-CU view."""
import os, sys
os.environ["RTD_FILL_DEBUG"] = "1"
sys.path.insert(0, os.getcwd())
import numpy as np
import torch
torch.cuda.init()
from raytracedicom_amd import engine, luts, scenarios
es = luts.synth_luts()
ct, _ = scenarios.hetero_phantom(512)
scn = scenarios.hetero_ct(es, n=512, angles=[0.0], ct=ct)
eng = engine.Engine(0)
eng.set_luts(es); eng.set_ct(scn.ct)
d = eng.device_alloc(4 * scn.n_voxels); eng.device_zero(d, 4 * scn.n_voxels)
f = eng.create_field(scn.beams[0], scn.dims)
for i in range(4):
    f.compute(d); t, info = f.finish()
    W, H, L = info["ray_dims"]; nT = (W // 32) * (H // 8)
    plan = f.fetch("layer_plan").reshape(L, 8); first = info["beam_first_inside"]
    dbg = f.fetch("fill_debug").reshape(-1, 4)
    if int(f.fetch("dose_reused")[0]) == 0: dbg = dbg[:2 * nT * L]    # (a walking compute: one block per walk, the other rows are older)
    dbg = dbg[dbg[:, 1] != 0]
    left = (dbg[:, 3] & 1) == 1
    dur = (dbg[:, 1] - dbg[:, 0]).astype(float)
    item = (dbg[:, 3] >> 8) & 0xffffffff; role = (dbg[:, 3] >> 4) & 1; seg = dbg[:, 3] >> 40
    print("compute %d sigma_reused %d: blocks %d (%d without steps), longest block %.0f ticks" % (i, int(f.fetch("sigma_reused")[0]), dbg.shape[0], int(left.sum()), dur.max()))
    if (dbg[:, 2] != 0).any():
        hw = dbg[:, 2]; cu = ((hw >> 32) & 0xF) << 16 | ((hw >> 13) & 7) << 8 | ((hw >> 12) & 1) << 4 | ((hw >> 8) & 0xF)
        cu = np.where(left, -1, cu)                                   # (a block without steps leaves no hardware id)
        spans = []
        for k in np.unique(cu[cu >= 0]):
            m = cu == k; t0 = dbg[m, 0].min(); j = np.flatnonzero(m)[np.argmax(dbg[m, 1])]
            spans.append((float(dbg[j, 1] - t0), float(dur[m].sum()), int(role[j]), int(seg[j]), float(dbg[j, 0] - t0), float(dur[j])))
        spans.sort()
        sp = np.array([s[0] for s in spans]); work = np.array([s[1] for s in spans])
        print("   per CU (%d): span mean %.0f longest %.0f ticks; block ticks per tick of span mean %.2f; the CU that ended last: by a role %d block of segment %d that started %.0f ticks in and took %.0f"
              % (len(spans), sp.mean(), sp.max(), (work / sp).mean(), spans[-1][2], spans[-1][3], spans[-1][4], spans[-1][5]))
    dbg, dur, role = dbg[~left], dur[~left], role[~left]
    nb = np.ceil((plan[:, 5] - first) / 8.0)
    for r in (0, 1):
        m = role == r
        # the layer of a block is not in the stamp: per-batch figure from the mean number of batches over the layers
        print("   role %d: ticks per block mean %.0f median %.0f max %.0f ; per batch (mean block / mean batches %.1f) %.0f" % (r, dur[m].mean(), np.median(dur[m]), dur[m].max(), nb.mean(), dur[m].mean() / nb.mean()))
f.destroy(); eng.close()
