"""Clock stamps of k_fill's blocks on the bench field (RTD_FILL_DEBUG=1) over four computes of one field — walked, recorded and
replayed, replayed, replayed: ticks per block and per batch of 8 steps, by role (0 the sigma walk or its replay, 1 the dose walk).
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
    dbg = f.fetch("fill_debug").reshape(-1, 4)[:2 * nT * L]
    dur = (dbg[:, 1] - dbg[:, 0]).astype(float)
    item = dbg[:, 3] >> 8; role = (dbg[:, 3] >> 4) & 1
    print("compute %d sigma_reused %d: blocks %d, longest block %.0f ticks" % (i, int(f.fetch("sigma_reused")[0]), dbg.shape[0], dur.max()))
    nb = np.ceil((plan[:, 5] - first) / 8.0)
    for r in (0, 1):
        m = role == r
        # the layer of a block is not in the stamp: per-batch figure from the mean number of batches over the layers
        print("   role %d: ticks per block mean %.0f median %.0f max %.0f ; per batch (mean block / mean batches %.1f) %.0f" % (r, dur[m].mean(), np.median(dur[m]), dur[m].max(), nb.mean(), dur[m].mean() / nb.mean()))
f.destroy(); eng.close()
