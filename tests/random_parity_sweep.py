"""Random parity sweep on a GPU box (not collected by pytest): seeded random scenarios through tests/gpu_support.compare_field,
every intermediate and the dose against the CPU oracle. Usage: python tests/random_parity_sweep.py FIRST_SEED END_SEED [rays | angles].
Ray weights and every integer are compared bit for bit; dose deviations confined to the tail are reported and the sweep goes on;
anything else raises."""
import os, sys, math
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
torch.zeros(1, device="cuda")
from oracle import oracle as orc
from raytracedicom_amd import engine, luts, scenarios
import gpu_support as T
orc.lib(); orc.set_threads(16)
synth = luts.synth_luts()
n_ok = 0
for seed in range(int(sys.argv[1]), int(sys.argv[2])):
    rng = np.random.default_rng(5000 + seed)
    n = int(rng.choice([48, 64, 96, 128]))
    ct, _ = scenarios.hetero_phantom(n, seed=int(rng.integers(1, 99)))
    spots = int(rng.integers(1, 14)); pitch = float(rng.choice([2.5, 4.0, 6.0, 9.0]))
    n_layers = int(rng.choice([1, 2, 3, 7, 14, 15, 17, 23, 30]))
    deg = float(rng.choice([0.0, 13.0, 45.0, 90.0, 141.0, 180.0, 270.0, 300.0]))
    dist = (math.inf, math.inf) if rng.random() < 0.4 else (float(rng.uniform(900, 3000)), float(rng.uniform(900, 3000)))
    steps = int(rng.choice([97, 200, 256, 333, 512, 600]))
    # (drawn last, so the scenarios of the earlier sweeps keep their seeds) a quarter of the scenarios with finer rays: batch radii
    # beyond 16 pixels, the second sweep launch
    rs = float(rng.choice([1.0, 1.0, 1.0, 0.75, 0.6])) if len(sys.argv) > 3 and sys.argv[3] == "rays" else 1.0
    if len(sys.argv) > 3 and sys.argv[3] == "angles":      # any gantry angle (the host's choice among the three sampling kernels, the transfers' lane axes)
        deg = float(rng.uniform(0.0, 360.0))
    if rs != 1.0:
        spots = min(spots, 6)
    scn = scenarios.hetero_ct(synth, n=n, spots=spots, pitch=pitch, n_layers=n_layers, angles=[deg], source_dist=dist, steps=steps, ct=ct,
                              ray_spacing=(rs, rs))
    try:
        T.compare_field(orc, engine, scn, scn.beams[0])
    except RuntimeError as e:
        if "larger than allowed" not in str(e):
            raise
        print("seed", seed, "radius overflow reported (a class beyond 32: the reference throws there too), rays", rs)
        continue
    except AssertionError as e:
        import traceback
        tb = traceback.format_exc()
        if "of.status == 0" in tb:             # the oracle stopped (a radius class beyond 32, where the reference throws): the engine must report it too
            rig = T.FieldRig(engine, scn, None)
            try:
                rig.compute(rig.field(scn.beams[0]))
                raise SystemExit("seed %d: the oracle reports an error, the engine does not" % seed)
            except RuntimeError as e2:
                assert "larger than allowed" in str(e2), str(e2)
            finally:
                rig.close()
            print("seed", seed, "radius overflow: oracle and engine both report it, rays", rs)
            continue
        if "(1.0, 0, 0.0)" in str(e):          # pencil too thin for the gamma sampling grid: every other comparison passed
            print("seed", seed, "gamma had no voxels to evaluate (all other comparisons passed)")
        elif "max rel err" in str(e):
            print("seed", seed, "ABOVE-FLOOR deviation:", str(e))
        elif "err[~mask]" in tb:               # tail voxels (< 1e-3 of max) beyond the tight floor tolerance: radius-class flip
            print("seed", seed, "TAIL-ONLY deviation (voxels below 1e-3 of the maximum)")
        elif "tile_radius differs" in str(e):
            print("seed", seed, "RADIUS-CLASS difference:", str(e)[:300])
        else:
            raise
    n_ok += 1
    print("seed", seed, "ok", n, spots, pitch, n_layers, deg, steps, rs, flush=True)
print("all", n_ok, "ok")
