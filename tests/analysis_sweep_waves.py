# (not collected by pytest: an analysis script on the CPU oracle, kept beside the tests because only tests may use the oracle)
"""How k_superpose_sweep's weight-table build sees a field (CPU oracle): per wave row-layer — (layer, step, source row, 64-column
segment of the patch grid) with at least one live source — the wave's radius rhoRow = max of its lanes' batch radii (<= 16), whether
the wave has erf lanes (1/sigma > 0.75, rtd_sweep.hpp swBuildT), whether it mixes them with series lanes, and whether some live lane
ends below rhoRow (its own tile's radius is smaller, or it is an erf lane whose entries stop at 5).

The patch grid starts at the corner of the rectangle of rays that carry dose (here: IDD > 0 over all layers and steps; the engine
takes it from the spot -> ray weights, which can only widen it). 1/sigma is the oracle's: at the 0.75 threshold the engine's own
value (rtol 2e-5) may fall on the other side for a few lanes.

Usage: python tests/analysis_sweep_waves.py [n = 512] [deg = 0]"""
import os
import sys

import numpy as np

SERIES_MAX_RS = np.float32(0.75)
MAX_R = 16


def wave_stats(of, beam):
    W, H, L = of.info["ray_dims"]
    S = beam.tracerSteps
    idd = of.get("idd").reshape(L, S, H, W)
    rsg = of.get("rsigma").reshape(L, S, H, W)
    tr = of.get("tile_radius").reshape(L, S, H // 8, W // 32)
    eff = of.get("eff_radius").reshape(L, -1)
    plan = of.get("layer_plan").reshape(L, 8)
    first = of.info["beam_first_inside"]
    live = (idd > 0).any(axis=(0, 1))
    xs = np.nonzero(live.any(axis=0))[0]
    ux0 = int(xs.min()) if xs.size else 0
    nP = (W - ux0 + 63) // 64
    st = dict(wave_row_layers=0, with_erf=0, mixed=0, short=0, short_series_only=0, rho16=0, rho_hist=np.zeros(MAX_R + 1, np.int64))
    for l in range(L):
        for k in range(first, int(plan[l, 6])):
            d = idd[l, k]
            if not (d > 0).any():
                continue
            r = tr[l, k]
            rr = np.where(r <= 32, eff[l][np.minimum(r, 33)], -1)
            rho = np.repeat(np.repeat(rr, 8, axis=0), 32, axis=1)[:H, :W]
            rho = np.where((d > 0) & (rho <= MAX_R), rho, -1)
            rs = rsg[l, k]
            pad = nP * 64 - (W - ux0)
            rho = np.pad(rho[:, ux0:], ((0, 0), (0, pad)), constant_values=-1).reshape(H, nP, 64)
            rs = np.pad(rs[:, ux0:], ((0, 0), (0, pad)), constant_values=0).reshape(H, nP, 64)
            alive = rho >= 0
            wav = alive.any(axis=2)
            if not wav.any():
                continue
            erf = alive & ~(rs <= SERIES_MAX_RS)
            ser = alive & ~erf
            rhoRow = rho.max(axis=2)
            last = np.where(erf, np.minimum(rho, 5), rho)
            short = (alive & (last < rhoRow[:, :, None])).any(axis=2)
            shortS = (ser & (rho < rhoRow[:, :, None])).any(axis=2)
            anyE = erf.any(axis=2)
            st["wave_row_layers"] += int(wav.sum())
            st["with_erf"] += int((wav & anyE).sum())
            st["mixed"] += int((wav & anyE & ser.any(axis=2)).sum())
            st["short"] += int((wav & short).sum())
            st["short_series_only"] += int((wav & ~anyE & shortS).sum())
            st["rho16"] += int((wav & (rhoRow == MAX_R)).sum())
            st["rho_hist"] += np.bincount(rhoRow[wav], minlength=MAX_R + 1)[:MAX_R + 1]
    return st


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from raytracedicom_amd import luts, scenarios
    from oracle import oracle
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    deg = float(sys.argv[2]) if len(sys.argv) > 2 else 0.0
    es = luts.synth_luts()
    ct, _ = scenarios.hetero_phantom(n)
    scn = scenarios.hetero_ct(es, n=n, angles=[deg], ct=ct)
    dose = np.zeros_like(scn.ct)
    of = oracle.run_field(scn, scn.beams[0], dose, keep_layers=True)
    st = wave_stats(of, scn.beams[0])
    tot = st["wave_row_layers"]
    for key in ("with_erf", "mixed", "short", "short_series_only", "rho16"):
        print("%-18s %8d  (%.1f %%)" % (key, st[key], 100.0 * st[key] / max(tot, 1)))
    print("wave row-layers    %8d" % tot)
    print("by rhoRow:", {i: int(v) for i, v in enumerate(st["rho_hist"]) if v})
