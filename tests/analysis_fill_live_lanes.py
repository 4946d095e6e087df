# (not collected by pytest: an analysis script on the CPU oracle, kept beside the tests because only tests may use the oracle)
# How many of k_fill's issued lane-steps belong to a ray that is alive, and how many waves hold a live ray when a tile's rays are
# dealt to its block's lanes by segments of 32 (the natural order), 16, 8 or 4 consecutive rays, live segments first (DESIGN.md
# section 4, K5 "Lane placement"). The bench field, set up as in analysis_fill_placement.py. Counts, not times.
import sys; import os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from raytracedicom_amd import luts, scenarios
from oracle import oracle
es=luts.synth_luts()
ct,_=scenarios.hetero_phantom(256)   # CT resolution does not matter for the BEV-side quantities
scn=scenarios.hetero_ct(es,n=256,angles=[0.0],ct=ct)
d=np.zeros_like(scn.ct); of=oracle.run_field(scn,scn.beams[0],d,keep_layers=True)
W,H,L=of.info["ray_dims"]
plan=of.get("layer_plan").reshape(L,8); first=of.info["beam_first_inside"]
rw=of.get("ray_weights").reshape(L,H,W)
fp=of.get("first_passive").reshape(L,H,W)
tx,ty=W//32,H//8; nT=tx*ty
steps=plan[:,5].astype(int)-first                    # steps of the layer's walks
live=rw>=1.0                                         # alive at the start of the walk (ray_weight_cutoff = 1)
alive=np.where(live,np.clip(fp-first,0,None),0)      # steps until the ray has passed its last step
print("ray grid %dx%dx%d, %d rays x %d live layer-steps = %.1f M lane-steps per role"%(W,H,L,W*H,steps.sum(),W*H*steps.sum()/1e6))
print("lane-steps of a ray that is alive: %.1f M (%.0f %%)"%(alive.sum()/1e6,100.0*alive.sum()/(W*H*steps.sum())))
frac=live.reshape(L,-1).mean(axis=1)
print("rays live at the start, per layer: %.0f .. %.0f %%"%(100*frac.min(),100*frac.max()))
tiles=live.reshape(L,ty,8,tx,32).any(axis=(2,4)).reshape(L,-1).sum(axis=1)
print("tiles with a live ray, per layer: %d .. %d of %d"%(tiles.min(),tiles.max(),nT))
share={}
for seg in (32,16,8,4):
    n=live.reshape(L,ty,8,tx,32//seg,seg).any(axis=5).sum(axis=(2,4)).reshape(L,nT)     # live segments per (layer, tile)
    waves=-(-n//(64//seg))                                                               # whole waves they fill
    share[seg]=(waves.sum(axis=1)*steps).sum()/(4.0*nT*steps.sum())                      # weighted by the layer's steps
print("segment width (lanes) | waves that hold a live ray | issue work against today's, a dead wave priced at 0.35 / 0.1 of a live one")
for seg,sh in share.items():
    today=share[32]+0.35*(1-share[32])
    print("%21d | %5.1f %% = %4.1f M lane-steps | %.2f / %.2f"%(seg,100*sh,sh*W*H*steps.sum()/1e6,(sh+0.35*(1-sh))/today,(sh+0.1*(1-sh))/today))
