"""GPU tests of k_fill's dead stores (rtd_fill.hpp DEAD STORES).

The replaying build leaves out the stores of a wave whose rays have all ended, and those of a wave that is dead from its start when
the bytes of its segments say that memory holds the dead values already. What can go wrong is a byte that says so when memory does
not: every test here moves rays between live and dead and compares every compute, bit for bit, with the first compute of a fresh
field under RTD_NO_DEAD_SKIP=1 and of one under RTD_NO_TRACE_REUSE=1, over everything the compute writes (the dose, the BEV dose, the
dose and 1/sigma arrays over the steps of each layer, the tile radii, the plan, the rays' last steps, the active rectangles).

The scene (96^3 heterogeneous phantom, 7 x 7 spots 6 mm apart, 4 layers, ray-weight cut-off 1) with the three left spot columns
below the cut-off has, as asserted from the fetched ray weights and last steps: a tile without a live ray, a tile that holds live
waves and dead ones (1 .. 12 of its 16 segments of 16 rays hold a live ray: the lane placement packs them into its first waves), and
live rays that end more than two batches before their layer's last step."""
import numpy as np
import pytest

from dead_work_support import FETCHED, compute, reference, same, set_weights, steps
from gpu_support import FieldRig, hetero_scene, nuc_luts, options, rig_fixture  # noqa: F401 (nuc_luts: a fixture)

pytestmark = pytest.mark.gpu

rig_of = rig_fixture(FieldRig)

CUTOFF = 1.0


def _scene(synth, **kw):
    return hetero_scene(synth, 96, [0.0], spots=7, pitch=6.0, layers=4, **kw)


def _left_dead(w):
    """The three left spot columns below the cut-off."""
    w = w.copy()
    w[:, :, :3] = 0.0
    return w


def _checked(out):
    """The stated properties of the scene, from what the compute fetched."""
    W, H, L = out["info"]["ray_dims"]
    first, after = steps(out)
    live = out["ray_weights"].reshape(L, H, W) >= CUTOFF
    segs = live.reshape(L, H // 8, 8, W // 32, 2, 16).any(axis=5)              # [layer][tile row][row][tile column][half row]
    n_live = segs.sum(axis=(2, 4))                                             # live segments per (layer, tile row, tile column)
    assert (n_live == 0).any(), n_live
    assert ((n_live >= 1) & (n_live <= 12)).any(), n_live
    last = out["first_passive"].reshape(L, H, W)
    assert any((live[l] & (last[l] > first) & (last[l] < after[l] - 16)).any() for l in range(L)), (first, after)


def _weights_sequence(rig, beam, f=None, expect_replay=True):
    """Zero -> nonzero (dead segments come alive), back to zero (live segments die: stored dead once, then skipped), nonzero and zero
    again, all zero, and back: every compute against a fresh reference field with the same weights."""
    full = beam.spotWeights.astype(np.float32)
    part = _left_dead(full)
    refs = {"part": reference(rig, beam.replace(spotWeights=part)), "full": reference(rig, beam),
            "none": reference(rig, beam.replace(spotWeights=np.zeros_like(full)))}
    weights = {"part": part, "full": full, "none": np.zeros_like(full)}
    if f is None:
        f = rig.field(beam.replace(spotWeights=part))
    for _ in range(3):                                                # walked, recorded and replayed, replayed
        same(compute(rig, f), refs["part"])
    for key in ("full", "part", "part", "full", "part", "none", "none", "part", "full"):
        set_weights(rig, f, weights[key])
        out = compute(rig, f)
        if expect_replay:
            assert out["sigma_reused"] == 2 and out["trace_reused"] == 1
        same(out, refs[key])
    assert refs["full"]["dose"].max() > 0 and refs["none"]["dose"].max() == 0
    return f


def test_unchanged_weights(rig_of, synth):
    """Four computes of one field (walked, recorded and replayed, replayed, replayed) equal the references."""
    scn = _scene(synth)
    beam = scn.beams[0].replace(spotWeights=_left_dead(scn.beams[0].spotWeights.astype(np.float32)))
    rig = rig_of(scn, options(CUTOFF))
    ref = reference(rig, beam, names=FETCHED + ("ray_weights",))
    _checked(ref)
    f = rig.field(beam)
    outs = [compute(rig, f) for _ in range(4)]
    assert tuple(o["sigma_reused"] for o in outs) == (0, 1, 2, 2)
    for o in outs:
        same(o, ref)
    assert ref["dose"].max() > 0


def test_changed_weights(rig_of, synth):
    scn = _scene(synth)
    _weights_sequence(rig_of(scn, options(CUTOFF)), scn.beams[0])


def test_natural_lane_order(rig_of, synth):
    """RTD_NO_FILL_COMPACT: a wave holds the segments of two tile rows as they lie."""
    scn = _scene(synth)
    rig = rig_of(scn, options(CUTOFF))
    f = rig.field(scn.beams[0].replace(spotWeights=_left_dead(scn.beams[0].spotWeights.astype(np.float32))), RTD_NO_FILL_COMPACT="1")
    _weights_sequence(rig, scn.beams[0], f)


def test_nuclear_halo(rig_of, nuc_luts):
    """NUCLEAR_CORR: every fill walks (and keeps the bytes)."""
    scn = _scene(nuc_luts)
    _weights_sequence(rig_of(scn, options(CUTOFF, nuclear=1)), scn.beams[0], expect_replay=False)


@pytest.mark.parametrize("change", ["ct", "luts", "cutoff"])
def test_new_epoch(rig_of, synth, change):
    """A change of CT, LUTs or options: the next compute traces and walks, and the bytes are rebuilt from what it stores. (A field
    keeps the cut-off it was created under: the new one makes a new epoch for it and changes nothing else.)"""
    scn = _scene(synth)
    b = scn.beams[0]
    part = b.replace(spotWeights=_left_dead(b.spotWeights.astype(np.float32)))
    rig = rig_of(scn, options(CUTOFF))
    f = rig.field(part)
    ref, ref_full = reference(rig, part), reference(rig, b)
    for _ in range(3):
        same(compute(rig, f), ref)
    if change == "ct":
        ct = scn.ct.copy()
        ct[:, :, : ct.shape[2] // 2] = np.minimum(ct[:, :, : ct.shape[2] // 2] + 150.0, 3071.0)
        rig.eng.set_ct(ct)
    elif change == "luts":
        rig.eng.set_luts(scn.luts)
    else:
        rig.eng.set_options(options(40.0))
    ref2, ref_full2 = (ref, ref_full) if change == "cutoff" else (reference(rig, part), reference(rig, b))
    outs = [compute(rig, f) for _ in range(4)]
    assert tuple(o["sigma_reused"] for o in outs) == (0, 1, 2, 2) and outs[0]["trace_reused"] == 0
    for o in outs:
        same(o, ref2)
    if change == "ct":
        assert not np.array_equal(ref2["dose"], ref["dose"])
    set_weights(rig, f, b.spotWeights.astype(np.float32))
    same(compute(rig, f), ref_full2)


def test_dose_influence_between_computes(rig_of, synth):
    """The batches of the dose-influence matrix go through k_fill with weights of their own: the bytes follow them."""
    scn = _scene(synth)
    b = scn.beams[0]
    rig = rig_of(scn, options(0.0))
    f = rig.field(b)
    ref = reference(rig, b)
    for _ in range(3):
        same(compute(rig, f), ref)
    assert f.dose_influence().nnz > 0
    for _ in range(2):
        same(compute(rig, f), ref)
    part = _left_dead(b.spotWeights.astype(np.float32))
    set_weights(rig, f, part)
    same(compute(rig, f), reference(rig, b.replace(spotWeights=part)))


def test_released_workspace(rig_of, synth):
    """A released field's workspace (its bytes set by the replaying computes above) goes to a new field of the same geometry, all of
    whose spot columns are alive: the new field's computes — walked, recorded and replayed, replayed — equal the references. What
    protects them is the reset in front of the new field's first, walking fill, which clears every byte; the clearing at the takeover
    itself is defensive and this test cannot tell whether it is there."""
    scn = _scene(synth)
    b = scn.beams[0]
    part = b.replace(spotWeights=_left_dead(b.spotWeights.astype(np.float32)))
    rig = rig_of(scn, options(CUTOFF))
    f = rig.field(part)
    ref = reference(rig, part)
    for _ in range(3):
        same(compute(rig, f), ref)
    rig.fields.remove(f)
    f.release()
    other = b                                                         # (the same geometry, every spot column alive)
    f2 = rig.field(other)
    ref2 = reference(rig, other)
    for _ in range(3):
        same(compute(rig, f2), ref2)
    assert not np.array_equal(ref2["dose"], ref["dose"])
