"""GPU tests of the dose record a field keeps beside its sigma record ("The dose record").

The compute that records the sigma walk also records, per (layer, step, ray), the difference of the cumulative depth dose that the
dose walk looks up (or a mark where the walk forces the dose to 0); the computes after it form the dose from the record, the density
and their own weights with the walk's operations in the walk's order. Nothing is reordered, so every comparison here is bitwise
(assert_array_equal, floats through their bit patterns): against a field created under RTD_NO_DOSE_REPLAY (it replays sigma and walks
the dose) and against one created under RTD_NO_TRACE_REUSE (every compute traces, plans and walks).

idd and rsigma are compared over the steps the fill writes, [beam_first_inside, afterLast of the layer), and bev over the slices the
superposition writes, [beam_first_inside, beam_first_calculated_passive): outside of them a buffer holds what it held before."""
import math

import numpy as np
import pytest

from gpu_support import FieldRig, bits, hetero_scene, options, rig_fixture
from raytracedicom_amd import scenarios

pytestmark = pytest.mark.gpu

_FETCHED = ("bev", "idd", "rsigma", "tile_radius", "eff_radius", "layer_plan", "first_passive", "active")

rig_of = rig_fixture(FieldRig)


def _compute(rig, f, names=_FETCHED):
    """One compute with a finish: ((dose_reused, sigma_reused), {dose, info, the fetched arrays})."""
    dose, info, _ = rig.compute(f)
    out = {"info": info, "dose": dose}
    for nm in names:
        out[nm] = f.fetch(nm).copy()
    return (int(f.fetch("dose_reused")[0]), int(f.fetch("sigma_reused")[0])), out


def _steps(out):
    """(beam_first_inside, afterLast per layer) of a result."""
    info = out["info"]
    plan = out["layer_plan"].reshape(info["ray_dims"][2], 8)
    return info["beam_first_inside"], [int(a) for a in plan[:, 5]]


def _written(out, nm):
    """The part of a fetched array that the compute wrote, as bit patterns where it holds floats."""
    a = out[nm]
    if nm in ("idd", "rsigma", "bev"):
        info = out["info"]
        first, after = _steps(out)
        if nm == "bev":
            S = a.size // ((info["ray_dims"][0] + 64) * (info["ray_dims"][1] + 64))
            return bits(a.reshape(S, -1)[first:max(info["beam_first_calculated_passive"], first)])
        W, H, L = info["ray_dims"]
        a = a.reshape(L, -1, H, W)
        return np.concatenate([bits(a[l, first:max(after[l], first)]).reshape(-1) for l in range(L)])
    return bits(a) if a.dtype == np.float32 else a


def _same(a, b, names=_FETCHED):
    assert a["info"] == b["info"]
    np.testing.assert_array_equal(bits(a["dose"]), bits(b["dose"]), err_msg="dose")
    for nm in names:
        np.testing.assert_array_equal(_written(a, nm), _written(b, nm), err_msg=nm)


def _runs(rig, beam, dose_expect, sigma_expect=None, **env):
    """Computes of one field with a finish in between -> the field and their results, after the check of what dose_reused (and
    sigma_reused: by default the same) read."""
    f = rig.field(beam, **env)
    runs = [_compute(rig, f) for _ in dose_expect]
    assert tuple(r[0] for r, _ in runs) == tuple(dose_expect)
    assert tuple(r[1] for r, _ in runs) == tuple(dose_expect if sigma_expect is None else sigma_expect)
    return f, [out for _, out in runs]


def _against_walking(rig, beam, outs, **env):
    """The results against a field that replays sigma but walks the dose, and against one that traces, plans and walks every time
    -> the first result of the former."""
    _, walked = _runs(rig, beam, (0, 0, 0), (0, 1, 2), **dict(env, RTD_NO_DOSE_REPLAY="1"))
    _, traced = _runs(rig, beam, (0,), **dict(env, RTD_NO_TRACE_REUSE="1"))
    for out in outs + walked[1:] + traced:
        _same(out, walked[0])
    return walked[0]


def _four_against_walking(rig, beam, **env):
    f, outs = _runs(rig, beam, (0, 1, 2, 2), **env)
    assert int(f.fetch("trace_reused")[0]) == 1
    return outs, _against_walking(rig, beam, outs, **env)


def _missing(synth, n=128):
    """A beam 1 m beside the volume: every sample is BORDER zero, the field is empty."""
    ct, voxel = scenarios.hetero_phantom(n)
    beam = scenarios.make_field(synth, n, voxel, (872.0, -128.0, -106.0), 0.0, 7, 6.0, 3, 5)
    return scenarios.Scenario("beam beside the volume", synth, ct, (voxel,) * 3, [beam])


def _set_weights(rig, f, w):
    dW = rig.eng.device_alloc(w.nbytes)
    try:
        rig.eng.to_device(dW, w)
        f.set_spot_weights(dW)
    finally:
        rig.eng.sync()
        rig.eng.device_free(dW)


@pytest.mark.parametrize("case", ["across", "diagonal", "along", "water", "missing"])
def test_four_computes(rig_of, synth, case):
    """Walked, recorded and replayed, replayed, replayed: the three sampling geometries (0 degrees; 37 degrees with a finite source
    distance; 90 degrees), water (still detected uniform, still on the uniform path) and an empty field."""
    if case == "water":
        scn = scenarios.water_cube(synth, n=64, n_layers=3, spots=7, pitch=6.0)
    elif case == "missing":
        scn = _missing(synth)
    else:
        deg, dist = {"across": (0.0, (math.inf, math.inf)), "diagonal": (37.0, (2000.0, 2500.0)), "along": (90.0, (math.inf, math.inf))}[case]
        scn = hetero_scene(synth, 128, [deg], source_dist=dist, spots=7, pitch=6.0)
    rig = rig_of(scn, options(1.0))
    outs, _ = _four_against_walking(rig, scn.beams[0])
    for out in outs:
        if case == "water":
            assert out["info"]["uniform_sigma"] == 1 and out["dose"].max() > 0
        elif case == "missing":
            assert out["dose"].max() == 0 and out["info"]["live_steps"] == 0
        else:
            assert out["info"]["uniform_sigma"] == 0 and out["dose"].max() > 0


@pytest.mark.parametrize("cutoff", [0.0, 1.0])
def test_revive_and_kill(rig_of, synth, cutoff):
    """The record is made under weights that take two spot rows out (0.5, below a cut-off of 1; exactly 0 at a cut-off of 0, where
    such a ray is alive and its dose is the product with a zero weight, signs included), then replayed under weights that bring them
    back and take two others out, then under weights with every spot in: each result equals a fresh field's walk with those weights.
    What the record holds for a ray must not depend on the weight the ray had when it was recorded."""
    scn = hetero_scene(synth, 128, [15.0], spots=7, pitch=6.0)
    b = scn.beams[0]
    out_of = np.float32(0.5 if cutoff == 1.0 else 0.0)
    w3 = b.spotWeights.copy()
    w1, w2 = w3.copy(), w3.copy()
    w1[:, :2, :] = out_of
    w2[:, -2:, :] = out_of
    names = _FETCHED + ("ray_weights",)
    rig = rig_of(scn, options(cutoff))
    f = rig.field(b.replace(spotWeights=w1))
    assert _compute(rig, f)[0] == (0, 0)
    r, first = _compute(rig, f, names)
    assert r == (1, 1)
    seen = {}
    for name, w in (("w1", w1), ("w2", w2), ("w3", w3)):
        if name != "w1":
            _set_weights(rig, f, w)
        r, got = _compute(rig, f, names)
        assert r == (2, 2)
        r0, ref = _compute(rig, rig.field(b.replace(spotWeights=w)), names)
        assert r0 == (0, 0)
        _same(got, ref, names)
        seen[name] = got
    _same(first, seen["w1"])
    assert not np.array_equal(seen["w1"]["dose"], seen["w2"]["dose"]) and not np.array_equal(seen["w2"]["dose"], seen["w3"]["dose"])
    W, H, L = first["info"]["ray_dims"]
    if cutoff == 1.0:
        # a whole 32 x 8 tile without a live ray while the record was made, with live rays when it is replayed
        live = {k: (v["ray_weights"].reshape(L, H // 8, 8, W // 32, 32) >= cutoff).any(axis=(2, 4)) for k, v in seen.items()}
        assert (~live["w1"] & live["w2"]).any() and (~live["w2"] & live["w3"]).any()
    else:
        # rays of weight exactly 0 inside the patient while the record was made, with a weight above 0 when it is replayed
        rw = {k: v["ray_weights"].reshape(L, H, W) for k, v in seen.items()}
        inside = (seen["w3"]["idd"].reshape(L, -1, H, W) > 0).any(axis=1)
        assert ((rw["w1"] == 0) & (rw["w2"] > 0) & inside).any() and ((rw["w2"] == 0) & (rw["w3"] > 0) & inside).any()


@pytest.mark.parametrize("dose_to_water", [0, 1])
def test_carry(rig_of, synth, dose_to_water):
    """mass <= 1e-2 keeps the dose of the step before. The phantom's air cavity and the air in front of the body give such steps on
    live rays (a parallel beam with rays 1 mm apart and steps of 1 mm: the step volume is 1, so the mass is the density, or the step
    of the water-equivalent depth under dose_to_water). The test counts, from the fetched density and idd, the live (layer, step, ray)
    whose density (mass) is below 0.01 and whose idd is not zero and equals the step before: without one it would prove nothing."""
    scn = hetero_scene(synth, 128, [0.0], spots=7, pitch=6.0, layers=3)
    opt = options(1.0)
    opt.dose_to_water = dose_to_water
    rig = rig_of(scn, opt)
    outs, ref = _four_against_walking(rig, scn.beams[0])
    W, H, L = ref["info"]["ray_dims"]
    S = scn.beams[0].tracerSteps
    first, after = _steps(ref)
    f = rig.fields[0]
    thick = f.fetch("density").reshape(S, H, W)
    if dose_to_water:
        wepl = f.fetch("wepl").reshape(S, H, W)
        thick = np.concatenate([wepl[:1], wepl[1:] - wepl[:-1]])
    idd = outs[3]["idd"].reshape(L, S, H, W)
    carried = 0
    for l in range(L):
        cur, prev = idd[l, first + 1:after[l]], idd[l, first:after[l] - 1]
        carried += int(((thick[first + 1:after[l]] < 1e-2) & (cur != 0) & (bits(cur) == bits(prev))).sum())
    assert carried > 0


def test_options_changed(rig_of, synth):
    """rtd_set_options between computes drops the record with the trace: the next compute walks, the one after it makes the record
    again, and each equals a field that computes for the first time under the new inputs. (A field keeps the options it was created
    under: for the field that exists the call is an epoch change, and the field it is compared with was created before the call; a
    field created after it runs under the new cut-off and is checked against its walking twins as well.)"""
    scn = hetero_scene(synth, 128, [10.0], spots=7, pitch=6.0)
    b = scn.beams[0]
    rig = rig_of(scn, options(1.0))
    f, before = _runs(rig, b, (0, 1, 2))
    fresh = rig.field(b)
    rig.eng.set_options(options(0.5))
    r0, ref = _compute(rig, fresh)
    assert r0 == (0, 0)
    after = [_compute(rig, f) for _ in range(3)]
    assert [r for r, _ in after] == [(0, 0), (1, 1), (2, 2)]
    for _, out in after:
        _same(out, ref)
    np.testing.assert_array_equal(bits(before[2]["dose"]), bits(ref["dose"]))
    later, _ = _four_against_walking(rig, b)                          # created under the cut-off of 0.5
    assert not np.array_equal(later[0]["first_passive"], ref["first_passive"])   # rays between the two cut-offs are alive now


def test_two_fields(rig_of, synth):
    """Two field objects on one handle, computed in turns: each keeps its own record."""
    scn = hetero_scene(synth, 128, [0.0, 37.0], spots=7, pitch=6.0)
    rig = rig_of(scn, options(1.0))
    fields = [rig.field(b) for b in scn.beams]
    outs = [[], []]
    for expect in (0, 1, 2, 2):
        for i, f in enumerate(fields):
            r, out = _compute(rig, f)
            assert r == (expect, expect)
            outs[i].append(out)
    for i, b in enumerate(scn.beams):
        _against_walking(rig, b, outs[i])
    assert not np.array_equal(outs[0][0]["dose"], outs[1][0]["dose"])


# name -> (CT size, layers, tracer steps)
_TAILS = {"tail": (96, 5, 512), "table_end": (128, 5, 162), "short": (128, 3, 6)}


@pytest.mark.parametrize("case", sorted(_TAILS))
def test_tail_batch(rig_of, synth, case):
    """The step counts c = afterLast - beam_first_inside of the layers against the batch of 8, and the end of the tables:
      tail        a layer with c = 7 mod 8 (full batches, then a tail batch) and one with c = 8 mod 16 (no tail)
      table_end   layers that end at the last step the planner gives (afterLast = S - 1) with c = 0 mod 8: the read-ahead of their
                  last batch lies wholly behind the step table and the record
      short       every layer has 0 < c < 8 (one tail batch, nothing else) and ends at S - 1"""
    n, layers, steps = _TAILS[case]
    scn = hetero_scene(synth, n, [0.0], spots=7, pitch=6.0, layers=layers, steps=steps)
    rig = rig_of(scn, options(1.0))
    _, ref = _four_against_walking(rig, scn.beams[0])
    assert ref["dose"].max() > 0
    first, after = _steps(ref)
    c = [a - first for a in after]
    assert all(x > 0 for x in c), (first, after)
    if case == "tail":
        assert any(x % 8 == 7 for x in c) and any(x % 16 == 8 for x in c), (first, after)
    elif case == "table_end":
        assert any(a == steps - 1 and (a - first) % 8 == 0 for a in after), (first, after)
    else:
        assert all(x < 8 for x in c) and all(a == steps - 1 for a in after), (first, after)


def test_no_dead_skip(rig_of, synth):
    """RTD_NO_DEAD_SKIP with the replay: every dead value stored, the same results; and equal to the field with the dead-store rules."""
    scn = hetero_scene(synth, 128, [20.0], spots=7, pitch=6.0)
    rig = rig_of(scn, options(1.0))
    outs, _ = _four_against_walking(rig, scn.beams[0], RTD_NO_DEAD_SKIP="1")
    _, plain = _runs(rig, scn.beams[0], (0, 1, 2))
    for out in plain:
        _same(out, outs[3])


def test_fill_that_does_not_fit(rig_of, synth):
    """A field keeps a dose record only while all blocks of its fill are resident on the GPU at once. RTD_DOSE_REPLAY_BLOCKS sets
    the number of blocks taken to fit: with 1 the field replays sigma and walks the dose (dose_reused stays 0 while sigma_reused
    reads 0, 1, 2, 2), with the field's own block count it keeps the record, with one less it does not; the results are the same."""
    scn = hetero_scene(synth, 128, [20.0], spots=7, pitch=6.0)
    b = scn.beams[0]
    rig = rig_of(scn, options(1.0))
    _, kept = _runs(rig, b, (0, 1, 2, 2))
    W, H, L = kept[0]["info"]["ray_dims"]
    blocks = 2 * (W // 32) * (H // 8) * L
    _, none = _runs(rig, b, (0, 0, 0, 0), (0, 1, 2, 2), RTD_DOSE_REPLAY_BLOCKS="1")
    _, below = _runs(rig, b, (0, 0, 0), (0, 1, 2), RTD_DOSE_REPLAY_BLOCKS=str(blocks - 1))
    _, at = _runs(rig, b, (0, 1, 2), RTD_DOSE_REPLAY_BLOCKS=str(blocks))
    for out in kept[1:] + none + below + at:
        _same(out, kept[0])
