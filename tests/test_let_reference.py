"""CPU checks of the numpy restatement of the LET rules (tests/let_reference.py) and of luts.synth_let: the restated depth against
geometry on a water phantom, the table lookup on a table that is linear in the sample index, and the synthetic table's properties."""
import math

import numpy as np

import let_reference as R
from raytracedicom_amd import luts, scenarios

F = np.float32
U = 2.0 ** -24


def gamma(n):
    return (n + 1) * U / (1.0 - (n + 1) * U)


def test_depth_is_geometric_depth_times_stopping_power():
    """A beam along -z of the gantry (= the dose grid's z axis) through a uniform phantom of relative stopping power sp, entered at
    step `first`: a voxel whose step coordinate k lies in [first, S - 1] has the depth (k - first + 1/2) * step * sp, the mid-point
    rule continued linearly. Behind the last step the depth is that of the last step; in front of step first - 1 it is 0.

    The bound is derived, not tuned. wepl[k] is a chain of at most S float32 additions of c = float32(sp * step); the mid-point
    adds 2 operations and the three blends 3 each, so the value carries at most gamma(S + 12) * depth_max. The step coordinate is
    the result of at most 16 float32 operations on magnitudes up to K (the offsets of the transfer parameters plus S plus the
    padding), so it is off by at most 16 u K steps, which the slope c turns into 16 u K c."""
    es = luts.synth_luts(n_energies=8, n_samples=64, n_hu=1200)
    n, voxel, S, first, sp, step = 64, 4.0, 200, 20, 1.04, 1.0
    origin = (-128.0, -128.0, -106.0)
    beam = scenarios.make_field(es, n, voxel, origin, 0.0, 3, 8.0, 1, 1, steps=S, step_len=step)
    W, H = 32, 24
    info = {"ray_res": [1.0, 1.0, -step], "ray_offset": [-16.0, -12.0, 128.0], "ray_dims": [W, H, 1], "beam_first_inside": first}
    c = F(sp * step)
    wepl = np.zeros(S, dtype=F)
    acc = F(0.0)
    for k in range(first, S):
        acc = F(acc + c)
        wepl[k] = acc
    wepl = np.broadcast_to(wepl[:, None, None], (S, H, W)).copy()
    tr = R.Transfer(beam, info)
    depth = R.box_depth(tr, wepl, (0, 0, 0), (n - 1, n - 1, n - 1))
    assert depth.dtype == F and depth.shape == (n, n, n)
    # the geometry in float64: gantry z of a voxel plane, its step coordinate
    gz = origin[2] + voxel * np.arange(n, dtype=np.float64)
    k = (gz - info["ray_offset"][2]) / info["ray_res"][2]
    want = np.where(k >= S - 1, (S - 1 - first + 0.5) * step * sp, np.where(k >= first, (k - first + 0.5) * step * sp, 0.0))
    checked = (k >= first) | (k <= first - 1)                         # (between first - 1 and first the rule's ramp is not geometric)
    assert (k >= S - 1).any() and ((k >= first) & (k < S - 1)).sum() > 20 and (k < first - 1).any()
    K = abs(float(tr.global_offset[2])) + abs(float(tr.coef_offset[2])) + S + 2 * 32 + first
    bound = gamma(S + 12) * float(want.max()) + 16 * U * K * float(c)
    err = np.abs(depth.astype(np.float64) - want[:, None, None])
    assert err[checked].max() <= bound, (err[checked].max(), bound)
    assert bound < 1e-2                                               # (mm: the bound is a rounding bound, not a tolerance)
    # lateral positions outside the ray grid are clamped, not zeroed: every voxel of a plane has the plane's depth
    assert np.all(np.abs(depth.astype(np.float64) - depth[:, :1, :1]) <= 4 * U * want.max() + 1e-30)


def test_lookup_on_a_linear_table():
    n_e, n_s = 4, 33
    table = (10.0 * np.arange(n_e)[:, None] + 0.5 * np.arange(n_s)[None, :]).astype(F)
    j = np.arange(n_s, dtype=F)
    for row in range(n_e):
        assert np.array_equal(R.lookup(table, F(row), F(1.0), j), table[row])                      # at the sample points
        assert np.array_equal(R.lookup(table, F(row), F(2.0), j[:16] * F(0.5)), table[row][:16])   # ... through the scale
    mid = R.lookup(table, F(1.0), F(1.0), j[:-1] + F(0.25))
    assert np.array_equal(mid, (table[1][:-1] + F(0.125)).astype(F))                               # linear between them
    ends = R.lookup(table, F(2.0), F(1.0), np.array([-3.0, -0.0, 32.0, 32.5, 1e6, np.inf, np.nan], dtype=F))
    assert np.array_equal(ends, np.array([table[2, 0], table[2, 0], table[2, 32], table[2, 32], table[2, 32], table[2, 32], table[2, 0]], dtype=F))
    # between rows: the fill's row weight; beyond the last row both rows are the last one
    assert np.array_equal(R.lookup(table, F(1.5), F(1.0), j), (table[1] + F(5.0)).astype(F))
    assert np.array_equal(R.lookup(table, F(7.25), F(1.0), j), table[3])
    assert np.array_equal(R.lookup(table, F(-1.0), F(1.0), j), table[0])


def test_let_values_are_the_product():
    table = (1.0 + np.arange(3)[:, None] + 0.25 * np.arange(9)[None, :]).astype(F)
    plan = np.array([[0.0, 1.0], [2.0, 0.5]], dtype=F)                # layer 0: row 0, scale 1; layer 1: row 2, scale 1/2
    indptr = np.array([0, 2, 2, 3, 5])                                # four spots, two per layer
    rows = np.array([0, 3, 1, 2, 3])
    vals = np.array([1.5, 2.0, 3.0, 0.5, 7.0], dtype=F)
    depth = np.array([0.0, 2.0, 4.0, 100.0], dtype=F)
    got = R.let_values(vals, rows, indptr, 2, plan, table, depth)
    want = np.array([1.5 * table[0, 0], 2.0 * table[0, 8], 3.0 * table[2, 1], 0.5 * table[2, 2], 7.0 * table[2, 8]], dtype=F)
    assert got.dtype == F and np.array_equal(got, want)


def test_synth_let():
    es = luts.synth_luts(n_energies=12, n_samples=128, n_hu=1200)
    t = luts.synth_let(es)
    assert t.dtype == F and t.shape == (es.nEnergies, es.nEnergySamples)
    assert np.isfinite(t).all() and (t >= 0).all()
    assert np.array_equal(t, luts.synth_let(es))
    assert np.array_equal(t, luts.synth_let(luts.synth_luts(n_energies=12, n_samples=128, n_hu=1200)))
    for i in range(es.nEnergies):
        peak = int(math.floor(float(es.peakDepths[i]) * float(es.scaleFacts[i])))   # the last sample not behind the peak
        assert 0 < peak < es.nEnergySamples - 1
        assert np.all(np.diff(t[i, :peak + 1]) >= 0), i
        assert t[i, peak] > 2.0 * t[i, 0]                            # (it does rise towards the peak)
        cap = t[i, -1]
        assert np.all(t[i, peak + 1:] <= cap) and t[i, peak + 2] == cap            # finite behind the peak: the cap of the floored range
    # the cap is the formula at the floor
    want = 0.1 * (luts.LET_R_MIN_MM / 10.0) ** (1.0 / luts.LET_P - 1.0) / (luts.LET_P * luts.LET_ALPHA ** (1.0 / luts.LET_P))
    assert t.max() == F(want)
