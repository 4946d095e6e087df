"""CPU checks of raytracedicom_amd.robust: the two ways a caller makes an error scenario with what exists."""
import numpy as np

from raytracedicom_amd import robust, scenarios


def _apply32(t, g):
    """The float32 transform as the engine receives it (abi.make_affine), evaluated in float32: m g + v."""
    a = t.as_abi()
    m = np.array(list(a.m), dtype=np.float32).reshape(3, 3)
    v = np.array(list(a.v), dtype=np.float32)
    g = np.asarray(g, dtype=np.float32)
    return ((m[:, 0] * g[0] + m[:, 1] * g[1]).astype(np.float32) + m[:, 2] * g[2]).astype(np.float32) + v


def _beam(es, deg):
    n, voxel = 96, 256.0 / 96
    b = scenarios.make_field(es, n, voxel, (-128.0, -128.0, -106.0), deg, 5, 8.0, 3, seed=3)
    # a dose grid of its own (2 mm), so that the two transforms differ
    b.gantryToDoseIdx = scenarios._geometry(128, 2.0, (-128.0, -128.0, -106.0), deg)
    return b


def test_shifted_beam_composes_both_transforms(synth):
    """T'(g) = T(g - shift) on random points for gantryToImIdx and gantryToDoseIdx, within 8 * 2^-24 * max|index| (float32
    transforms: the two sides differ by a handful of roundings of numbers of the size of the index)."""
    rng = np.random.default_rng(0)
    for deg, shift in ((0.0, (3.0, 0.0, 0.0)), (30.0, (-2.5, 1.5, 4.0)), (90.0, (0.0, -3.0, 2.0))):
        b = _beam(synth, deg)
        s = robust.shifted_beam(b, shift)
        for name in ("gantryToImIdx", "gantryToDoseIdx"):
            T, Ts = getattr(b, name), getattr(s, name)
            assert Ts is not T
            worst = 0.0
            for _ in range(200):
                g = rng.uniform(-150.0, 150.0, 3).astype(np.float32)
                want = _apply32(T, (g - np.asarray(shift, dtype=np.float32)).astype(np.float32))
                got = _apply32(Ts, g)
                bound = 8 * 2.0 ** -24 * max(float(np.abs(want).max()), float(np.abs(got).max()))
                worst = max(worst, float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) / bound)
                assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= bound), (name, g, got, want)
            print("%s at %g degrees: largest difference %.3f of the bound" % (name, deg, worst))


def test_shifted_beam_shares_everything_else(synth):
    b = _beam(synth, 30.0)
    s = robust.shifted_beam(b, (3.0, 0.0, 0.0))
    assert s is not b
    for name in ("spotWeights", "beamEnergies", "spotSigmas", "spotIdxToGantry"):
        assert getattr(s, name) is getattr(b, name), name
    assert s.raySpacing == b.raySpacing and s.tracerSteps == b.tracerSteps and s.sourceDist == b.sourceDist
    assert set(vars(s)) == set(vars(b))
    assert np.array_equal(s.gantryToImIdx.m, b.gantryToImIdx.m) and np.array_equal(s.gantryToDoseIdx.m, b.gantryToDoseIdx.m)
    # the original is untouched, and a beam whose two transforms are one object keeps them one
    assert not np.array_equal(s.gantryToImIdx.v, b.gantryToImIdx.v)
    one = scenarios.make_field(synth, 96, 256.0 / 96, (-128.0, -128.0, -106.0), 0.0, 5, 8.0, 3, seed=3)
    assert one.gantryToDoseIdx is one.gantryToImIdx
    so = robust.shifted_beam(one, (0.0, 2.0, 0.0))
    assert so.gantryToDoseIdx is so.gantryToImIdx
    # scenario_beams: one list per shift, a zero shift gives the beams themselves
    lists = robust.scenario_beams([b, one], [(0, 0, 0), (3, 0, 0), (-3, 0, 0)])
    assert len(lists) == 3 and lists[0][0] is b and lists[0][1] is one and lists[1][0] is not b
    assert np.allclose(lists[1][0].gantryToImIdx.v + lists[2][0].gantryToImIdx.v, 2 * b.gantryToImIdx.v, atol=1e-9)


def test_range_scaled_luts_changes_the_stopping_power_table_only(synth):
    es = synth
    sc = robust.range_scaled_luts(es, 1.035)
    assert sc is not es and sc.spVector.dtype == np.float32 and sc.spVector.flags["C_CONTIGUOUS"]
    assert np.array_equal(sc.spVector, (es.spVector * np.float32(1.035)).astype(np.float32)) and not np.array_equal(sc.spVector, es.spVector)
    for k, v in vars(es).items():
        if k == "spVector":
            continue
        w = getattr(sc, k)
        assert w is v or w == v, k
    assert set(vars(sc)) == set(vars(es))
    same = robust.range_scaled_luts(es, 1.0)
    assert same.spVector.tobytes() == es.spVector.tobytes()
    a = sc.as_abi()
    assert a.n_sp_samples == es.nSpSamples and a.sp_scale_fact == es.as_abi().sp_scale_fact
