"""k_superpose_sweep's weight-table build on the waves it treats apart (rtd_sweep.hpp swBuildT): erf lanes (1/sigma > 0.75) beside
series lanes in one wave, erf lanes whose entries stop at 5, and lanes whose own batch radius is below their wave's. Shallow steps of
a heterogeneous field with coarse rays (1.5 mm: sharp sources) and fine ones (0.75 mm: radii up to 21, the row |dy| = 16 and the second
launch). The sweep against k_superpose_mfma (RTD_NO_SWEEP), which builds its tables its own way: BEV doses within 1e-5 of each other
relative to the maximum region, identical support, both within the parity bar of the oracle."""
import numpy as np
import pytest

from raytracedicom_amd import scenarios
from analysis_sweep_waves import wave_stats

pytestmark = pytest.mark.gpu


def _rel_close(a, b, rtol, floor_frac=1e-3, atol_frac=1e-6):
    a = a.astype(np.float64); b = b.astype(np.float64)
    mx = np.abs(b).max()
    mask = np.abs(b) > floor_frac * mx
    err = np.abs(a - b)
    assert (err[mask] <= rtol * np.abs(b[mask]) + atol_frac * mx).all(), "max rel err %g" % (err[mask] / np.abs(b[mask])).max()
    assert (err[~mask] <= 2 * rtol * floor_frac * mx + atol_frac * mx).all()


def _run(engine, scn, beam):
    eng = engine.Engine(0)
    eng.set_luts(scn.luts)
    eng.set_ct(scn.ct)
    n = scn.n_voxels
    d = eng.device_alloc(4 * n)
    eng.device_zero(d, 4 * n)
    fld = eng.create_field(beam, scn.dims)
    try:
        fld.compute(d)
        _, info = fld.finish()
        dose = np.empty_like(scn.ct)
        eng.to_host(dose, d)
        return fld.fetch("bev").copy(), dose, info
    finally:
        fld.destroy(); eng.device_free(d); eng.close()


@pytest.mark.parametrize("spacing", [(1.5, 1.5), (0.75, 0.75)])
def test_sweep_tables_on_mixed_and_short_waves(orc, engine, synth, monkeypatch, spacing):
    ct, voxel = scenarios.hetero_phantom(96)
    beam = scenarios.make_field(synth, 96, 256.0 / 96, (-128.0, -128.0, -106.0), 20.0, 5, 6.0, 6, 11, (1900.0, 2300.0), 200,
                                ray_spacing=spacing, weight_lo=400.0)
    scn = scenarios.Scenario("rays %g mm" % spacing[0], synth, ct, (voxel,) * 3, [beam])
    ref = np.zeros_like(ct)
    of = orc.run_field(scn, beam, ref, keep_layers=True)
    W, H, L = of.info["ray_dims"]
    st = wave_stats(of, beam)
    if spacing[0] > 1.0:
        assert st["mixed"] > 0 and st["short"] > st["short_series_only"] > 0, st       # erf beside series; short erf and series lanes
    else:
        assert st["rho16"] > 0 and st["short_series_only"] > 0 and of.info["max_radius"] > 16, (st, of.info["max_radius"])
    res = {}
    for name, env in (("sweep", None), ("mfma", "1")):
        if env is None:
            monkeypatch.delenv("RTD_NO_SWEEP", raising=False)
        else:
            monkeypatch.setenv("RTD_NO_SWEEP", env)
        bev, dose, info = _run(engine, scn, beam)
        res[name] = (bev.reshape(-1, H + 64, W + 64), dose)
    monkeypatch.delenv("RTD_NO_SWEEP", raising=False)
    (bs, ds), (bm, dm) = res["sweep"], res["mfma"]
    obev = of.get("bev").reshape(-1, H + 64, W + 64)
    big = obev > 1e-3 * obev.max()
    assert (np.abs(bs.astype(np.float64) - bm)[big] / obev[big]).max() <= 1e-5
    k0 = of.info["beam_first_inside"]
    np.testing.assert_array_equal(bs[k0:] == 0, bm[k0:] == 0)
    for b in (bs, bm):
        _rel_close(b, obev, rtol=1e-4)
    _rel_close(ds, ref, rtol=1e-4)
    _rel_close(dm, ref, rtol=1e-4)
