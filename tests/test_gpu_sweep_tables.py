"""k_superpose_sweep's weight-table build on the waves it treats apart (rtd_sweep.hpp swBuildT): erf lanes (1/sigma > 0.75) beside
series lanes in one wave, erf lanes whose entries stop at 5, and lanes whose own batch radius is below their wave's. Shallow steps of
a heterogeneous field with coarse rays (1.5 mm: sharp sources) and fine ones (0.75 mm: radii up to 21, the row |dy| = 16 and the second
launch). The sweep against k_superpose_mfma (RTD_NO_SWEEP), which builds its tables its own way: BEV doses within 1e-5 of each other
relative to the maximum region, identical support, both within the parity bar of the oracle."""
import numpy as np
import pytest

from analysis_sweep_waves import wave_stats
from gpu_support import FieldRig, rel_close, rig_fixture
from raytracedicom_amd import scenarios

pytestmark = pytest.mark.gpu

rig_of = rig_fixture(FieldRig)


@pytest.mark.parametrize("spacing", [(1.5, 1.5), (0.75, 0.75)])
def test_sweep_tables_on_mixed_and_short_waves(orc, rig_of, synth, spacing):
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
        rig = rig_of(scn, None)
        fld = rig.field(beam, RTD_NO_SWEEP=env)
        dose, _, _ = rig.compute(fld)
        res[name] = (fld.fetch("bev").reshape(-1, H + 64, W + 64).copy(), dose)
    (bs, ds), (bm, dm) = res["sweep"], res["mfma"]
    obev = of.get("bev").reshape(-1, H + 64, W + 64)
    big = obev > 1e-3 * obev.max()
    assert (np.abs(bs.astype(np.float64) - bm)[big] / obev[big]).max() <= 1e-5
    k0 = of.info["beam_first_inside"]
    np.testing.assert_array_equal(bs[k0:] == 0, bm[k0:] == 0)
    for b in (bs, bm):
        rel_close(b, obev, rtol=1e-4)
    rel_close(ds, ref, rtol=1e-4)
    rel_close(dm, ref, rtol=1e-4)
