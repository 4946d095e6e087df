"""CPU tests of tests/lut_shapes.py: every table runs through the oracle, the resampled tables describe the default physics, and
the sizes that make the tables what they are for are recomputed and printed."""
import numpy as np
import pytest

import lut_shapes as LS
from raytracedicom_amd import scenarios


def _oracle_dose(orc, scn):
    dose = np.zeros_like(scn.ct)
    of = orc.run_field(scn, scn.beams[0], dose, keep_layers=False)
    status, error = of.status, of.error
    of.close()
    return status, error, dose


@pytest.mark.parametrize("name", LS.NAMES)
def test_every_table_runs_through_the_oracle(orc, name):
    es = LS.table(name)
    status, error, dose = _oracle_dose(orc, LS.scene(es))
    assert status == 0, (status, error)
    assert np.isfinite(dose).all() and dose.max() > 0 and dose.min() >= 0, (float(dose.min()), float(dose.max()))


def test_mixed_describes_the_default_physics(orc):
    """The oracle's dose under `mixed` against its dose under the default tables, relative, above 1e-3 of the maximum. The bound of
    5e-4 is the one the tables were specified with: four times the 1.12e-4 measured for them then (the float32 rounding of the
    table positions hu * scale and of the resampled entries). This module's resampling, in float64 and rounded once, gives 1.6e-5;
    the value found is printed, so a later change of the tables shows up."""
    scn = LS.scene(LS.default())
    mixed = scenarios.Scenario("mixed", LS.table("mixed"), scn.ct, scn.spacing, scn.beams)
    (s0, e0, d0), (s1, e1, d1) = _oracle_dose(orc, scn), _oracle_dose(orc, mixed)
    assert s0 == 0 and s1 == 0, (e0, e1)
    big = d0 > 1e-3 * d0.max()
    rel = float((np.abs(d1.astype(np.float64) - d0)[big] / d0[big]).max())
    print("mixed against the default tables: max relative difference %.3g over %d voxels above 1e-3 of the maximum" % (rel, int(big.sum())))
    assert big.sum() > 1000
    assert rel <= 5e-4, rel
    es = LS.table("mixed")
    d = LS.default()
    assert es.nDensitySamples != es.nSpSamples and es.nDensitySamples != es.nRRlSamples
    assert (es.nDensitySamples, es.nSpSamples, es.nRRlSamples) == (6143, 1536, 1536) and d.nDensitySamples == d.nSpSamples == d.nRRlSamples == 3072
    assert (es.densityScaleFact, es.spScaleFact, es.rRlScaleFact) == (2.0, 0.5, 500.0)


def test_the_shapes_document_themselves():
    """The byte and entry counts of the module's docstring, from n_samples, 512 steps and n_hu. (The GPU tests do not rely on them:
    they ask the engine which build it launched.)"""
    fill = {n: LS.fill_lds_bytes(LS.table(n)) for n in LS.ROWS}
    trace = {n: LS.trace_lut_entries(LS.table(n)) for n in tuple(LS.HU) + ("mixed",)}
    for n, b in fill.items():
        print("%-18s %d energies x %5d samples: rows %6d B + step table %d B = %6d B" % (
            n, LS.table(n).nEnergies, LS.table(n).nEnergySamples, 8 * LS.table(n).nEnergySamples, 4 * LS.STEPS, b))
    for n, e in trace.items():
        print("%-18s density %5d + stopping power %5d = %5d entries, %6d B" % (n, LS.table(n).nDensitySamples, LS.table(n).nSpSamples, e, 4 * e))
    assert fill == {"rows_last_in_lds": 57344, "rows_first_global": 57352, "rows_global": 67584, "rows_2049": 18440}
    assert fill["rows_last_in_lds"] == 56 * 1024 and 2 * LS.table("rows_2049").nEnergySamples > 4096
    assert trace == {"hu_6048": 12096, "hu_6049": 12098, "hu_12672": 25344, "hu_12673": 25346, "mixed": 6143 + 1536}
    nuc = LS.table("rows_global_nuclear")
    assert nuc.nucWeightMatrix.shape == nuc.nucSqSigmaMatrix.shape == nuc.ciddMatrix.shape == (LS.N_ENERGIES, 8192)
    np.testing.assert_array_equal(nuc.ciddMatrix, LS.table("rows_global").ciddMatrix)
