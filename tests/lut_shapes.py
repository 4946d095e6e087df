"""Look-up tables of other shapes than luts.synth_luts()'s default (147 energies x 1024 samples, three HU tables of 3072 entries,
scale factors 1 / 1 / 1000), for tests/test_lut_shapes_reference.py and tests/test_gpu_lut_shapes.py. A plain module like
asym_scenes.py: no tests, no fixtures. Every table is an EnergyStruct made of synth_luts arrays, built once per process.

What each shape is for (the engine's branches on the table sizes; a GPU test learns which side it took from
rtd_field_fetch "launch_builds", never from the byte counts here):

  rows_last_in_lds     40 x 6912   the two cumulative-IDD rows of a layer (2 x 4 x n_samples bytes) and the step table of a 512-step
                                   field (4 x 512 bytes) are 57 344 bytes together: the last size k_fill stages in LDS
  rows_first_global    40 x 6913   the first size whose rows k_fill reads from global memory
  rows_global          40 x 8192   global rows well clear of the edge; rows_global_nuclear: the same with the NUCLEAR_CORR tables
  rows_2049            40 x 2049   two rows of more than 4096 floats: the other side of fillTabOffset's branch, rows still in LDS
  hu_6048 / hu_6049    n_hu        density + stopping-power tables of 12 096 / 12 098 entries: the along-beam tracer's LDS limit
  hu_12672 / hu_12673  n_hu        25 344 / 25 346 entries: the diagonal tracer's LDS limit (and the tail loop of the tables' staging)
  mixed                            the default tables on other grids: density 6143 entries at scale 2, stopping power 1536 at 0.5,
                                   1/X0 1536 at 500: the density table longer than the other two, no scale factor of 1 or 1000

mixed describes the same physics as the default tables: the density and stopping-power tables are piecewise linear in HU + 1000 with
their knee at 1000, which both new grids (steps of 0.5 and of 2) contain, so the resampled tables interpolate to the same function;
the 1/X0 table has its knee at density 1 (entry 1000 of the default grid, entry 500 of the new one) and is weakly curved above it."""
import functools

import numpy as np

from raytracedicom_amd import luts

N_ENERGIES = 40
STEPS = 512                       # tracer steps of the scene below (make_field's default)

ROWS = {"rows_last_in_lds": 6912, "rows_first_global": 6913, "rows_global": 8192, "rows_2049": 2049}
HU = {"hu_6048": 6048, "hu_6049": 6049, "hu_12672": 12672, "hu_12673": 12673}
NAMES = tuple(ROWS) + ("rows_global_nuclear",) + tuple(HU) + ("mixed",)

MIXED = {"density": (6143, 2.0), "sp": (1536, 0.5), "rrl": (1536, 500.0)}     # (entries, scale factor)


def _resampled(vec, scale_old, n_new, scale_new):
    """A table sampled at index = x * scale_old, on the grid index = x * scale_new (linear interpolation in float64)."""
    x = np.arange(n_new, dtype=np.float64) / scale_new
    return np.interp(x * scale_old, np.arange(vec.size, dtype=np.float64), vec.astype(np.float64))


@functools.lru_cache(maxsize=None)
def default():
    return luts.synth_luts()


@functools.lru_cache(maxsize=None)
def _base(nuclear):
    return luts.synth_luts(n_energies=N_ENERGIES, nuclear=nuclear)


def _rows(n_samples, nuclear=False):
    """synth_luts(40 energies x 1024 samples) with every depth row resampled onto n_samples samples: sample j of the new row lies at
    the depth of sample j * 1024 / n_samples of the old one, so the rows' scale factors (samples per mm) grow by n_samples / 1024.
    (synth_luts itself builds long rows by a convolution whose cost grows with the square of their length: 20 s for 8192 samples.)"""
    b = _base(nuclear)
    old = np.arange(b.nEnergySamples, dtype=np.float64)
    at = np.arange(n_samples, dtype=np.float64) * (b.nEnergySamples / float(n_samples))

    def rows(m):
        return None if m is None else np.stack([np.interp(at, old, r.astype(np.float64)) for r in m])
    return luts.EnergyStruct(b.energiesPerU, b.peakDepths, b.scaleFacts.astype(np.float64) * (n_samples / float(b.nEnergySamples)), rows(b.ciddMatrix),
                             b.densityScaleFact, b.densityVector, b.spScaleFact, b.spVector, b.rRlScaleFact, b.rRlVector,
                             rows(b.nucWeightMatrix), rows(b.nucSqSigmaMatrix))


@functools.lru_cache(maxsize=None)
def table(name):
    """The EnergyStruct of one of NAMES."""
    if name in ROWS:
        return _rows(ROWS[name])
    if name == "rows_global_nuclear":
        return _rows(ROWS["rows_global"], nuclear=True)
    if name in HU:
        return luts.synth_luts(n_energies=N_ENERGIES, n_hu=HU[name])
    assert name == "mixed", name
    d = default()
    (nd, sd), (ns, ss), (nr, sr) = MIXED["density"], MIXED["sp"], MIXED["rrl"]
    return luts.EnergyStruct(d.energiesPerU, d.peakDepths, d.scaleFacts, d.ciddMatrix,
                             sd, _resampled(d.densityVector, d.densityScaleFact, nd, sd),
                             ss, _resampled(d.spVector, d.spScaleFact, ns, ss),
                             sr, _resampled(d.rRlVector, d.rRlScaleFact, nr, sr))


def scene(es, angle=15.0, **kw):
    """The scene of both test files: the 64^3 heterogeneous phantom, one field of 5 x 5 spots 6 mm apart, 3 layers, 512 steps
    (64 x 56 rays, radii up to 16 - 17)."""
    from gpu_support import hetero_scene
    return hetero_scene(es, 64, [angle], spots=5, pitch=6.0, layers=3, **kw)


def fill_lds_bytes(es, steps=STEPS):
    """Bytes of the fill's staged LUT rows and step table: two rows of n_samples floats, one float per step."""
    return 2 * 4 * es.nEnergySamples + 4 * steps


def trace_lut_entries(es):
    """Entries of the two tables every tracer kernel stages in LDS."""
    return es.nDensitySamples + es.nSpSamples
