"""The scenes of tests/asym_scenes.py on the CPU oracle alone (no GPU).

Two things are pinned here so that the GPU comparisons of tests/test_gpu_asym_grids.py cannot pass over nothing:
  * the conditions on the inputs: every scene deposits dose, on a good part of its dose grid and up to a face of it where stated, with
    six pairwise different dims, rays on both sides of the weight cut-off, radii above 16 in F, one sigma per slice in U only;
  * the oracle's own handling of a dose grid that is not the CT grid, oracle against oracle (test_lattice_grid_samples_the_ct_grid_dose).
"""
import numpy as np
import pytest

import asym_scenes as S


@pytest.fixture(scope="module")
def nuc_luts():
    from raytracedicom_amd import luts
    return luts.synth_luts(nuclear=True)


@pytest.fixture(scope="module")
def runs(orc, synth, nuc_luts):
    """name -> (scene, oracle field, dose), each scene run once."""
    cache = {}

    def get(name, grid=None):
        key = (name, grid)
        if key not in cache:
            scn = S.scene(nuc_luts if name == "N" else synth, name, grid)
            dose = np.zeros(scn.dose_shape, dtype=np.float32)
            of = orc.run_field(scn, scn.beams[0], dose, options=S.options(name), keep_layers=True, dose_dims=scn.dose_dims)
            cache[key] = (scn, of, dose)
        return cache[key]
    return get


@pytest.mark.parametrize("name", S.NAMES)
def test_scene_is_exercised(runs, name):
    scn, of, dose = runs(name)
    assert of.status == 0, of.error
    mx = float(dose.max())
    assert mx > 0
    assert (dose > 1e-3 * mx).mean() >= 0.03
    dims = list(scn.dims) + list(scn.dose_dims)
    assert len(set(dims)) == 6, dims                                  # CT dims, dose dims: all six pairwise different
    assert scn.dose_shape == dose.shape and scn.ct.shape == (scn.dims[2], scn.dims[1], scn.dims[0])
    b = scn.beams[0]
    assert not np.array_equal(b.gantryToImIdx.m, b.gantryToDoseIdx.m) and not np.array_equal(b.gantryToImIdx.v, b.gantryToDoseIdx.v)
    assert len(set(scn.spacing)) == 3 and len(set(scn.dose_spacing)) == 3
    assert np.all(b.spotSigmas[:, 1] > 1.3 * b.spotSigmas[:, 0])      # sigma_y is not sigma_x
    rw = of.get("ray_weights")
    cut = S.options(name).ray_weight_cutoff
    assert (rw >= cut).any() and (rw < cut).any()                     # live and dead rays


@pytest.mark.parametrize("name,want", [("A", ("z1",)), ("B", ("z0", "z1")), ("C", ("x1",)), ("D", ("y0", "y1"))])
def test_dose_reaches_a_face_of_the_dose_grid(runs, name, want):
    _, _, dose = runs(name)
    hit = tuple(k for k, v in S.faces(dose).items() if v.max() > 1e-3 * dose.max())
    assert hit == want, hit


def test_f_has_radii_above_16(runs):
    _, of, _ = runs("F")
    assert of.info["max_radius"] > 16
    assert S.tiles_above(of, 16) > 0
    assert of.info["ray_dims"] == [160, 88, 3]


@pytest.mark.parametrize("name", [n for n in S.NAMES if n != "N"])
def test_one_sigma_per_slice_in_u_only(runs, name):
    """rtd_field_info.uniform_sigma is the engine's finding (the oracle has one superposition and does not report it); what it follows
    from is visible in the oracle's 1/sigma: U (a parallel beam square onto a face of the water box) has one value per depositing slice,
    bit for bit; the heterogeneous scenes have not, and neither has W — A's oblique divergent beam enters the water box through
    slanted faces, ray by ray at another step, so water alone does not make its slices uniform."""
    _, of, _ = runs(name)
    n, bad = S.nonuniform_slices(of)
    assert n > 100
    if name == "U":
        assert bad == 0
    else:
        assert bad > n // 2, (n, bad)


# measured here, oracle against oracle (maximum relative deviation on voxels above 1e-3 of the maximum; below it, relative to the maximum)
LATTICE_MEASURED = {"A": 5.97e-5, "C": 1.28e-5}
LATTICE_FLOOR_MEASURED = {"A": 4.8e-8, "C": 1.3e-8}


@pytest.mark.parametrize("name", ["A", "C"])
def test_lattice_grid_samples_the_ct_grid_dose(runs, name):
    """The transfer point-samples the BEV dose at voxel centres, so the dose on the lattice grid (every voxel centre of it a CT voxel
    centre: strides 2, 1, 3, offsets 3, 5, 4) equals the dose on the CT's own grid at [4::3, 5::1, 3::2]. The two runs differ only in
    gantryToDoseIdx: two float32 affines that take the same world point to the BEV through differently rounded coefficients, so the
    sampling positions differ by some 1e-5 of a ray pixel and the interpolated dose by that times its relative slope. Measured:
    5.97e-5 (A) and 1.28e-5 (C) on the voxels above 1e-3 of the maximum, 4.8e-8 (A) and 1.3e-8 (C) of the maximum below. Asserted: 3 x the measured
    value; the margin covers a re-seeding of the phantom noise, not an error — a wrong stride, offset or axis is an error of order 1.

    The integral: sum(dose) x voxel volume on the coarse grid is at most that on the CT's grid (which contains it) and within 10 %
    of it — what is missing is cut off by the coarse grid's z1 / x1 face (A: 0.04096 against 0.04225)."""
    _, _, d_lat = runs(name, "lattice")
    scn_ct, _, d_ct = runs(name, "ct")
    ref = S.lattice_of(d_ct).astype(np.float64)
    assert ref.shape == d_lat.shape
    mx = ref.max()
    big = ref > 1e-3 * mx
    assert big.sum() > 1000
    err = np.abs(d_lat.astype(np.float64) - ref)
    rel = float((err[big] / ref[big]).max())
    low = float(err[~big].max() / mx)
    print("scene %s: lattice against the CT grid: max rel %.3g above the floor, %.3g of the maximum below" % (name, rel, low))
    assert rel <= 3.0 * LATTICE_MEASURED[name], rel
    assert low <= 3.0 * LATTICE_FLOOR_MEASURED[name], low
    scn, _, d_coarse = runs(name)
    i_coarse = float(d_coarse.astype(np.float64).sum() * np.prod(scn.dose_spacing))
    i_ct = float(d_ct.astype(np.float64).sum() * np.prod(scn_ct.dose_spacing))
    print("scene %s: integral %.5g on the coarse grid, %.5g on the CT grid" % (name, i_coarse, i_ct))
    assert 0.9 * i_ct <= i_coarse <= i_ct


def test_beam_settings_replace(synth):
    """BeamSettings.replace changes the named field and keeps the other eight; the new beam goes through __init__ again (the shape
    assertion fires on a weight array of another layer count); a name that is no constructor field is a TypeError."""
    b = S.scene(synth, "A").beams[0]
    w = np.full(b.spotWeights.shape, 2.0)                             # float64: converted like a constructor argument
    c = b.replace(spotWeights=w)
    assert c is not b and c.spotWeights.dtype == np.float32 and np.array_equal(c.spotWeights, w)
    assert not np.array_equal(b.spotWeights, w)                       # the original is untouched
    for k in ("beamEnergies", "spotIdxToGantry", "gantryToImIdx", "gantryToDoseIdx"):
        assert getattr(c, k) is getattr(b, k), k
    assert np.shares_memory(c.spotSigmas, b.spotSigmas) and c.spotSigmas.shape == b.spotSigmas.shape
    assert (c.raySpacing, c.tracerSteps, c.sourceDist) == (b.raySpacing, b.tracerSteps, b.sourceDist)
    t = object()
    assert b.replace(gantryToDoseIdx=t).gantryToDoseIdx is t and b.replace().spotWeights is b.spotWeights
    with pytest.raises(AssertionError):
        b.replace(spotWeights=np.ones((b.spotWeights.shape[0] + 1,) + b.spotWeights.shape[1:]))
    with pytest.raises(TypeError):
        b.replace(spotWeight=w)
