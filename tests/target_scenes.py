"""Fields and targets for the tests of the spot selection (a plain module, no tests): the geometry of a scene of tests/asym_scenes.py
with a spot map worth selecting from — 9 x 7 spots at 7 x 5 mm pitch with the scene's spot offset, 8 layers from 70 to 125 MeV/u,
ray-weight cut-off 0 — and an ellipsoid target of 16 x 11 x 13 mm semi-axes (world x, y, z) in the middle of the field."""
import numpy as np

import asym_scenes as S
import target_reference as T
from raytracedicom_amd import scenarios

SEMI_AXES = (16.0, 11.0, 13.0)
MARGINS = ((0.0, 0.0, 0.0), (6.0, 2.0, 5.0))     # (lateral, proximal, distal) mm


def scene(luts, name):
    """Scene `name` of asym_scenes with the candidate beam below as its one beam."""
    scn = S.scene(luts, name)
    b = scn.beams[0]
    energies, sigmas = scenarios.water_cube_energies(luts, 8, e0=70.0, e1=125.0)
    scn.beams = [b.replace(spotWeights=np.ones((8, 7, 9), dtype=np.float32), beamEnergies=energies, spotSigmas=sigmas)]
    return scn


def options():
    return S.options(cutoff=0.0)


def world_of(scn, p):
    """World mm of dose-grid coordinates p = (px, py, pz)."""
    return tuple(float(scn.dose_origin[c]) + float(p[c]) * float(scn.dose_spacing[c]) for c in range(3))


def central_point(scn, g, wepl, peaks):
    """The world point of the central ray (W / 2, H / 2) at the first step whose wepl reaches the mean of peak depths 2 and 5."""
    i, j = g.W // 2, g.H // 2
    depth = 0.5 * (float(peaks[2]) + float(peaks[5]))
    col = np.asarray(wepl).reshape(g.S, g.H, g.W)[:, j, i]
    k = int((col < depth).sum())
    assert k < g.S, "the central ray never reaches %g mm" % depth
    p = T.dose_index(g, np.float32(i), np.float32(j), np.float32(k))
    return world_of(scn, p)


def ellipsoid(scn, centre, semi_axes=SEMI_AXES):
    """uint8 [Z][Y][X] mask of the dose grid: voxel centres inside the ellipsoid."""
    nx, ny, nz = scn.dose_dims
    x = (scn.dose_origin[0] + scn.dose_spacing[0] * np.arange(nx))[None, None, :]
    y = (scn.dose_origin[1] + scn.dose_spacing[1] * np.arange(ny))[None, :, None]
    z = (scn.dose_origin[2] + scn.dose_spacing[2] * np.arange(nz))[:, None, None]
    r = ((x - centre[0]) / semi_axes[0]) ** 2 + ((y - centre[1]) / semi_axes[1]) ** 2 + ((z - centre[2]) / semi_axes[2]) ** 2
    return (r <= 1.0).astype(np.uint8)


def target(scn, g, wepl, peaks):
    """The scene's target. B: the ellipsoid is moved along world z until its centre lies on the last slice of the fine grid, so that
    the grid cuts it in half and the rays that cross the missing half have samples in it that fall outside the grid."""
    c = central_point(scn, g, wepl, peaks)
    if scn.name == "B":
        c = (c[0], c[1], scn.dose_origin[2] + scn.dose_spacing[2] * (scn.dose_dims[2] - 1))
    return ellipsoid(scn, c)


def two_slabs(scn, g, wepl, peaks, half_gap=8.0):
    """A hollow target for the scenes whose beam runs along world x (C, U): a 30 x 15 x 15 mm ellipsoid around the central point
    without the voxels within half_gap mm of its centre plane x = const — two parts, one behind the other along every ray."""
    c = central_point(scn, g, wepl, peaks)
    m = ellipsoid(scn, c, (30.0, 15.0, 15.0))
    x = scn.dose_origin[0] + scn.dose_spacing[0] * np.arange(scn.dose_dims[0])
    m[:, :, np.abs(x - c[0]) < half_gap] = 0
    return m


def with_last_energy(luts, beam, energy):
    """`beam` with the energy of its last layer replaced (and that layer's spot sigmas by the water cube's rule)."""
    energies = beam.beamEnergies.copy()
    energies[-1] = energy
    sigmas = beam.spotSigmas.copy()
    sigmas[-1] = scenarios.water_cube_energies(luts, 1, e0=energy)[1][0]
    return beam.replace(beamEnergies=energies, spotSigmas=sigmas)
