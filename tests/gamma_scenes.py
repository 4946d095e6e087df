"""Dose pairs for the gamma-index tests (tests/test_gamma_reference.py, tests/test_gpu_gamma.py): a Gaussian blob as the reference
and a noisy copy of it as the evaluated dose. A plain module (no tests, no plugin).

Every parity scene has at least 1000 evaluated voxels and a pass rate between 0.05 and 0.95 by the CPU oracle at threshold 0.10
(tests/test_gamma_reference.py asserts it), so that no comparison passes on an all-pass or all-fail volume."""
import collections

import numpy as np

Scene = collections.namedtuple("Scene", "name seed dims_zyx spacing dd dta amp")

# The brick of the search kernel is 32 x 4 x 4 voxels (x, y, z).
SCENES = (
    Scene("aniso", 7, (23, 29, 37), (1.0, 1.5, 2.5), 0.02, 2.0, 0.10),        # radii 3, 2, 2; every dim odd and no multiple of the brick
    Scene("iso2mm", 7, (15, 18, 21), (2.0, 2.0, 2.0), 0.02, 2.0, 0.08),       # radii 2, 2, 2
    Scene("thin", 7, (5, 40, 70), (1.0, 1.0, 3.0), 0.03, 3.0, 0.60),          # radii 5, 5, 2; nz barely above one brick
    Scene("bricks", 7, (9, 10, 67), (1.0, 3.0, 3.0), 0.02, 2.0, 0.10),        # three bricks on every axis; radii 3, 1, 1
    Scene("flat", 7, (1, 45, 50), (1.0, 1.0, 2.0), 0.02, 2.0, 0.10),          # nz = 1; radii 3, 3, 2
)


def by_name(name):
    for s in SCENES:
        if s.name == name:
            return s
    raise KeyError(name)


def scene(seed, dims_zyx, sp_xyz, amp):
    """ref: 2.0 * exp(-r^2 / (2 * 12^2)), r in mm from the centre at (0.45, 0.55, 0.5) of the extent n * spacing (x, y, z), node i at i * spacing; ev: ref with
    multiplicative Gaussian noise of relative amplitude amp. Both float32 [Z][Y][X]."""
    nz, ny, nx = dims_zyx
    rng = np.random.default_rng(seed)
    x = np.arange(nx, dtype=np.float64) * sp_xyz[0] - 0.45 * nx * sp_xyz[0]
    y = np.arange(ny, dtype=np.float64) * sp_xyz[1] - 0.55 * ny * sp_xyz[1]
    z = np.arange(nz, dtype=np.float64) * sp_xyz[2] - 0.50 * nz * sp_xyz[2]
    r2 = z[:, None, None] ** 2 + y[None, :, None] ** 2 + x[None, None, :] ** 2
    ref = (2.0 * np.exp(-r2 / (2.0 * 12.0 ** 2))).astype(np.float32)
    ev = (ref * (1 + amp * rng.standard_normal(ref.shape))).astype(np.float32)
    return ref, ev


def pair(s):
    return scene(s.seed, s.dims_zyx, s.spacing, s.amp)
