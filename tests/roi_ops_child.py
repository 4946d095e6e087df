"""Run by tests/test_gpu_roi_ops.py in a child process (RTD_ROI_MARGIN_NAIVE is read when a handle is created, from the process
environment): the mid-sized margin case below on the device, the voxel lists written to the .npz named on the command line. A plain
module (no tests)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

DIMS = (200, 180, 60)                      # (x, y, z)
SPACING = (1.0, 1.0, 1.0)
# a 12-voxel table on five sides and a 7-voxel one on the sixth; (name, margins, contract)
CASES = (("expand", (12.0, 12.0, 12.0, 12.0, 12.0, 7.0), 0), ("contract", (12.0, 12.0, 12.0, 12.0, 12.0, 7.0), 1))


def mid_mask():
    """Two ellipsoids joined by a thin bar, a cavity in the larger one, and seeded specks; it touches the faces x = 0 and z = nz - 1."""
    nx, ny, nz = DIMS
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    big = ((x - 60) / 62.0) ** 2 + ((y - 90) / 70.0) ** 2 + ((z - 40) / 30.0) ** 2 <= 1.0
    cavity = ((x - 70) / 9.0) ** 2 + ((y - 95) / 11.0) ** 2 + ((z - 35) / 6.0) ** 2 <= 1.0
    small = ((x - 165) / 20.0) ** 2 + ((y - 60) / 25.0) ** 2 + ((z - 20) / 14.0) ** 2 <= 1.0
    bar = (np.abs(y - 75) <= 1) & (np.abs(z - 25) <= 1) & (x >= 100) & (x <= 160)
    specks = np.random.default_rng(41).random((nz, ny, nx)) < 2e-5
    return (big & ~cavity) | small | bar | specks


def upload(eng, mask):
    """The Roi of a [Z][Y][X] mask: the bytes go to the device, rtd_roi_from_mask reads them."""
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    d = eng.device_alloc(m.size)
    try:
        eng.to_device(d, m)
        return eng.roi_from_mask(d, (m.shape[2], m.shape[1], m.shape[0]))
    finally:
        eng.device_free(d)


def run(eng):
    """name -> the voxel list of the case."""
    src = upload(eng, mid_mask())
    out = {}
    for name, margins, contract in CASES:
        r = src.contract(margins, SPACING) if contract else src.expand(margins, SPACING)
        out[name] = r.voxels()
        r.close()
    src.close()
    return out


def main(path):
    from raytracedicom_amd import engine
    with engine.Engine(0) as eng:
        np.savez(path, **run(eng))


if __name__ == "__main__":
    main(sys.argv[1])
