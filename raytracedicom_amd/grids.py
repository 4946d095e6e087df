"""Grids of dose volumes: the affine map between the voxel indices of two grids, as Engine.resample_dose takes it.

Mirrors rtd_dicom::idxToIdx (include/rtd_dicom.hpp): composed in float64 from the two index-to-world transforms, rounded to float32 once.
"""
import numpy as np

from . import abi


def _parts(t):
    """(M, v) in float64 from a 4x4 matrix or an (M, v) pair."""
    if isinstance(t, (tuple, list)) and len(t) == 2:
        m, v = np.asarray(t[0], dtype=np.float64).reshape(3, 3), np.asarray(t[1], dtype=np.float64).reshape(3)
        return m, v
    a = np.asarray(t, dtype=np.float64)
    if a.shape != (4, 4):
        raise ValueError("an index-to-world transform is a 4x4 matrix or an (M, v) pair")
    return a[:3, :3].copy(), a[:3, 3].copy()


def index_map(dst_idx_to_world, src_idx_to_world):
    """The rtd_affine (abi.RtdAffine) that takes a voxel index of the destination grid to the voxel index of the source grid at the same
    place: inverse(src_idx_to_world) o dst_idx_to_world. Each transform: 4x4, or (M 3x3, v 3), float64, index (x, y, z) -> world mm."""
    md, vd = _parts(dst_idx_to_world)
    ms, vs = _parts(src_idx_to_world)
    det = float(np.dot(ms[0], np.cross(ms[1], ms[2])))
    if det == 0.0 or not np.isfinite(det):
        raise ValueError("the source grid's index-to-world matrix is singular")
    # the adjugate over the determinant, as rtd_dicom::idxToIdx writes it: rows of the inverse = cross products of the columns' partners
    inv = np.stack([np.cross(ms[1], ms[2]), np.cross(ms[2], ms[0]), np.cross(ms[0], ms[1])], axis=1) / det
    return abi.make_affine(inv @ md, inv @ (vd - vs))
