"""Grids of dose volumes: the affine map between the voxel indices of two grids, as Engine.resample_dose takes it, and the maps of
a deformable warp (Engine.warp_dose).

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


def _inverse(ms):
    """The inverse of an index-to-world matrix in float64: the adjugate over the determinant, as rtd_dicom::idxToIdx writes it (rows of
    the inverse = cross products of the columns' partners)."""
    det = float(np.dot(ms[0], np.cross(ms[1], ms[2])))
    if det == 0.0 or not np.isfinite(det):
        raise ValueError("the source grid's index-to-world matrix is singular")
    return np.stack([np.cross(ms[1], ms[2]), np.cross(ms[2], ms[0]), np.cross(ms[0], ms[1])], axis=1) / det


def index_map(dst_idx_to_world, src_idx_to_world):
    """The rtd_affine (abi.RtdAffine) that takes a voxel index of the destination grid to the voxel index of the source grid at the same
    place: inverse(src_idx_to_world) o dst_idx_to_world. Each transform: 4x4, or (M 3x3, v 3), float64, index (x, y, z) -> world mm."""
    md, vd = _parts(dst_idx_to_world)
    ms, vs = _parts(src_idx_to_world)
    inv = _inverse(ms)
    return abi.make_affine(inv @ md, inv @ (vd - vs))


def warp_maps(dst_idx_to_world, src_idx_to_world, dvf_idx_to_world):
    """The maps of an rtd_warp whose field holds displacements in world mm on a grid of its own -> (dst_idx_to_src_idx,
    dst_idx_to_dvf_idx, k): the two index maps as index_map makes them, and k, the linear part of inverse(src_idx_to_world) (3x3
    float32), which takes a displacement in mm to source-index units. Composed in float64, rounded to float32 once. The triple is what
    abi.make_warp takes in front of the field's device pointer and dims."""
    ms, _ = _parts(src_idx_to_world)
    return index_map(dst_idx_to_world, src_idx_to_world), index_map(dst_idx_to_world, dvf_idx_to_world), _inverse(ms).astype(np.float32)
