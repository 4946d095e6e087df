"""The rule of include/rtd.h "Spots from a target", restated in numpy (a plain module, no tests): rtd_field_project_target and
rtd_field_select_spots from arrays. Every float operation is a float32 numpy operation in the header's order, so the results are
meant to equal the engine's bit for bit.

Inputs: wepl [S][H][W] float32 (rtd_field_fetch "wepl"), peak depths [L] float32 ("layer_plan" column 2), a Geometry (the scalars
of rtd_field_info and of the beam) and the mask [Z][Y][X] of the dose grid."""
import numpy as np

F = np.float32


class Geometry:
    """ray_dims (W, H), ray_res, ray_offset (3 each, float32: rtd_field_info), source_dist (2), gantry_to_dose (m 9, v 3), the spot map
    (nx, ny) with spot_delta / spot_offset (spot_idx_to_gantry), steps S."""

    def __init__(self, ray_dims, ray_res, ray_offset, source_dist, m, v, spot_dims, spot_delta, spot_offset, steps):
        self.W, self.H = int(ray_dims[0]), int(ray_dims[1])
        self.ray_res = np.asarray(ray_res, dtype=F)
        self.ray_offset = np.asarray(ray_offset, dtype=F)
        self.source_dist = np.asarray(source_dist, dtype=F)
        self.m = np.asarray(m, dtype=F).reshape(9)
        self.v = np.asarray(v, dtype=F).reshape(3)
        self.spot_nx, self.spot_ny = int(spot_dims[0]), int(spot_dims[1])
        self.spot_delta = np.asarray(spot_delta, dtype=F)
        self.spot_offset = np.asarray(spot_offset, dtype=F)
        self.S = int(steps)


def geometry_of(info, beam):
    """From a field info dict (engine Field.finish()[1] or oracle OracleField.info) and its scenarios.BeamSettings."""
    sw = np.asarray(beam.spotWeights)
    return Geometry(info["ray_dims"][:2], info["ray_res"], info["ray_offset"], beam.sourceDist, beam.gantryToDoseIdx.m, beam.gantryToDoseIdx.v,
                    (sw.shape[2], sw.shape[1]), beam.spotIdxToGantry.delta, beam.spotIdxToGantry.offset, beam.tracerSteps)


def dose_index(g, i, j, k):
    """(a): the float32 dose-grid coordinates (px, py, pz) of ray-grid points; i, j, k broadcastable float32 arrays."""
    with np.errstate(all="ignore"):
        gx = i * g.ray_res[0] + g.ray_offset[0]
        gy = j * g.ray_res[1] + g.ray_offset[1]
        gz = k * g.ray_res[2] + g.ray_offset[2]
        gx = gx * (F(1.0) - gz / g.source_dist[0])
        gy = gy * (F(1.0) - gz / g.source_dist[1])
        m, v = g.m, g.v
        return tuple(((m[3 * c] * gx + m[3 * c + 1] * gy) + m[3 * c + 2] * gz) + v[c] for c in range(3))


def nearest_voxel(g, dims):
    """(a): (q, in_grid) — the nearest-voxel coordinates (three float32 arrays) of every sample and the bool array [S][H][W] of the
    samples whose nearest voxel lies in the grid dims = (nx, ny, nz)."""
    nx, ny, nz = dims
    i = np.arange(g.W, dtype=F)[None, None, :]
    j = np.arange(g.H, dtype=F)[None, :, None]
    k = np.arange(g.S, dtype=F)[:, None, None]
    p = dose_index(g, i, j, k)
    assert all(c.dtype == F for c in p)
    with np.errstate(all="ignore"):
        q = [np.broadcast_to(np.floor(c + F(0.5)), (g.S, g.H, g.W)) for c in p]
        ok = (q[0] >= F(0)) & (q[0] < F(nx)) & (q[1] >= F(0)) & (q[1] < F(ny)) & (q[2] >= F(0)) & (q[2] < F(nz))
    return q, ok


def project(g, mask):
    """(a): the inside samples as a bool array [S][H][W]."""
    mask = np.asarray(mask)
    nz, ny, nx = mask.shape
    q, ok = nearest_voxel(g, (nx, ny, nz))
    qi = [np.where(ok, c, F(0)).astype(np.int64) for c in q]
    return ok & (mask[qi[2], qi[1], qi[0]] != 0)


def pack(inside):
    """The packed layout: uint32 [ceil(S / 32)][H][W], bit k & 31 of word k >> 5."""
    S, H, W = inside.shape
    out = np.zeros(((S + 31) // 32, H, W), dtype=np.uint32)
    for k in range(S):
        out[k >> 5] |= inside[k].astype(np.uint32) << np.uint32(k & 31)
    return out


def summary(inside, wepl):
    """(b) as the dict Field.project_target returns."""
    n = int(inside.sum())
    if n == 0:
        return {"n_samples": 0, "wepl_min": 0.0, "wepl_max": 0.0, "ray_lo": [0, 0], "ray_hi": [0, 0], "step_lo": 0, "step_hi": 0}
    w = wepl[inside]
    ks, js, is_ = np.nonzero(inside)
    return {"n_samples": n, "wepl_min": float(w.min()), "wepl_max": float(w.max()), "ray_lo": [int(is_.min()), int(js.min())],
            "ray_hi": [int(is_.max()), int(js.max())], "step_lo": int(ks.min()), "step_hi": int(ks.max())}


def hits(inside, wepl, peaks, proximal=0.0, distal=0.0):
    """(c): uint8 [L][H][W]."""
    S = inside.shape[0]
    wepl = np.asarray(wepl, dtype=F)
    # target samples among the steps 0 .. k - 1, so that a range [kLo, kHi] holds one iff cum[kHi + 1] > cum[kLo]
    cum = np.concatenate([np.zeros((1,) + inside.shape[1:], dtype=np.int64), np.cumsum(inside, axis=0, dtype=np.int64)], axis=0)
    out = np.zeros((len(peaks),) + inside.shape[1:], dtype=np.uint8)
    for l, peak in enumerate(np.asarray(peaks, dtype=F)):
        lo, hi = peak - F(distal), peak + F(proximal)
        k_lo = (wepl < lo).sum(axis=0)
        k_hi = np.minimum((wepl < hi).sum(axis=0), S - 1)
        reach = k_lo < S
        a = np.minimum(k_lo, S - 1)
        got = np.take_along_axis(cum, (k_hi + 1)[None], axis=0)[0] > np.take_along_axis(cum, a[None], axis=0)[0]
        out[l] = (reach & got).astype(np.uint8)
    return out


def spot_rays(g, sx, sy, lateral=0.0):
    """(d): the ray set of spot (sx, sy) as a bool array [H][W]."""
    cx = (g.spot_offset[0] - g.ray_offset[0]) / g.ray_res[0] + F(sx) * (g.spot_delta[0] / g.ray_res[0])
    cy = (g.spot_offset[1] - g.ray_offset[1]) / g.ray_res[1] + F(sy) * (g.spot_delta[1] / g.ray_res[1])
    assert cx.dtype == F and cy.dtype == F
    rays = np.zeros((g.H, g.W), dtype=bool)
    near_x, near_y = np.floor(cx + F(0.5)), np.floor(cy + F(0.5))
    if F(0) <= near_x < F(g.W) and F(0) <= near_y < F(g.H):
        rays[int(near_y), int(near_x)] = True
    m = F(lateral)
    if m > F(0):
        with np.errstate(over="ignore"):
            dx = (np.arange(g.W, dtype=F) - cx) * g.ray_res[0]
            dy = (np.arange(g.H, dtype=F) - cy) * g.ray_res[1]
            rays |= (dx * dx)[None, :] + (dy * dy)[:, None] <= m * m
    return rays


def spots(g, hit, lateral=0.0):
    """(d): the spot mask uint8 [L][ny][nx]."""
    out = np.zeros((hit.shape[0], g.spot_ny, g.spot_nx), dtype=np.uint8)
    for sy in range(g.spot_ny):
        for sx in range(g.spot_nx):
            rays = spot_rays(g, sx, sy, lateral)
            out[:, sy, sx] = hit[:, rays].any(axis=1)
    return out


def select(g, mask, wepl, peaks, lateral=0.0, proximal=0.0, distal=0.0):
    """Everything at once: (inside [S][H][W] bool, summary dict, hits [L][H][W], spot mask [L][ny][nx])."""
    wepl = np.asarray(wepl, dtype=F).reshape(g.S, g.H, g.W)
    inside = project(g, mask)
    hit = hits(inside, wepl, peaks, proximal, distal)
    return inside, summary(inside, wepl), hit, spots(g, hit, lateral)
