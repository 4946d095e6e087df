"""The rules of include/rtd.h "Dose-averaged LET", restated in numpy (a plain module, no tests): the voxel -> (ray, step) position,
the clamped trilinear water-equivalent depth, the table lookup and the product. Every float operation is a float32 numpy operation
in the header's order, so the results are meant to equal the engine's bit for bit.

Inputs: the beam (scenarios.BeamSettings), ray_dims / ray_res / ray_offset / beam_first_inside of the field info, wepl [S][H][W]
float32 (rtd_field_fetch "wepl"), "layer_plan" columns 0 and 1 (energyIdx, energyScaleFact) and the LET table."""
import numpy as np

F = np.float32
PAD = F(32.0)       # the padding of the beam's-eye-view grid on either side of the ray grid


def _f(a):
    return np.asarray(a, dtype=F)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _inverse3(m):
    """inverse(Mat3) of rtd_geometry.hpp: float32 cofactors, one reciprocal of the determinant taken in float64 and rounded."""
    a = _f(m).reshape(3, 3)
    det = (a[0, 0] * (a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]) - a[0, 1] * (a[1, 0] * a[2, 2] - a[1, 2] * a[2, 0])) \
        + a[0, 2] * (a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0])
    ood = F(1.0 / np.float64(det))
    adj = np.array([
        [a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1], a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2], a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]],
        [a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2], a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0], a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]],
        [a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0], a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1], a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]]], dtype=F)
    return (adj * ood).astype(F)     # (the product with the diagonal matrix adds exact zeros)


class Transfer:
    """TransferParams of a field (rtd_geometry.hpp: invertAndShift of the ray-index -> dose-index map by the padding, then
    makeTransferParams), with the z shift by -beam_first_inside that the plan applies on the device."""

    def __init__(self, beam, info):
        m, v = _f(beam.gantryToDoseIdx.m).reshape(3, 3), _f(beam.gantryToDoseIdx.v).reshape(3)
        res, off = _f(info["ray_res"]), _f(info["ray_offset"])
        dist = _f(beam.sourceDist)
        self.first = int(info["beam_first_inside"])
        with np.errstate(all="ignore"):
            inv = _inverse3(m)
            nv = (v * F(-1.0)).astype(F)
            iv = np.array([_dot(inv[r], nv) for r in range(3)], dtype=F)
            delta = (F(1.0) / res).astype(F)
            offset = ((F(-1.0) * off) / res + np.array([PAD, PAD, F(0.0)], dtype=F)).astype(F)
            t = inv.T                                                 # rows of the transpose
            self.coef_i = (t[0] * delta).astype(F)
            self.coef_j = (t[1] * delta).astype(F)
            self.inc = (t[2] * delta).astype(F)
            self.coef_offset = (iv * delta).astype(F)
            self.global_offset = offset.copy()
            self.global_offset[2] = offset[2] + (-F(self.first))
            self.norm_dist = (delta[2] * dist).astype(F)

    def fan_index(self, x, y, z):
        """getFanIdx(z) after init(x, y): the padded beam's-eye-view position (three float32 arrays) of dose voxels; x, y, z
        broadcastable integer arrays."""
        x, y, z = (np.asarray(c).astype(F) for c in (x, y, z))
        with np.errstate(all="ignore"):
            start = [(x * self.coef_i[c] + y * self.coef_j[c]) + self.coef_offset[c] for c in range(3)]
            r = [start[c] + z * self.inc[c] for c in range(3)]
            r[0] = r[0] * (F(1.0) + r[2] / (self.norm_dist[0] - r[2]))
            r[1] = r[1] * (F(1.0) + r[2] / (self.norm_dist[1] - r[2]))
            return tuple((r[c] + self.global_offset[c]).astype(F) for c in range(3))

    def trace_index(self, x, y, z):
        """The position in the indices of the [S][H][W] trace arrays: (i, j, k) float32."""
        px, py, pz = self.fan_index(x, y, z)
        return (px - PAD).astype(F), (py - PAD).astype(F), (pz + F(self.first)).astype(F)


def nodes(p, n):
    """Per axis: (node 0, node 1, weight of node 1), clamped at both faces with weight 0."""
    p = _f(p)
    with np.errstate(all="ignore"):
        fl = np.floor(p)
        a = (p - fl).astype(F)
        low = ~(p >= F(0.0))
        high = p >= F(n - 1)
        i0 = np.where(low | high, 0, fl).astype(np.int64)
        i0 = np.where(high, n - 1, i0)
        i1 = np.where(low | high, i0, i0 + 1)
        a = np.where(low | high, F(0.0), a).astype(F)
    return i0, i1, a


def lerp(a, v0, v1):
    return ((F(1.0) - a) * v0 + a * v1).astype(F)


def step_depth(wepl, first):
    """[S][H][W]: the depth at which the fill evaluates a step's dose, 0.5 * (wepl[k] + old), old = wepl[k - 1] behind the entry
    step `first` and 0 up to it."""
    wepl = _f(wepl)
    old = np.zeros_like(wepl)
    old[1:] = wepl[:-1]
    k = np.arange(wepl.shape[0])[:, None, None]
    old = np.where(k > first, old, F(0.0)).astype(F)
    return (F(0.5) * (wepl + old)).astype(F)


def water_depth(tr, wepl, x, y, z):
    """The clamped trilinear depth (float32) of dose voxels (x, y, z): broadcastable integer arrays."""
    d = step_depth(wepl, tr.first)
    S, H, W = d.shape
    pi, pj, pk = tr.trace_index(x, y, z)
    i0, i1, ax = nodes(pi, W)
    j0, j1, ay = nodes(pj, H)
    k0, k1, az = nodes(pk, S)
    c00 = lerp(ax, d[k0, j0, i0], d[k0, j0, i1])
    c10 = lerp(ax, d[k0, j1, i0], d[k0, j1, i1])
    c01 = lerp(ax, d[k1, j0, i0], d[k1, j0, i1])
    c11 = lerp(ax, d[k1, j1, i0], d[k1, j1, i1])
    return lerp(az, lerp(ay, c00, c10), lerp(ay, c01, c11))


def box_depth(tr, wepl, lo, hi):
    """The depth over the inclusive dose-index box lo .. hi (x, y, z) as a [Z][Y][X] array of the box."""
    x = np.arange(lo[0], hi[0] + 1)[None, None, :]
    y = np.arange(lo[1], hi[1] + 1)[None, :, None]
    z = np.arange(lo[2], hi[2] + 1)[:, None, None]
    return water_depth(tr, wepl, x, y, z)


def lookup(table, energy_idx, scale, depth):
    """L(l, d) for one layer (energy_idx, scale: float32 scalars) at float32 depths: the fill's two rows and row weight, the sample
    position depth * scale clamped to the row."""
    table = _f(table)
    n_e, n_s = table.shape
    py = F(energy_idx)
    fy = np.floor(py)
    w = F(py - fy)
    r0, r1 = int(fy), int(fy) + 1
    if not py >= F(0.0):
        r0, r1, w = 0, 0, F(0.0)
    r0, r1 = min(r0, n_e - 1), min(r1, n_e - 1)
    with np.errstate(all="ignore"):
        x0, x1, ax = nodes(_f(depth) * F(scale), n_s)
    return lerp(w, lerp(ax, table[r0][x0], table[r0][x1]), lerp(ax, table[r1][x0], table[r1][x1]))


def let_values(d_values, d_rows, d_indptr, spots_per_layer, layer_plan, table, depth_of_voxel):
    """N = float32(D * L) on the CSC structure: depth_of_voxel is indexed by the flat voxel index of the dose grid."""
    out = np.empty_like(_f(d_values))
    cols = np.repeat(np.arange(len(d_indptr) - 1, dtype=np.int64), np.diff(d_indptr))
    layer = cols // spots_per_layer
    for l in np.unique(layer):
        m = layer == l
        out[m] = (_f(d_values)[m] * lookup(table, layer_plan[l, 0], layer_plan[l, 1], _f(depth_of_voxel)[d_rows[m]])).astype(F)
    return out
