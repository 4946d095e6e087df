"""The numpy restatement of rtd_dose_warp and rtd_dose_warp_t (include/rtd.h "Deformable dose warping"): float32 operations in the
stated order for the forward rule and the contributions of the transposed one, int64 sums of quanta (np.add.at) for its accumulation.
Volumes are [Z][Y][X], the field is [3][Z][Y][X]; dims and the maps are (x, y, z) as in the header. No engine code is imported here."""
import collections

import numpy as np

import resample_reference as rr

F = np.float32

# m, v: dst_idx_to_src_idx; fm, fv: dst_idx_to_dvf_idx; k: disp_to_src_idx (3x3); dvf: [3][Z][Y][X] float32
Warp = collections.namedtuple("Warp", "m v fm fv k dvf")


def make(m, v, fm, fv, k, dvf):
    return Warp(np.asarray(m, dtype=F).reshape(3, 3), np.asarray(v, dtype=F).reshape(3), np.asarray(fm, dtype=F).reshape(3, 3),
                np.asarray(fv, dtype=F).reshape(3), np.asarray(k, dtype=F).reshape(3, 3), np.ascontiguousarray(dvf, dtype=F))


# ---- the cases the CPU and the GPU tests share ----

SRC_DIMS, DST_DIMS, DVF_DIMS = (37, 19, 11), (50, 23, 9), (9, 7, 5)
K = np.array([[0.5, 0.1, 0.0], [-0.05, 0.4, 0.02], [0.0, 0.03, 0.8]])      # displacement ("mm") -> source voxels: not diagonal


def spanning(dvf_dims, dst_dims):
    """dst_idx_to_dvf_idx of a field whose first and last nodes lie on the first and last destination voxels (a dimension of 1: all on node 0)."""
    return np.diag([(f - 1) / (d - 1) if d > 1 else 0.0 for f, d in zip(dvf_dims, dst_dims)]), np.zeros(3)


def random_field(dvf_dims, amplitude=2.5, seed=3, k=K):
    """[3][Z][Y][X] float32: k times the field is uniform in +-amplitude source voxels per axis."""
    s = np.random.default_rng(seed).uniform(-amplitude, amplitude, (3, dvf_dims[2], dvf_dims[1], dvf_dims[0]))
    return np.einsum("ab,bzyx->azyx", np.linalg.inv(k), s).astype(F)


def standard(dvf_dims=DVF_DIMS, dst_dims=DST_DIMS, seed=3, amplitude=2.5):
    """The standard case: the rotation map of the resampling tests, a field that spans the destination, +-2.5 source voxels."""
    m, v = rr.rotation_map()
    fm, fv = spanning(dvf_dims, dst_dims)
    return make(m, v, fm, fv, K, random_field(dvf_dims, amplitude, seed))


def collapsing(point=(18.0, 9.0, 5.0), dst_dims=DST_DIMS, seed=4):
    """A field on the destination's own grid that sends every destination voxel into the one source cell above `point`: every
    contribution of the transposed rule lands on the same 8 nodes."""
    m, v = rr.rotation_map()
    base = [b.astype(np.float64) for b in rr.positions(m, v, dst_dims)]
    jitter = np.random.default_rng(seed).uniform(0.05, 0.95, (3,) + base[0].shape)
    s = np.stack([point[a] + jitter[a] - base[a] for a in range(3)])
    return make(m, v, np.eye(3), np.zeros(3), K, np.einsum("ab,bzyx->azyx", np.linalg.inv(K), s).astype(F))


def _blend(a, b, w):
    return (a + (w * (b - a).astype(F)).astype(F)).astype(F)


def displacement(w, dst_dims):
    """-> (u: three float32 arrays [Z][Y][X], known: bool, false where a field position is a NaN)."""
    q = rr.positions(w.fm, w.fv, dst_dims)
    known = ~(np.isnan(q[0]) | np.isnan(q[1]) | np.isnan(q[2]))
    n = (w.dvf.shape[3], w.dvf.shape[2], w.dvf.shape[1])
    i0, i1, t = [], [], []
    for a in range(3):
        qc = np.minimum(np.maximum(np.where(known, q[a], F(0.0)), F(0.0)), F(n[a] - 1)).astype(F)
        f = np.floor(qc).astype(F)
        t.append((qc - f).astype(F))
        i0.append(f.astype(np.int64))
        i1.append(np.minimum(f.astype(np.int64) + 1, n[a] - 1))
    u = []
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            vol = w.dvf[c]
            c00 = _blend(vol[i0[2], i0[1], i0[0]], vol[i0[2], i0[1], i1[0]], t[0])
            c10 = _blend(vol[i0[2], i1[1], i0[0]], vol[i0[2], i1[1], i1[0]], t[0])
            c01 = _blend(vol[i1[2], i0[1], i0[0]], vol[i1[2], i0[1], i1[0]], t[0])
            c11 = _blend(vol[i1[2], i1[1], i0[0]], vol[i1[2], i1[1], i1[0]], t[0])
            u.append(_blend(_blend(c00, c10, t[1]), _blend(c01, c11, t[1]), t[2]))
    return u, known


def positions(w, dst_dims):
    """p_a of every destination voxel, the displacement included: three float32 arrays [Z][Y][X]; a NaN where the field position is one."""
    u, known = displacement(w, dst_dims)
    base = rr.positions(w.m, w.v, dst_dims)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            s = (((w.k[a, 0] * u[0]).astype(F) + (w.k[a, 1] * u[1]).astype(F)).astype(F) + (w.k[a, 2] * u[2]).astype(F)).astype(F)
            out.append(np.where(known, (base[a] + s).astype(F), F(np.nan)).astype(F))
    return out


def _nodes(p, n):
    """The resampler's Outside and Nodes rules for positions p on a grid of n = (nx, ny, nz) -> (inside, i0 int64 per axis (0 where
    outside), t float32 per axis)."""
    with np.errstate(invalid="ignore"):
        inside = np.ones(p[0].shape, dtype=bool)
        for a in range(3):
            inside &= (p[a] > F(-1.0)) & (p[a] < F(n[a]))
        f = [np.floor(np.where(inside, q, F(0.0))).astype(F) for q in p]
        t = [(np.where(inside, q, F(0.0)) - fl).astype(F) for q, fl in zip(p, f)]
    i0 = [fl.astype(np.int64) for fl in f]
    return inside, i0, t


def warp(src, w, dst_dims, *, scale=1.0, src_scale=1.0, accumulate=False, dst=None):
    """-> (dst [Z][Y][X] float32, inside [Z][Y][X] bool). With accumulate, dst is the volume added to (a copy is returned)."""
    val = rr.node_values(src, src_scale)
    nz, ny, nx = val.shape
    inside, i0, t = _nodes(positions(w, dst_dims), (nx, ny, nz))

    def node(dx, dy, dz):
        ix, iy, iz = i0[0] + dx, i0[1] + dy, i0[2] + dz
        ok = inside & (ix >= 0) & (ix <= nx - 1) & (iy >= 0) & (iy <= ny - 1) & (iz >= 0) & (iz <= nz - 1)
        got = val[np.clip(iz, 0, nz - 1), np.clip(iy, 0, ny - 1), np.clip(ix, 0, nx - 1)]
        return np.where(ok, got, F(0.0)).astype(F)

    with np.errstate(invalid="ignore", over="ignore"):
        c00 = _blend(node(0, 0, 0), node(1, 0, 0), t[0])
        c10 = _blend(node(0, 1, 0), node(1, 1, 0), t[0])
        c01 = _blend(node(0, 0, 1), node(1, 0, 1), t[0])
        c11 = _blend(node(0, 1, 1), node(1, 1, 1), t[0])
        e = _blend(_blend(c00, c10, t[1]), _blend(c01, c11, t[1]), t[2])
        out = (F(scale) * e).astype(F)
        if accumulate:
            base = np.array(dst, dtype=F, copy=True)
            assert base.shape == out.shape
            res = np.where(inside, (base + out).astype(F), base)
        else:
            res = np.where(inside, out, F(0.0))
    return np.ascontiguousarray(res, dtype=F), inside


def scaled_gradient(g, scale):
    """sg = scale * g in float32, with everything that is not finite counted as zero."""
    with np.errstate(invalid="ignore", over="ignore"):
        sg = (F(scale) * np.asarray(g, dtype=F)).astype(F)
    return np.where(np.isfinite(sg), sg, F(0.0)).astype(F)


def exponent(m):
    """E of m = f * 2^E with f in [0.5, 1) (m > 0, float32; a denormal included)."""
    return int(np.frexp(F(m))[1])


def _contributions(g, w, src_dims, scale):
    """Every contribution of the transposed rule -> (node index int64, c float32, destination voxel int64), flat arrays over the
    (voxel, node) pairs whose voxel is inside and whose node lies on the source grid."""
    nx, ny, nz = (int(d) for d in src_dims)
    sg = scaled_gradient(g, scale)
    dst_dims = (sg.shape[2], sg.shape[1], sg.shape[0])
    inside, i0, t = _nodes(positions(w, dst_dims), (nx, ny, nz))
    wt = [((F(1.0) - ta).astype(F), ta) for ta in t]
    voxel = np.arange(sg.size, dtype=np.int64).reshape(sg.shape)
    idx, con, vox = [], [], []
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                ix, iy, iz = i0[0] + dx, i0[1] + dy, i0[2] + dz
                ok = inside & (ix >= 0) & (ix <= nx - 1) & (iy >= 0) & (iy <= ny - 1) & (iz >= 0) & (iz <= nz - 1)
                c = (((sg * wt[0][dx]).astype(F) * wt[1][dy]).astype(F) * wt[2][dz]).astype(F)
                idx.append(((iz * ny + iy) * nx + ix)[ok])
                con.append(c[ok])
                vox.append(voxel[ok])
    return np.concatenate(idx), np.concatenate(con), np.concatenate(vox)


def warp_t(g, w, src_dims, scale=1.0, accumulate=False, base=None):
    """-> g_src [Z][Y][X] float32 on src_dims (x, y, z). With accumulate, base is the volume added to (a copy is returned)."""
    nx, ny, nz = (int(d) for d in src_dims)
    start = np.array(base, dtype=F, copy=True).reshape(nz, ny, nx) if accumulate else np.zeros((nz, ny, nx), dtype=F)
    big = float(np.abs(scaled_gradient(g, scale)).max())
    if big == 0.0:
        return start
    e = exponent(big)
    idx, con, _ = _contributions(g, w, src_dims, scale)
    sums = np.zeros(nx * ny * nz, dtype=np.int64)
    np.add.at(sums, idx, np.rint(con.astype(np.float64) * 2.0 ** (30 - e)).astype(np.int64))      # (np.rint: ties to even)
    out = (sums.astype(np.float64) * 2.0 ** (e - 30)).astype(F).reshape(nz, ny, nx)
    with np.errstate(invalid="ignore", over="ignore"):
        return (start + out).astype(F) if accumulate else out


class Exact:
    """A sparse operator in float64 as (row, column, value) triples with repeated pairs allowed: A @ x, A.T @ y, abs(A), A.counts()."""

    def __init__(self, rows, cols, vals, shape):
        self.rows, self.cols, self.vals, self.shape = rows, cols, vals, shape

    @property
    def T(self):
        return Exact(self.cols, self.rows, self.vals, (self.shape[1], self.shape[0]))

    def __abs__(self):
        return Exact(self.rows, self.cols, np.abs(self.vals), self.shape)

    def __matmul__(self, x):
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        assert x.size == self.shape[1]
        return np.bincount(self.rows, weights=self.vals * x[self.cols], minlength=self.shape[0])

    def counts(self):
        """Entries per column."""
        return np.bincount(self.cols, minlength=self.shape[1])


def warp_exact(w, src_dims, dst_dims):
    """The forward operator at scale 1 on a float32 source as float64 weights, [destination voxels] x [source voxels]: per inside
    voxel and existing node the product of the three weights (1 - t_a | t_a, exact in float64 from the float32 t_a)."""
    ones = np.ones((int(dst_dims[2]), int(dst_dims[1]), int(dst_dims[0])), dtype=F)
    nx, ny, nz = (int(d) for d in src_dims)
    inside, i0, t = _nodes(positions(w, dst_dims), (nx, ny, nz))
    t = [ta.astype(np.float64) for ta in t]
    voxel = np.arange(ones.size, dtype=np.int64).reshape(ones.shape)
    rows, cols, vals = [], [], []
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                ix, iy, iz = i0[0] + dx, i0[1] + dy, i0[2] + dz
                ok = inside & (ix >= 0) & (ix <= nx - 1) & (iy >= 0) & (iy <= ny - 1) & (iz >= 0) & (iz <= nz - 1)
                wgt = (t[0] if dx else 1.0 - t[0]) * (t[1] if dy else 1.0 - t[1]) * (t[2] if dz else 1.0 - t[2])
                rows.append(voxel[ok])
                cols.append(((iz * ny + iy) * nx + ix)[ok])
                vals.append(wgt[ok])
    return Exact(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), (ones.size, nx * ny * nz))
