"""The numpy restatement of rtd_dose_resample and rtd_dose_quantize (include/rtd.h "Dose volumes between grids"): float32 operations in
the stated order for the resampling, float64 for the quantiser. Volumes are [Z][Y][X]; dims and the map are (x, y, z) as in the header.
No engine code is imported here."""
import numpy as np

F = np.float32
F32, U16, U32 = 0, 1, 2


def identity():
    return np.eye(3), np.zeros(3)


def rotation_map():
    """The general map of the tests: 17 degrees about z, scaled by 0.6 (z by 1.3), shifted so that part of 50 x 23 x 9 lands in 37 x 19 x 11."""
    a = np.deg2rad(17.0)
    m = np.array([[0.6 * np.cos(a), -0.6 * np.sin(a), 0.0], [0.6 * np.sin(a), 0.6 * np.cos(a), 0.0], [0.0, 0.0, 1.3]])
    return m, np.array([-4.5, -2.5, -0.75])


def positions(m, v, dst_dims):
    """p_a of every destination voxel: three float32 arrays [Z][Y][X], each product and sum rounded, in the header's order."""
    m = np.asarray(m, dtype=F).reshape(3, 3)
    v = np.asarray(v, dtype=F).reshape(3)
    nx, ny, nz = (int(d) for d in dst_dims)
    x = np.arange(nx, dtype=F)[None, None, :]
    y = np.arange(ny, dtype=F)[None, :, None]
    z = np.arange(nz, dtype=F)[:, None, None]
    out = []
    for a in range(3):
        p = ((m[a, 0] * x + m[a, 1] * y).astype(F) + (m[a, 2] * z).astype(F)).astype(F) + v[a]
        out.append(np.broadcast_to(p.astype(F), (nz, ny, nx)))
    return out


def node_values(src, src_scale):
    """The float32 value of every source node: the float itself, or float(double(raw) * src_scale)."""
    src = np.asarray(src)
    if src.dtype == np.float32:
        return src
    assert src.dtype in (np.uint16, np.uint32)
    return (src.astype(np.float64) * np.float64(src_scale)).astype(F)


def resample(src, m, v, dst_dims, *, scale=1.0, src_scale=1.0, accumulate=False, dst=None):
    """-> (dst [Z][Y][X] float32, inside [Z][Y][X] bool). With accumulate, dst is the volume added to (a copy is returned)."""
    val = node_values(src, src_scale)
    nz, ny, nx = val.shape
    n = (nx, ny, nz)
    p = positions(m, v, dst_dims)
    with np.errstate(invalid="ignore"):
        inside = np.ones(p[0].shape, dtype=bool)
        for a in range(3):
            inside &= (p[a] > F(-1.0)) & (p[a] < F(n[a]))
    f = [np.floor(q).astype(F) for q in p]
    t = [(q - fl).astype(F) for q, fl in zip(p, f)]
    i0 = [np.where(inside, fl, 0).astype(np.int64) for fl in f]

    def node(dx, dy, dz):
        ix, iy, iz = i0[0] + dx, i0[1] + dy, i0[2] + dz
        ok = inside & (ix >= 0) & (ix <= nx - 1) & (iy >= 0) & (iy <= ny - 1) & (iz >= 0) & (iz <= nz - 1)
        got = val[np.clip(iz, 0, nz - 1), np.clip(iy, 0, ny - 1), np.clip(ix, 0, nx - 1)]
        return np.where(ok, got, F(0.0)).astype(F)

    def blend(a, b, w):
        return (a + (w * (b - a).astype(F)).astype(F)).astype(F)

    with np.errstate(invalid="ignore", over="ignore"):
        c00 = blend(node(0, 0, 0), node(1, 0, 0), t[0])
        c10 = blend(node(0, 1, 0), node(1, 1, 0), t[0])
        c01 = blend(node(0, 0, 1), node(1, 0, 1), t[0])
        c11 = blend(node(0, 1, 1), node(1, 1, 1), t[0])
        e = blend(blend(c00, c10, t[1]), blend(c01, c11, t[1]), t[2])
        out = (F(scale) * e).astype(F)
        if accumulate:
            base = np.array(dst, dtype=F, copy=True)
            assert base.shape == out.shape
            res = np.where(inside, (base + out).astype(F), base)
        else:
            res = np.where(inside, out, F(0.0))
    return np.ascontiguousarray(res, dtype=F), inside


def grid_scaling(max_dose, bits):
    """The scale the quantiser chooses: strtod of the "%.10g" text of x = double(max) / qmax, with x grown by 1e-10 of itself while the
    largest dose would be clamped (ten digits can round x down by two 32-bit steps); 1 for an all-zero dose."""
    if not max_dose > 0:
        return 1.0
    mx, qmax = float(F(max_dose)), float(2 ** bits - 1)
    x = mx / qmax
    while True:
        s = float("%.10g" % x)
        if np.rint(mx / s) <= qmax:
            return s
        x = x * (1.0 + 1e-10)


def quantize(dose, bits=16, scaling=0.0):
    """-> (ints, scaling, n_clamped): q = rint(double(d) / s), ties to even, clamped to [0, 2^bits - 1]; a NaN stores 0."""
    d = np.asarray(dose, dtype=F)
    qmax = float(2 ** bits - 1)
    if scaling == 0.0:
        finite = d[np.isfinite(d)]
        scaling = grid_scaling(max(float(finite.max()) if finite.size else 0.0, 0.0), bits)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = np.rint(d.astype(np.float64) / np.float64(scaling))
        ok = (q >= 0.0) & (q <= qmax)
        stored = np.where(q >= 0.0, np.minimum(q, qmax), 0.0)
    stored = np.where(np.isnan(stored), 0.0, stored)
    return stored.astype(np.uint16 if bits == 16 else np.uint32), scaling, int((~ok).sum())
