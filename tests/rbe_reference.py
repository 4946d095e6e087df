"""The numpy restatement of the variable-RBE contract (include/rtd.h "Variable-RBE dose"). A test helper, not
product code: the device kernels are compared with it bit for bit.

A tissue is (alpha_x, beta_x, rbe_max[2], rbe_min[2]) as float32 fields (what the C struct holds). coefficients() forms a0 .. b1 the way
the host does: in float64 from those fields, each rounded once to float32. forward() / backward() are the per-voxel float32 steps in
the order of the header (numpy rounds every operation and never contracts; its float32 division and square root are correctly
rounded). Rbe is the object: a class per voxel, later assignments overwrite earlier ones, and a box leaves what lies outside alone.
forward64 is the same formulas in float64 from the same float32 coefficients' SOURCES (the tissue fields), for the error bounds."""
import numpy as np

F = np.float32


def tissue_fields(t):
    """An abi.RtdRbeTissue (or a 4-tuple alpha_x, beta_x, rbe_max, rbe_min) -> the float32 fields the C struct holds."""
    if isinstance(t, tuple):
        ax, bx, mx, mn = t
    else:
        ax, bx, mx, mn = t.alpha_x, t.beta_x, tuple(t.rbe_max), tuple(t.rbe_min)
    return F(ax), F(bx), (F(mx[0]), F(mx[1])), (F(mn[0]), F(mn[1]))


def coefficients(t):
    """-> float32 [a0, a1, b0, b1, alpha_x, beta_x]: products in float64 of the float32 fields, rounded once."""
    ax, bx, mx, mn = tissue_fields(t)
    a64, sb = np.float64(ax), np.sqrt(np.float64(bx))
    return np.array([F(a64 * np.float64(mx[0])), F(a64 * np.float64(mx[1])), F(sb * np.float64(mn[0])), F(sb * np.float64(mn[1])), ax, bx], dtype=F)


def _effect(c, d, n):
    """c: float32 coefficient arrays (a0, a1, b0, b1, ax, bx), each broadcastable against d. -> (e, B) in float32."""
    a0, a1, b0, b1 = c[0], c[1], c[2], c[3]
    A = (a0 * d).astype(F) + (a1 * n).astype(F)
    B = (b0 * d).astype(F) + (b1 * n).astype(F)
    e = A + (B * B).astype(F)
    return e.astype(F), B.astype(F)


def _root(c, e):
    ax, bx = c[4], c[5]
    return np.sqrt(((ax * ax).astype(F) + ((F(4.0) * bx).astype(F) * e).astype(F)).astype(F)).astype(F)


def forward(c, d, n):
    """R in float32; c as _effect takes it (per-voxel coefficient arrays or scalars)."""
    d, n = np.asarray(d, dtype=F), np.asarray(n, dtype=F)
    c = [np.asarray(x, dtype=F) for x in c]
    with np.errstate(all="ignore"):
        e, _ = _effect(c, d, n)
        ok = e >= F(0.0)
        s = _root(c, np.where(ok, e, F(0.0)))
        R = ((F(2.0) * e).astype(F) / (s + c[4]).astype(F)).astype(F)
    return np.where(ok, R, F(0.0)).astype(F)


def derivatives(c, d, n):
    """(fd, fn) in float32, 0 where e is not >= 0."""
    d, n = np.asarray(d, dtype=F), np.asarray(n, dtype=F)
    c = [np.asarray(x, dtype=F) for x in c]
    with np.errstate(all="ignore"):
        e, B = _effect(c, d, n)
        ok = e >= F(0.0)
        k = (F(1.0) / _root(c, np.where(ok, e, F(0.0)))).astype(F)
        B2 = (F(2.0) * B).astype(F)
        fd = (k * (c[0] + (B2 * c[2]).astype(F)).astype(F)).astype(F)
        fn = (k * (c[1] + (B2 * c[3]).astype(F)).astype(F)).astype(F)
    return np.where(ok, fd, F(0.0)).astype(F), np.where(ok, fn, F(0.0)).astype(F)


def backward(c, d, n, g):
    """(g_d, g_n) = (g * fd, g * fn) in float32."""
    fd, fn = derivatives(c, d, n)
    g = np.asarray(g, dtype=F)
    with np.errstate(all="ignore"):
        return (g * fd).astype(F), (g * fn).astype(F)


def forward64(t, d, n):
    """(R, fd, fn, a1) in float64 from the tissue's float32 fields, every step in float64 (no rounding of the coefficients)."""
    ax, bx, mx, mn = tissue_fields(t)
    ax, bx, mx, mn = np.float64(ax), np.float64(bx), (np.float64(mx[0]), np.float64(mx[1])), (np.float64(mn[0]), np.float64(mn[1]))
    d, n = np.asarray(d, dtype=np.float64), np.asarray(n, dtype=np.float64)
    sb = np.sqrt(bx)
    a0, a1, b0, b1 = ax * mx[0], ax * mx[1], sb * mn[0], sb * mn[1]
    A, B = a0 * d + a1 * n, b0 * d + b1 * n
    e = A + B * B
    s = np.sqrt(ax * ax + 4.0 * bx * e)
    return 2.0 * e / (s + ax), (a0 + 2.0 * B * b0) / s, (a1 + 2.0 * B * b1) / s, a1


class Rbe:
    """The object: dims (x, y, z), a uint8 class per voxel (x fastest), a tissue per class."""

    def __init__(self, dims, tissue):
        self.dims = tuple(int(v) for v in dims)
        self.n_voxels = self.dims[0] * self.dims[1] * self.dims[2]
        self.classes = np.zeros(self.n_voxels, dtype=np.uint8)
        self.table = [coefficients(tissue)]

    def add_tissue(self, tissue):
        assert len(self.table) < 256
        self.table.append(coefficients(tissue))
        return len(self.table) - 1

    def assign(self, where, class_id):
        assert 0 <= class_id < len(self.table)
        a = np.asarray(where)
        idx = np.flatnonzero(a) if a.dtype == np.bool_ else a.reshape(-1).astype(np.int64)
        assert idx.size == 0 or (idx.min() >= 0 and idx.max() < self.n_voxels)
        self.classes[idx] = class_id                                   # (a later assignment overwrites an earlier one)

    def _coef(self):
        tab = np.stack(self.table).astype(F)                           # [classes][6]
        return [tab[self.classes, k] for k in range(6)]

    def box_mask(self, box):
        m = np.zeros((self.dims[2], self.dims[1], self.dims[0]), dtype=bool)
        if box is None:
            m[:] = True
        else:
            lo, hi = box
            m[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
        return m.reshape(-1)

    def dose(self, d, n, out, box=None):
        """out (flat float32) with R written inside the box and untouched outside it."""
        m = self.box_mask(box)
        res = np.array(out, dtype=F).reshape(-1)
        res[m] = forward(self._coef(), np.asarray(d, dtype=F).reshape(-1), np.asarray(n, dtype=F).reshape(-1))[m]
        return res

    def backward(self, d, n, g, out_d, out_n, box=None):
        m = self.box_mask(box)
        gd, gn = backward(self._coef(), np.asarray(d, dtype=F).reshape(-1), np.asarray(n, dtype=F).reshape(-1), np.asarray(g, dtype=F).reshape(-1))
        rd, rn = np.array(out_d, dtype=F).reshape(-1), np.array(out_n, dtype=F).reshape(-1)
        rd[m], rn[m] = gd[m], gn[m]
        return rd, rn
