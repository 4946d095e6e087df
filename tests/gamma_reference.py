"""The gamma index of include/rtd.h ("Gamma index of two dose volumes") restated in numpy, float32 operation by operation: vectorised
over the volume, one shifted (and, with interp > 1, blended) copy of the evaluated dose per offset. A plain module (no tests, no
plugin); tests/test_gamma_reference.py checks it against the CPU oracle, tests/test_gpu_gamma.py checks the engine against it.

Every number is a numpy float32 scalar or array, so every product, quotient, sum and difference is rounded to float32 as the header
states; numpy's float32 division and square root are correctly rounded."""
import collections

import numpy as np

F = np.float32

Result = collections.namedtuple("Result", "n_passed n_evaluated max_gamma norm map")


def triple(res):
    """(pass_rate, n_evaluated, max_gamma) as oracle.gamma_pass_rate and Engine.gamma return it."""
    return (res.n_passed / res.n_evaluated if res.n_evaluated else 1.0, res.n_evaluated, float(res.max_gamma))


def radii(spacing, dta, search_mult=1.5):
    return [int(np.ceil(F(F(search_mult) * F(dta)) / F(s))) for s in spacing]


def _axis(i, k, n):
    """Offset i of an axis with n nodes at k samples per step: (index of the lower node per voxel, of the upper one, t, exists)."""
    b = i // k                                                        # floor_div
    f = i - b * k
    p = np.arange(n) + b
    ok = (p >= 0) & (p <= n - 1) & ~((p == n - 1) & (f != 0))
    lo = np.clip(p, 0, n - 1)                                         # (clipped where the sample is skipped: never used there)
    return lo, np.minimum(lo + 1, n - 1), F(f) / F(k), ok


def _blend(a, b, t):
    return a + t * (b - a)


def gamma(ref, ev, spacing, dd=0.01, dta=1.0, threshold=0.10, *, local=False, interp=1, norm_dose=0.0, search_mult=1.5, mask=None):
    """ref, ev: [Z][Y][X] float32; spacing (x, y, z) mm; mask: [Z][Y][X], non-zero = evaluate -> Result (the map is float32 [Z][Y][X],
    -1 where nothing is evaluated)."""
    ref = np.ascontiguousarray(ref, dtype=F)
    ev = np.ascontiguousarray(ev, dtype=F)
    nz, ny, nx = ref.shape
    k = int(interp)
    assert k in (1, 2, 4, 8)
    norm = F(norm_dose) if norm_dose > 0 else max(F(0.0), ref.max())
    gmap = np.full(ref.shape, -1.0, dtype=F)
    if not norm > 0:
        return Result(0, 0, F(0.0), norm, gmap)
    thr = F(threshold) * norm
    evaluated = ref >= thr
    if mask is not None:
        evaluated &= np.asarray(mask) != 0
    if local:
        evaluated &= ref > 0
    dd_v = F(dd) * ref if local else F(dd) * norm
    dd2 = dd_v * dd_v
    dta2 = F(dta) * F(dta)
    rx, ry, rz = radii(spacing, dta, search_mult)
    step = [F(s) / F(k) for s in spacing]
    best = np.full(ref.shape, np.inf, dtype=F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        # the blend runs along x, then y, then z: the x blend of an x offset serves all its (y, z) offsets, the y blend all its z offsets
        for ix in range(-k * rx, k * rx + 1):
            lo, up, tx, okx = _axis(ix, k, nx)
            cx = ev[:, :, lo] if k == 1 else _blend(ev[:, :, lo], ev[:, :, up], tx)
            ox = F(ix) * step[0]
            for iy in range(-k * ry, k * ry + 1):
                lo, up, ty, oky = _axis(iy, k, ny)
                cy = cx[:, lo, :] if k == 1 else _blend(cx[:, lo, :], cx[:, up, :], ty)
                oy = F(iy) * step[1]
                okxy = oky[None, :, None] & okx[None, None, :]
                for iz in range(-k * rz, k * rz + 1):
                    lo, up, tz, okz = _axis(iz, k, nz)
                    e = cy[lo] if k == 1 else _blend(cy[lo], cy[up], tz)
                    oz = F(iz) * step[2]
                    dist2 = (ox * ox + oy * oy) + oz * oz
                    dv = e - ref
                    g2 = dist2 / dta2 + (dv * dv) / dd2
                    best = np.where(okz[:, None, None] & okxy & (g2 < best), g2, best)
        g = np.sqrt(best)
    gmap[evaluated] = g[evaluated]
    n = int(evaluated.sum())
    return Result(int((evaluated & (g <= F(1.0))).sum()), n, g[evaluated].max() if n else F(0.0), norm, gmap)
