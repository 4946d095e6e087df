"""CPU checks of tests/rbe_reference.py, the float32 restatement of the variable-RBE contract (include/rtd.h "Variable-RBE dose";
DESIGN.md section 23), against the same formulas in float64, against known answers, and of its object rules (classes, overwrite, box,
the e >= 0 rule, the host's coefficients). No GPU needed."""
import numpy as np
import pytest

import rbe_reference as R
from raytracedicom_amd import abi, rbe

F = np.float32
BETA_X = 0.05
ABX = (2.0, 3.0, 10.0)
N_SAMPLES = 2_000_000


@pytest.fixture(scope="module")
def samples():
    """d in [0, 80] with exact zeros and values down to the 1e-4 scale, LETd in [0, 20], n = float32(d * LETd)."""
    rng = np.random.default_rng(23)
    d = (80.0 * rng.random(N_SAMPLES)).astype(F)
    d[: N_SAMPLES // 8] = (1e-4 * (1.0 + 99.0 * rng.random(N_SAMPLES // 8))).astype(F) * (10.0 ** rng.integers(0, 3, N_SAMPLES // 8)).astype(F)
    d[:1000] = 0.0
    letd = (20.0 * rng.random(N_SAMPLES)).astype(F)
    letd[1000:2000] = 0.0
    n = (d * letd).astype(F)
    assert d.min() == 0.0 and d[d > 0].min() < 2e-4 and d.max() > 79.0
    return d, n


@pytest.mark.parametrize("abx", ABX)
@pytest.mark.parametrize("model", rbe.MODELS)
def test_float32_steps_against_float64(samples, model, abx):
    """Relative error of R and of fd at most 1e-6; |fn - fn64| <= 1e-6 * (|a1| + |fn64|) (fn changes sign for McNamara). For the
    constant model additionally |R - 1.1 d| <= 1e-6 * 1.1 d."""
    d, n = samples
    t = rbe.tissue(model, abx * BETA_X, BETA_X)
    c = R.coefficients(t)
    got_r = R.forward(c, d, n).astype(np.float64)
    got_fd, got_fn = (x.astype(np.float64) for x in R.derivatives(c, d, n))
    r64, fd64, fn64, a1 = R.forward64(t, d, n)
    assert np.all(r64 >= 0) and np.all(fd64 > 0)
    err_r = np.abs(got_r - r64)
    live = r64 > 0
    worst_r = float((err_r[live] / r64[live]).max())
    worst_fd = float((np.abs(got_fd - fd64) / fd64).max())
    worst_fn = float((np.abs(got_fn - fn64) / (abs(a1) + np.abs(fn64) + 1e-300)).max())
    print("%s abx %g: worst relative error R %.3g, fd %.3g; fn against |a1| + |fn| %.3g" % (model, abx, worst_r, worst_fd, worst_fn))
    assert np.all(err_r <= 1e-6 * r64), worst_r
    assert np.all(np.abs(got_fd - fd64) <= 1e-6 * fd64), worst_fd
    assert np.all(np.abs(got_fn - fn64) <= 1e-6 * (abs(a1) + np.abs(fn64))), worst_fn
    if model == "constant":
        want = 1.1 * d.astype(np.float64)
        worst = float((np.abs(got_r - want)[live] / want[live]).max())
        print("constant abx %g: worst |R - 1.1 d| / (1.1 d) = %.3g" % (abx, worst))
        assert np.all(np.abs(got_r - want) <= 1e-6 * want), worst


def rbe64(model, abx, d, letd, beta_x=BETA_X):
    """R / d in float64 straight from the table of models (no float32 anywhere)."""
    alpha_x = abx * beta_x
    mx, mn = rbe.lines(model, alpha_x, beta_x)
    alpha, sqb = alpha_x * (mx[0] + mx[1] * letd), np.sqrt(beta_x) * (mn[0] + mn[1] * letd)
    e = alpha * d + (sqb * d) ** 2
    return 2.0 * e / (np.sqrt(alpha_x * alpha_x + 4.0 * beta_x * e) + alpha_x) / d


@pytest.mark.parametrize("model,abx,want", [("mcnamara", 2.0, 1.19363), ("wedenberg", 3.0, 1.14868), ("carabe", 2.0, 1.18596), ("mcnamara", 10.0, 1.07693)])
def test_pins_against_coefficient_typos(model, abx, want):
    """Regression values (float64 evaluations of the formulas at beta_x = 0.05, d = 2, LETd = 2.5), not literature values; and the
    float32 restatement on the tissue record agrees with them."""
    got = float(rbe64(model, abx, 2.0, 2.5))
    assert abs(got - want) <= 1e-5, got
    c = R.coefficients(rbe.tissue(model, abx * BETA_X, BETA_X))
    r32 = float(R.forward(c, F(2.0), F(5.0))) / 2.0
    assert abs(r32 - want) <= 1e-5, r32


@pytest.mark.parametrize("model", rbe.MODELS)
def test_derivatives_against_finite_differences(model):
    """fd and fn of the float64 formulas are the central differences of R in d and in n."""
    rng = np.random.default_rng(5)
    d = 0.01 + 80.0 * rng.random(20000)
    n = d * 20.0 * rng.random(20000)
    for abx in ABX:
        t = rbe.tissue(model, abx * BETA_X, BETA_X)
        _, fd, fn, a1 = R.forward64(t, d, n)
        hd, hn = 1e-5 * d, 1e-5 * (n + 1.0)
        num_d = (R.forward64(t, d + hd, n)[0] - R.forward64(t, d - hd, n)[0]) / (2.0 * hd)
        num_n = (R.forward64(t, d, n + hn)[0] - R.forward64(t, d, n - hn)[0]) / (2.0 * hn)
        assert np.all(np.abs(num_d - fd) <= 1e-6 * np.abs(fd)), float((np.abs(num_d - fd) / np.abs(fd)).max())
        assert np.all(np.abs(num_n - fn) <= 1e-6 * (abs(a1) + np.abs(fn))), float(np.abs(num_n - fn).max())


def test_monotone_in_dose_and_in_let():
    """R rises with d at fixed LETd for every model, and with LETd at fixed d for wedenberg."""
    d = np.linspace(0.0, 80.0, 4001)
    for model in rbe.MODELS:
        for abx in ABX:
            t = rbe.tissue(model, abx * BETA_X, BETA_X)
            for letd in (0.0, 1.0, 5.0, 20.0):
                r = R.forward64(t, d, d * letd)[0]
                assert np.all(np.diff(r) > 0), (model, abx, letd)
    letd = np.linspace(0.0, 20.0, 2001)
    for abx in ABX:
        t = rbe.tissue("wedenberg", abx * BETA_X, BETA_X)
        for dv in (0.1, 2.0, 60.0):
            assert np.all(np.diff(R.forward64(t, dv, dv * letd)[0]) > 0), (abx, dv)


def test_host_coefficients_are_float64_products_rounded_once():
    t = rbe.tissue("mcnamara", 0.1, 0.05)
    assert C_sizeof(t) == 32
    c = R.coefficients(t)
    ax, bx = np.float64(F(0.1)), np.float64(F(0.05))
    mx, mn = [np.float64(F(v)) for v in t.rbe_max], [np.float64(F(v)) for v in t.rbe_min]
    want = [F(ax * mx[0]), F(ax * mx[1]), F(np.sqrt(bx) * mn[0]), F(np.sqrt(bx) * mn[1]), F(0.1), F(0.05)]
    assert c.dtype == F and np.array_equal(c.view(np.uint32), np.array(want, dtype=F).view(np.uint32))
    # ... which is not always the float32 product of the float32 fields (that would round twice)
    many = np.random.default_rng(1).random(20000).astype(F)
    twice = (many * F(0.3)).astype(F)
    once = (many.astype(np.float64) * np.float64(F(0.3))).astype(F)
    assert np.array_equal(twice, once)                                 # a single product IS rounded once either way ...
    sb32 = (np.sqrt(many).astype(F) * F(0.3)).astype(F)
    sb64 = (np.sqrt(many.astype(np.float64)) * np.float64(F(0.3))).astype(F)
    assert not np.array_equal(sb32, sb64)                              # ... the square root in float32 first is not


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


def test_object_rules():
    """Class 0 everywhere; later assignments overwrite; bool masks and index arrays; the box leaves the outside alone; e < 0 and NaN give
    R = fd = fn = 0; e == 0 takes the formulas (k = 1 / alpha_x)."""
    dims = (7, 5, 3)
    t0, t1, t2 = rbe.tissue("wedenberg", 0.5, 0.05), rbe.tissue("mcnamara", 0.1, 0.05), rbe.tissue("constant", 0.1, 0.05)
    o = R.Rbe(dims, t0)
    assert o.add_tissue(t1) == 1 and o.add_tissue(t2) == 2
    a = np.zeros((3, 5, 7), dtype=bool)
    a[:, 1:4, 2:6] = True
    o.assign(a.reshape(-1), 1)
    idx = np.flatnonzero(a.reshape(-1))[::2]
    o.assign(idx, 2)
    want = np.zeros(105, dtype=np.uint8)
    want[a.reshape(-1)] = 1
    want[idx] = 2
    assert np.array_equal(o.classes, want) and set(np.unique(want)) == {0, 1, 2}
    rng = np.random.default_rng(3)
    d = (10.0 * rng.random(105)).astype(F)
    n = (d * 5.0).astype(F)
    d[0], n[0] = 0.0, 0.0
    n[1] = -1e6                                                        # e < 0
    n[2] = np.nan
    out0 = np.full(105, F(-7.5))
    box = ((1, 0, 1), (5, 4, 2))
    got = o.dose(d, n, out0, box)
    m = o.box_mask(box)
    assert m.sum() == 5 * 5 * 2 and np.all(got[~m] == F(-7.5)) and np.all(got[m] > 0)
    full = o.dose(d, n, out0)
    assert full[0] == 0 and full[1] == 0 and full[2] == 0 and np.all(full[3:] > 0)
    for cls in (0, 1, 2):
        sel = (want == cls) & (np.arange(105) > 2)
        assert np.array_equal(full[sel], R.forward(o.table[cls], d[sel], n[sel]))
    g = np.ones(105, dtype=F)
    gd, gn = o.backward(d, n, g, np.zeros(105, dtype=F), np.zeros(105, dtype=F))
    assert gd[1] == 0 and gn[1] == 0 and gd[2] == 0 and gn[2] == 0
    c0 = o.table[0]
    assert gd[0] == (F(1.0) / np.sqrt(c0[4] * c0[4])) * c0[0] and gd[0] > 0      # e == 0: k = 1 / alpha_x, a gradient without dose
    assert abi.RTD_RBE_MAX_CLASSES == 256
