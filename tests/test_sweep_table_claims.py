"""Host-side checks of the two exactness claims k_superpose_sweep's table build (rtd_sweep.hpp swBuildT) rests on:

  * an erf lane (1/sigma > 0.75) has entry i >= 6 exactly +0: both arguments r (i -+ 0.5) of swErf are >= 4.125, where swErf clamps
    (fminf(t, 4)) and selects its second branch, so erfNew == erfOld bit for bit and 0.5 * (erfNew - erfOld) * w = +0;
  * a dead lane (no dose: w = +0, r = 1/4) stores its series entries unmasked: they are +0 because the series factor is positive.

swErf is evaluated in float32 with numpy, its fused multiply-adds as a float64 product and sum rounded once to float32 — not always
the device's bits, but both sides of each comparison go through the same arithmetic, which is what the claims are about."""
import numpy as np

f32 = np.float32


def _fma(a, b, c):
    return f32(np.float64(a) * np.float64(b) + np.float64(c))


def sw_erf(t):
    """rtd_sweep.hpp swErf, operation by operation."""
    t = f32(t)
    s2 = f32(t * t)
    r = f32(8.694667811e-05)
    for c in (-8.215559851e-04, 5.207134257e-03, -2.686173980e-02, 1.128373582e-01, -3.761263625e-01, 1.283791669e-01):
        r = _fma(r, s2, f32(c))
    small = _fma(r, t, t)
    u = f32(f32(np.fmin(t, f32(4.0))) - f32(0.875))
    p = f32(-3.116289875e-08)
    for c in (2.754377229e-06, -5.187475768e-05, 5.094422115e-04, -3.331390714e-03, 1.650326662e-02, -6.772692889e-02,
              -1.192432172e+00, -3.506067286e+00, -2.211398194e+00):
        p = _fma(p, u, f32(c))
    big = f32(f32(1.0) - f32(np.exp2(p)))
    return small if t < f32(0.875) else big


def _erf_lane_rs():
    lo = np.nextafter(f32(0.75), f32(np.inf))
    rs = [lo, np.nextafter(lo, f32(np.inf)), f32(0.7500001), f32(0.76), f32(0.8), f32(1.0), f32(1.5), f32(3.0), f32(17.0),
          f32(1e4), f32(3e38), f32(np.inf), f32(np.nan)]
    rs += list(np.geomspace(0.75, 100.0, 2000, dtype=np.float32)[1:])
    return rs


@np.errstate(over="ignore", invalid="ignore")                          # (1/sigma = 3e38, inf, NaN: the arguments overflow)
def test_erf_entries_from_six_on_are_exact_zeros():
    for r in _erf_lane_rs():
        assert not (r <= f32(0.75))                                   # an erf lane (swBuild's `series` is false)
        for i in range(6, 17):
            old = sw_erf(f32(r * f32(f32(i - 2) + f32(1.5))))          # the two arguments of entry i as the build forms them
            new = sw_erf(f32(r * f32(f32(i - 1) + f32(1.5))))
            assert np.float32(old).tobytes() == np.float32(new).tobytes(), (r, i)
            for w in (f32(1e-20), f32(0.3), f32(1.0), f32(7e3)):
                e = f32(f32(f32(0.5) * f32(new - old)) * w)
                assert e.tobytes() == f32(0.0).tobytes(), (r, i, w, e)


def test_the_erf_cut_is_not_below_six():
    """At entry 5 the lower argument r * 4.5 stays below the clamp for 1/sigma just above 0.75: entry 5 must still be evaluated."""
    r = np.nextafter(f32(0.75), f32(np.inf))
    assert f32(r * f32(4.5)) < f32(4.0)
    assert sw_erf(f32(r * f32(4.5))) != sw_erf(f32(r * f32(5.5)))


def test_dead_lane_series_entries_are_positive_zeros():
    r = f32(0.25)
    h2 = f32(r * r); h4 = f32(h2 * h2)
    k1 = f32(h2 * f32(1.0 / 24.0)); k2 = f32(h4 * f32(1.0 / 1920.0)); k3 = f32(f32(h4 * h2) * f32(1.0 / 322560.0))
    c0 = f32(f32(f32(f32(1.0) - f32(f32(2.0) * k1)) + f32(f32(12.0) * k2)) - f32(f32(120.0) * k3))
    c1 = f32(f32(f32(f32(4.0) * k1) - f32(f32(48.0) * k2)) + f32(f32(720.0) * k3)) * h2
    c2 = f32(f32(f32(16.0) * k2) - f32(f32(480.0) * k3)) * h4
    c3 = f32(f32(f32(64.0) * k3) * f32(h4 * h2))
    q = f32(np.exp2(f32(f32(-1.4426950409) * h2)))
    assert c0 > 0 and q > 0
    w = f32(0.0)
    gq = f32(f32(f32(0.5641895835) * r) * w)
    cq = f32(q * q)
    gq = f32(gq * q); q = f32(q * cq)
    for i in range(1, 17):
        wi = f32(i * i)
        s = _fma(_fma(_fma(c3, wi, c2), wi, c1), wi, c0)
        assert s > 0, (i, s)
        e = f32(gq * s)
        assert e.tobytes() == f32(0.0).tobytes()
        gq = f32(gq * q); q = f32(q * cq)
