"""The named variable-RBE models as tissues of the C ABI (include/rtd.h "Variable-RBE dose"). The ABI takes six
numbers per tissue class: photon alpha_x (1/Gy) and beta_x (1/Gy^2) and the two lines RBEmax = rbe_max[0] + rbe_max[1] * LETd,
RBEmin = rbe_min[0] + rbe_min[1] * LETd (LETd in keV/um). The models here are the phenomenological LQ models that are linear in LETd."""
import math

from . import abi

MODELS = ("constant", "mcnamara", "wedenberg", "carabe")


def lines(model, alpha_x, beta_x):
    """-> (rbe_max[2], rbe_min[2]) as Python floats (float64), with abx = alpha_x / beta_x in Gy."""
    alpha_x, beta_x = float(alpha_x), float(beta_x)
    if not (alpha_x > 0.0 and beta_x > 0.0 and math.isfinite(alpha_x) and math.isfinite(beta_x)):
        raise ValueError("alpha_x and beta_x must be positive and finite, not %r and %r" % (alpha_x, beta_x))
    abx = alpha_x / beta_x
    if model == "constant":        # the clinical 1.1
        return (1.1, 0.0), (1.1, 0.0)
    if model == "mcnamara":        # McNamara, Schuemann, Paganetti 2015
        return (0.99064, 0.35605 / abx), (1.1012, -0.0038703 * math.sqrt(abx))
    if model == "wedenberg":       # Wedenberg, Lind, Hardemark 2013
        return (1.0, 0.434 / abx), (1.0, 0.0)
    if model == "carabe":          # Carabe, Moteabbed, Depauw, Schuemann, Paganetti 2012
        return (0.843, 0.154 * 2.686 / abx), (1.09, 0.006 * 2.686 / abx)
    raise ValueError("unknown RBE model %r (one of %s)" % (model, ", ".join(MODELS)))


def tissue(model, alpha_x, beta_x):
    """The abi.RtdRbeTissue of a named model for a tissue with photon parameters alpha_x (1/Gy) and beta_x (1/Gy^2)."""
    mx, mn = lines(model, alpha_x, beta_x)
    t = abi.RtdRbeTissue()
    t.alpha_x, t.beta_x = float(alpha_x), float(beta_x)
    for i in range(2):
        t.rbe_max[i] = mx[i]
        t.rbe_min[i] = mn[i]
    return t
