"""fp64 restatement of the guided mix of DESIGN.md §3.8 (mg_cfg_stats_f32, mg_cfg_coef_f32, mg_cfg_combine_coef_f32), for tests/test_guidance.py.
Plain Python floats (IEEE fp64, one rounding per operation, no contraction); the sums are np.longdouble (wider than fp64) of the exact
fp64 terms."""
import math

import numpy as np


def stats_terms(u, c):
    """u, c: fp32 arrays -> the five fp64 term arrays (u, c, u^2, c^2, u c); every product of two fp32 values is exact in fp64"""
    u, c = np.asarray(u, dtype=np.float64).ravel(), np.asarray(c, dtype=np.float64).ravel()
    return u, c, u * u, c * c, u * c


def stats_ref(u, c):
    """-> (sums [5] as np.longdouble, sum |terms| [5] as float): the reference of cfg_stats and the scale of its error bound"""
    terms = stats_terms(u, c)
    return [t.astype(np.longdouble).sum() for t in terms], [float(np.abs(t).astype(np.longdouble).sum()) for t in terms]


def variances(stats, n, au, ac):
    """(var_p, var_c) of p = au u + ac c and of c, from the five sums over n elements"""
    Su, Sc, Suu, Scc, Suc = (float(v) for v in stats)
    n = float(n)
    mp = (au * Su + ac * Sc) / n
    ep = (au * au * Suu + 2.0 * au * ac * Suc + ac * ac * Scc) / n
    mc = Sc / n
    return ep - mp * mp, Scc / n - mc * mc


def coef_ref(stats, n, g, zero_star, rescale):
    """-> (a_u, a_c) in fp64, before the rounding to fp32.  g and rescale are the fp32 values the C ABI carries."""
    Su, Sc, Suu, Scc, Suc = (float(v) for v in stats)
    g, rescale = float(np.float32(g)), float(np.float32(rescale))
    s = Suc / (Suu + 1e-8) if zero_star else 1.0
    au, ac = s * (1.0 - g), g
    if rescale > 0.0:
        varp, varc = variances(stats, n, au, ac)
        f = 1.0
        if varp > 0.0 and varc >= 0.0:
            f = rescale * math.sqrt(varc / varp) + (1.0 - rescale)
        au, ac = au * f, ac * f
    return au, ac


def combine_ref(u, c, au, ac):
    """a_u u + a_c c in fp64"""
    return au * np.asarray(u, dtype=np.float64) + ac * np.asarray(c, dtype=np.float64)
