"""
CPU twin of the mixture density of the log-return (include/svmc_est.h; csrc/svmc_est.hip's cond_density_*_kernel),
shared by tests/test_cond_density_host.py and tests/test_gpu_cond_density.py.

Two forms, both numpy.longdouble with the keep decisions taken in double (cmc_twin.keep_mask: f11's rule):
  direct()     the estimator written DIRECTLY, no identity used: a kept path with cv > 0 contributes the Gaussian of its log-return
               under the kernel, v_j = N(x; mu_j + gamma cv_j, cv_j), with the weight W_j = exp(gamma mu_j + gamma^2 cv_j / 2);
                   pdf = sum_j W_j v_j / sum_j W_j,   error = sqrt(sum_j (W_j (v_j - pdf))^2) / sum_j W_j
               -- the sums run over EVERY kept path, a cv == 0 path with v_j = 0;
  sums_form()  the header's statement: S1, S2 (gamma-independent), C, sum W, sum W^2 and e^{gamma x}, formed once.
               mutate= names a deliberate error tests/test_cond_density_host.py must see:
                   "no_cross_term"     the term -2 pdf e^{gamma x} C dropped from the error
                   "sum_w_for_sum_w2"  sum W where sum W^2 belongs
The one deliberate difference from row f18 (tilted_cond_greeks_twin): a gamma at which a kept path's W^2 is not finite in double is
NaN altogether, and its statistics count those paths (n_weight_dropped); the other sums leave them out.
The long-double exponentials are numpy's own (expl), not the double exponential with a first-order correction of
tilted_cond_greeks_twin.phi_l.
"""
import numpy as np

import cmc_twin as ct

LD = np.longdouble
STATS = ("sum_weights", "n_kept", "n_dropped", "n_zero_cv", "n_weight_dropped")
MUTATIONS = ("no_cross_term", "sum_w_for_sum_w2")
SQRT_2PI = np.sqrt(2 * LD(np.pi))


def _rows(mu, cv):
    mu = np.asarray(mu, dtype=np.float64).ravel()
    cv = np.asarray(cv, dtype=np.float64)
    cv = np.full(mu.size, float(cv)) if cv.ndim == 0 else cv.ravel()
    return mu, cv


def weights(mu, cv, gamma):
    """(kept mask of f11's rule, W [kept] long double, weight-dropped mask [kept] decided in double)"""
    mu, cv = _rows(mu, cv)
    keep = ct.keep_mask(mu, cv)
    m, c = mu[keep], cv[keep]
    with np.errstate(all="ignore"):
        wd = np.exp(gamma * m + (0.5 * gamma * gamma) * c)
        bad = ~np.isfinite(wd * wd)
        w = np.exp(LD(gamma) * m.astype(LD) + LD(gamma) * LD(gamma) * c.astype(LD) / 2)
    return keep, w, bad


def stats_of(mu, cv, gamma):
    mu, cv = _rows(mu, cv)
    keep, w, bad = weights(mu, cv, gamma)
    return dict(sum_weights=w[~bad].sum() if (~bad).any() else LD(0), n_kept=int(keep.sum()), n_dropped=int(mu.size - keep.sum()),
                n_zero_cv=int(np.sum(cv[keep] == 0.0)), n_weight_dropped=int(bad.sum()))


def gaussians(mu, cv, x, shift=0.0):
    """N(x; mu_j + shift cv_j, cv_j) per path for the scalar x, long double; 0 where cv == 0"""
    m, c = np.asarray(mu, dtype=np.float64).astype(LD), np.asarray(cv, dtype=np.float64).astype(LD)
    pos = c > 0
    sd = np.sqrt(np.where(pos, c, LD(1)))
    with np.errstate(all="ignore"):
        z = (LD(x) - (m + LD(shift) * c)) / sd
        return np.where(pos, np.exp(-(z * z) / 2) / (sd * SQRT_2PI), LD(0))


def direct(mu, cv, x_grid, gamma):
    """(pdf [P], error [P], stats) -- no identity used.  x_grid may be long double"""
    mu, cv = _rows(mu, cv)
    keep, w, bad = weights(mu, cv, gamma)
    st = stats_of(mu, cv, gamma)
    xs = np.asarray(x_grid).ravel()
    nan = np.full(xs.size, np.nan, dtype=LD)
    if bad.any() or not keep.any():
        return nan, nan.copy(), st
    m, c = mu[keep], cv[keep]
    W = w.sum()
    pdf, err = [], []
    for x in xs:
        v = gaussians(m, c, x, gamma)
        p = (w * v).sum() / W
        pdf.append(p)
        err.append(np.sqrt(((w * (v - p)) ** 2).sum()) / W if keep.sum() > 1 else LD(0))      # one kept path gives error 0
    return np.array(pdf, dtype=LD), np.array(err, dtype=LD), st


def sums_form(mu, cv, x_grid, gamma, mutate=None):
    """(pdf [P], error [P], stats) by the header's sums"""
    assert mutate is None or mutate in MUTATIONS
    mu, cv = _rows(mu, cv)
    keep, w, bad = weights(mu, cv, gamma)
    st = stats_of(mu, cv, gamma)
    xs = np.asarray(x_grid).ravel()
    nan = np.full(xs.size, np.nan, dtype=LD)
    if bad.any() or not keep.any():
        return nan, nan.copy(), st
    m, c = mu[keep], cv[keep]
    W, Q = w.sum(), (w * w).sum()
    if mutate == "sum_w_for_sum_w2":
        Q = W
    pdf, err = [], []
    for x in xs:
        n = gaussians(m, c, x)
        s1, s2, cc = n.sum(), (n * n).sum(), (w * n).sum()
        eg = np.exp(LD(gamma) * LD(x))
        p = eg * s1 / W
        cross = LD(0) if mutate == "no_cross_term" else 2 * p * eg * cc
        var = eg * eg * s2 - cross + p * p * Q if keep.sum() > 1 else LD(0)
        pdf.append(p)
        err.append(np.sqrt(max(var, LD(0))) / W)
    return np.array(pdf, dtype=LD), np.array(err, dtype=LD), st


def condition(mu, cv, x_grid, gamma):
    """per point, the condition of the identity W_j N(x; mu_j + gamma cv_j, cv_j) = e^{gamma x} N(x; mu_j, cv_j) in extended precision:
    1 + |gamma| max|mu| + gamma^2 max cv / 2 + |gamma x| + z^2 / 2 -- the magnitudes of the exponents that are rounded before they are
    exponentiated, on either side.  z^2 / 2 is a path's; a sum's is the mean of z_j^2 / 2 under the terms' own weights W_j v_j (the
    error's: their squares; the larger of the two is taken), since a sum's relative error is the terms' relative errors averaged with
    the terms as weights."""
    mu, cv = _rows(mu, cv)
    keep, w, _ = weights(mu, cv, gamma)
    m, c = mu[keep], cv[keep]
    out = []
    for x in np.asarray(x_grid).ravel():
        pos = c > 0
        n = gaussians(m, c, x)
        z2 = np.where(pos, (LD(x) - m.astype(LD)) ** 2 / np.where(pos, c, 1.0).astype(LD), LD(0)) / 2
        t = w * n
        zz = max(float((u * z2).sum() / u.sum()) if u.sum() > 0 else 0.0 for u in (t, t * t))     # a value's terms, an error's squares
        out.append(1.0 + abs(gamma) * float(np.max(np.abs(m), initial=0.0)) + gamma * gamma * float(np.max(c, initial=0.0)) / 2
                   + abs(gamma * float(x)) + zz)
    return np.array(out)
