"""
CPU twin of the conditional Monte Carlo estimator under the exponential risk-premia kernel (include/svmc_ext.h, DESIGN.md row f17;
csrc/svmc_ext.hip), shared by tests/test_tilted_cond_host.py and tests/test_gpu_tilted_cond.py.

The estimator as the header states it, in numpy.longdouble with the keep decisions taken in double; Black-76 and the normal CDF as
tests/cmc_twin.py evaluates them (black_l, ndtr_l, keep_mask).  Given a path's conditioning variables x ~ N(mu, cv), and
    E[e^{gamma x} g(x)] = e^{gamma mu + gamma^2 cv / 2} E[g(y)],   y ~ N(mu + gamma cv, cv)          (Esscher)
so a path contributes the weight W = exp(gamma mu + gamma^2 cv / 2) times the Black-76 price of F_t = F exp(mu + (gamma + 1/2) cv).
shift_forward=False leaves the gamma cv out of the forward: the deliberate error tests/test_tilted_cond_host.py must see.
"""
import numpy as np

import cmc_twin as ct

LD = np.longdouble
STATS = ("normalizer", "normalizer_stderr", "gamma_forward", "gamma_forward_stderr", "effective_sample_size", "n_kept", "n_dropped",
         "sum_weights")


def keep_mask(mu, cv, forward, gamma):
    """the keep rule, decided in double: f11's rule (cmc_twin.keep_mask) and W^2, (W F_t)^2 finite"""
    mu, cv = np.asarray(mu, dtype=np.float64), np.asarray(cv, dtype=np.float64)
    with np.errstate(all="ignore"):
        w = np.exp(gamma * mu + (0.5 * gamma * gamma) * cv)
        ft = forward * np.exp(mu + (gamma + 0.5) * cv)
        return ct.keep_mask(mu, cv) & np.isfinite(w * w) & np.isfinite((w * ft) ** 2)


def corr_of(mu, cv, forward, recenter):
    """f11's recentring in long double: mean(F e) - F over the paths f11 keeps (cmc_twin.estimator's expression), 0 without it"""
    if not recenter:
        return LD(0)
    keep = ct.keep_mask(mu, cv)
    if not keep.any():
        return LD(np.nan)
    e = np.exp(np.asarray(mu, dtype=np.float64)[keep].astype(LD) + np.asarray(cv, dtype=np.float64)[keep].astype(LD) / 2)
    return LD(forward) * (e[0] + (e - e[0]).mean()) - LD(forward)


def path_terms(mu, cv, forward, strike, put, gamma, corr=0.0, shift_forward=True):
    """(W, F_t, B) per path in long double for the scalar strike: the weight, the shifted forward and the Black-76 price against
    K' = strike + corr"""
    m, c = np.asarray(mu, dtype=np.float64).astype(LD), np.asarray(cv, dtype=np.float64).astype(LD)
    g, F = LD(gamma), LD(forward)
    w = np.exp(g * m + g * g * c / 2)
    lr = m + ((g if shift_forward else LD(0)) + LD(0.5)) * c
    ft, ln_ft = F * np.exp(lr), np.log(F) + lr
    return w, ft, ct.black_l(ft, ln_ft, c, LD(strike) + LD(corr), put)


def estimator(mu, cv, forward, strikes, types, gamma, recenter=False, shift_forward=True):
    """(prices [K], stderrs [K], stats dict of STATS and "corr") of include/svmc_ext.h's estimator; types: 'C' | 'P' per strike"""
    mu, cv = np.asarray(mu, dtype=np.float64).ravel(), np.asarray(cv, dtype=np.float64).ravel()
    n = mu.size
    corr = corr_of(mu, cv, forward, recenter)
    keep = keep_mask(mu, cv, forward, gamma)
    n_kept = int(keep.sum())
    m, c = mu[keep], cv[keep]
    prices, errs = [], []
    with np.errstate(all="ignore"):
        w, ft, _ = path_terms(m, c, forward, 1.0, False, gamma, 0.0, shift_forward)
        W = w.sum() if n_kept else LD(0)
        cl, ln_ft = c.astype(LD), np.log(ft)
        for k, t in zip(np.asarray(strikes, dtype=np.float64).ravel(), np.asarray(types).ravel()):
            b = ct.black_l(ft, ln_ft, cl, LD(k) + corr, str(t) == "P")
            price = (w * b).sum() / W if n_kept else LD(np.nan)
            prices.append(price)
            errs.append(np.sqrt(((w * (b - price)) ** 2).sum()) / W if n_kept else LD(np.nan))
        N = LD(n_kept) / W
        spot = ft - corr
        gf = (w * spot).sum() / W if n_kept else LD(np.nan)
        stats = dict(normalizer=N, normalizer_stderr=np.sqrt(((1 - N * w) ** 2).sum()) / W, gamma_forward=gf,
                     gamma_forward_stderr=np.sqrt(((w * (spot - gf)) ** 2).sum()) / W,
                     effective_sample_size=W * W / (w * w).sum() if n_kept else LD(np.nan), n_kept=n_kept, n_dropped=n - n_kept,
                     sum_weights=W, corr=corr)
    return np.array(prices, dtype=LD), np.array(errs, dtype=LD), stats


def plain_tilted(x, forward, strikes, types, gamma, corr=0.0):
    """the plain estimator under the kernel (include/svmc.h row f8) on terminal log-returns x, long double: (prices, stderrs, stats)"""
    xl = np.asarray(x, dtype=np.float64).astype(LD)
    w = np.exp(LD(gamma) * xl)
    spot = LD(forward) * np.exp(xl) - LD(corr)
    W = w.sum()
    sg = np.where(np.asarray(types).ravel() == "C", 1.0, -1.0).astype(LD)
    pay = np.maximum(sg[None, :] * (spot[:, None] - np.asarray(strikes, dtype=np.float64).ravel().astype(LD)[None, :]), LD(0))
    price = (w[:, None] * pay).sum(axis=0) / W
    err = np.sqrt(((w[:, None] * (pay - price[None, :])) ** 2).sum(axis=0)) / W
    N = LD(xl.size) / W
    gf = (w * spot).sum() / W
    stats = dict(normalizer=float(N), normalizer_stderr=float(np.sqrt(((1 - N * w) ** 2).sum()) / W), gamma_forward=float(gf),
                 gamma_forward_stderr=float(np.sqrt(((w * (spot - gf)) ** 2).sum()) / W), effective_sample_size=float(W * W / (w * w).sum()))
    return price.astype(np.float64), err.astype(np.float64), stats
