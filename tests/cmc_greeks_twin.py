"""
CPU twin of the conditional Monte Carlo Greeks (csrc/svmc_cmc.hip cond_deriv_kernel / cond_deriv_finish_kernel; include/svmc.h,
DESIGN.md row f13), shared by tests/test_cmc_greeks_host.py and tests/test_gpu_cmc_greeks.py.  numpy.longdouble on cmc_twin's
keep rule, normal CDF and Black-76 price; the keep decisions are taken in double.

Per kept path, s = +1 call / -1 put, e = exp(mu + cv / 2), F_c = F e, c = mean_kept(e) - 1 (0 without recentring), K' = K + F c:
    d1 = (ln F_c - ln K') / sd + sd / 2, d2 = d1 - sd, sd = sqrt(cv)
    B_f = N(d1) | N(d1) - 1,  B_k = -N(d2) | N(-d2)
    delta = e B_f + c B_k,  dual_delta = B_k,  dual_gamma = phi(d2) / (K' sd),  gamma = (K / F)^2 dual_gamma
    cv == 0: B_f = s 1{s (F_c - K') > 0}, B_k = -B_f, gammas 0;   K' <= 0: call (1, -1), put (0, 0), gammas 0
value = DF mean_kept, error = DF x population deviation over the kept paths / sqrt(n); sums of value_i - shift, shift = path 0's value
or, where path 0 is dropped, the value at (mu, cv) = (0, 0).
"""
import numpy as np

import cmc_twin as ct

LD = np.longdouble
FIELDS = ("price", "stderr", "delta", "delta_stderr", "dual_delta", "dual_delta_stderr", "gamma", "gamma_stderr", "dual_gamma",
          "dual_gamma_stderr")
SQRT_2PI = np.sqrt(2 * LD(np.pi))


def path_terms(e, fc, ln_fc, cv, kp, put, c, mutate=None):
    """per path (delta_i, dual_delta_i, dual_gamma_i) against the scalar strike kp; mutate="no_c_bk" drops c B_k from delta"""
    zero = np.zeros_like(fc)
    if not kp > 0:
        bf = zero if put else zero + 1
        bk = -bf
        dg = zero
    else:
        s = -1 if put else 1
        pos = cv > 0
        sd = np.sqrt(np.where(pos, cv, LD(1)))
        d1 = (ln_fc - np.log(LD(kp))) / sd + sd / 2
        d2 = d1 - sd
        bf_pos = -ct.ndtr_l(-d1) if put else ct.ndtr_l(d1)
        bk_pos = ct.ndtr_l(-d2) if put else -ct.ndtr_l(d2)
        itm = np.where(s * (fc - kp) > 0, LD(s), LD(0))
        bf = np.where(pos, bf_pos, itm)
        bk = np.where(pos, bk_pos, -itm)
        dg = np.where(pos, np.exp(-d2 * d2 / 2) / SQRT_2PI / (kp * sd), LD(0))
    delta = e * bf + (0 if mutate == "no_c_bk" else c * bk)
    return delta, bk, dg


def estimator(mu, cv, forward, strikes, types, discfactor=1.0, recenter=True, mutate=None):
    """({field of FIELDS: [K] float64}, stats dict with n_zero_cv) of include/svmc.h's conditional Greeks; mutate: a deliberate
    error for tests/test_cmc_greeks_host.py -- "no_c_bk" | "kp_in_gamma_factor" """
    mu, cv = np.asarray(mu, dtype=np.float64), np.asarray(cv, dtype=np.float64)
    n = mu.size
    keep = ct.keep_mask(mu, cv)
    prices, errs, stats = ct.estimator(mu, cv, forward, strikes, types, discfactor, recenter)
    m_, c_ = mu[keep].astype(LD), cv[keep].astype(LD)
    h = m_ + c_ / 2
    e = np.exp(h)
    F, DF = LD(forward), LD(discfactor)
    fc, ln_fc = F * e, np.log(F) + h
    n_kept = int(keep.sum())
    mean_e = (e[0] + (e - e[0]).mean()) if n_kept else LD(np.nan)
    c = (mean_e - 1) if recenter else LD(0)
    first_kept = bool(keep[0]) if n else False
    out = {f: [] for f in FIELDS}
    for k, t in zip(np.asarray(strikes, dtype=np.float64).ravel(), np.asarray(types).ravel()):
        put = str(t) == "P"
        kp = LD(k) + F * c
        terms = path_terms(e, fc, ln_fc, c_, kp, put, c, mutate)
        if first_kept:
            shift = [v[0] for v in terms]
        else:                                                  # the value at (mu, cv) = (0, 0)
            one = np.ones(1, dtype=LD)
            shift = [v[0] for v in path_terms(one, F * one, np.log(F) * one, 0 * one, kp, put, c, mutate)]
        vals = []
        for v, sh in zip(terms, shift):
            if n_kept:
                d = v - sh
                vals.append((DF * (sh + d.mean()), DF * d.std() / np.sqrt(LD(n))))
            else:
                vals.append((LD(np.nan), LD(np.nan)))
        r2 = ((kp if mutate == "kp_in_gamma_factor" else LD(k)) / F) ** 2
        for name, (v, s) in zip(("delta", "dual_delta", "dual_gamma"), vals):
            out[name].append(float(v))
            out[name + "_stderr"].append(float(s))
        out["gamma"].append(float(r2 * vals[2][0]))
        out["gamma_stderr"].append(float(r2 * vals[2][1]))
    out["price"], out["stderr"] = list(prices), list(errs)
    stats = dict(stats, n_zero_cv=int(np.sum(cv[keep] == 0.0)))
    return {f: np.array(v, dtype=np.float64) for f, v in out.items()}, stats


def log_return_pdf(mu, cv, x_grid, recenter=False):
    """the density composition of get_log_return_mc_pdf_conditional on host (mu, cv): calls at K_j = exp(x_j), F = DF = 1"""
    strikes = np.exp(np.asarray(x_grid, dtype=np.float64))
    g, stats = estimator(mu, cv, 1.0, strikes, ["C"] * strikes.size, 1.0, recenter)
    return strikes * g["dual_gamma"], strikes * g["dual_gamma_stderr"], stats
