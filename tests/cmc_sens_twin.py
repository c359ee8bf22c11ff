"""
CPU twin of the conditional estimator's parameter sensitivities on common random numbers (csrc/svmc_cmc.hip cond_sens_jobs_kernel /
cond_sens_pairs_kernel / cond_sens_finish_kernel; include/svmc.h), shared by tests/test_cmc_sens_host.py and
tests/test_gpu_cmc_sens.py.  numpy.longdouble on cmc_twin's keep rule, normal CDF and Black-76 price and cmc_greeks_twin's dual
delta; the keep decisions are taken in double.

Per job j in (up, dn): e = exp(mu + cv / 2), c_j = mean_kept_j(e) - 1 (0 without recentring), K'_j = K + F c_j, q_j = mean_kept_j(B_k).
A pair (path i) is kept iff the path is kept in both jobs:
    d_i = B_i^up - B_i^dn,   sens = DF mean_pairs(d) / (2 h)
    dt_i = d_i + F (q_up (e_i^up - 1) - q_dn (e_i^dn - 1)) with recentring, d_i without
    error = DF x population deviation over the pairs of dt / sqrt(n) / (2 h)
sums of value_i - value_path0 (0 where path 0 is not a kept pair); no kept pair: NaN, NaN, 0.
"""
import numpy as np

import cmc_greeks_twin as gt
import cmc_twin as ct

LD = np.longdouble


def job_terms(mu, cv, forward, recenter):
    """(keep mask, and on ALL paths -- garbage where dropped -- e, fc, ln_fc, cv in long double; c_j)"""
    mu, cv = np.asarray(mu, dtype=np.float64), np.asarray(cv, dtype=np.float64)
    keep = ct.keep_mask(mu, cv)
    with np.errstate(all="ignore"):
        m_, c_ = np.where(keep, mu, 0.0).astype(LD), np.where(keep, cv, 0.0).astype(LD)
        h = m_ + c_ / 2
        e = np.exp(h)
    F = LD(forward)
    if keep.any():
        first = e[keep][0]
        mean_e = first + (e[keep] - first).mean()
    else:
        mean_e = LD(np.nan)
    c = (mean_e - 1) if recenter else LD(0)
    return keep, e, F * e, np.log(F) + h, c_, c


def estimator(mu_up, cv_up, mu_dn, cv_dn, step, forward, strikes, types, discfactor=1.0, recenter=True, mutate=None):
    """(sens [K], sens_stderr [K], n_pairs [K]) of include/svmc.h's sensitivity estimator for ONE parameter and ONE expiry;
    mutate="d_only": the error from the deviation of d alone (the delta-method term dropped), for tests/test_cmc_sens_host.py"""
    n = np.asarray(mu_up).size
    F, DF, h2 = LD(forward), LD(discfactor), 2 * LD(step)
    ku, eu, fcu, lfu, cvu, cu = job_terms(mu_up, cv_up, forward, recenter)
    kd, ed, fcd, lfd, cvd, cd = job_terms(mu_dn, cv_dn, forward, recenter)
    pair = ku & kd
    n_pairs = int(pair.sum())
    sens, errs = [], []
    for k, t in zip(np.asarray(strikes, dtype=np.float64).ravel(), np.asarray(types).ravel()):
        put = str(t) == "P"
        kpu, kpd = LD(k) + F * cu, LD(k) + F * cd
        if n_pairs == 0:
            sens.append(np.nan), errs.append(np.nan)
            continue
        with np.errstate(all="ignore"):
            bu = ct.black_l(fcu, lfu, cvu, kpu, put)
            bd = ct.black_l(fcd, lfd, cvd, kpd, put)
            d = (bu - bd)[pair]
            dt = d
            if recenter and mutate != "d_only":
                qu = gt.path_terms(eu[ku], fcu[ku], lfu[ku], cvu[ku], kpu, put, cu)[1].mean()
                qd = gt.path_terms(ed[kd], fcd[kd], lfd[kd], cvd[kd], kpd, put, cd)[1].mean()
                dt = d + F * (qu * (eu[pair] - 1) - qd * (ed[pair] - 1))
        sh_d, sh_t = (d[0], dt[0]) if pair[0] else (LD(0), LD(0))
        sens.append(float(DF * (sh_d + (d - sh_d).mean()) / h2))
        errs.append(float(DF * (dt - sh_t).std() / np.sqrt(LD(n)) / h2))
    return np.array(sens), np.array(errs), np.full(len(sens), n_pairs, dtype=np.int64)


# ---- the toy model of DESIGN.md row f14: a lognormal volatility at one date, the return Gaussian given it -------------------------
TOY_SIGMA, TOY_BUMP, TOY_T, TOY_PATHS = 0.8, 8e-4, 0.25, 4096


def toy_jobs(seed, rho, n=TOY_PATHS):
    """(mu_up, cv_up, mu_dn, cv_dn) of the toy model on ONE draw b ~ N(0, 1): sigma = (0.8 +- 8e-4) exp(b / 2 - 1 / 8),
    cv = (1 - rho^2) sigma^2 T, mu = -sigma^2 T / 2 + rho sigma sqrt(T) b"""
    b = np.random.default_rng(seed).standard_normal(n)
    out = []
    for s0 in (TOY_SIGMA + TOY_BUMP, TOY_SIGMA - TOY_BUMP):
        sigma = s0 * np.exp(b / 2 - 0.125)
        out += [-0.5 * sigma * sigma * TOY_T + rho * sigma * np.sqrt(TOY_T) * b, (1 - rho * rho) * sigma * sigma * TOY_T]
    return out
