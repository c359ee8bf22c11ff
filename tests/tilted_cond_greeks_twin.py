"""
CPU twin of the conditional Monte Carlo Greeks under the exponential risk-premia kernel (include/svmc_est.h, DESIGN.md row f18;
csrc/svmc_est.hip), shared by tests/test_tilted_cond_greeks_host.py and tests/test_gpu_tilted_cond_greeks.py.

The estimator as the header states it, in numpy.longdouble on tilted_cond_twin's keep rule, weight, shifted forward and recentring
and on cmc_twin's normal CDF; the keep decisions are taken in double.  Per kept path, s = +1 call / -1 put:
    W = exp(gamma mu + gamma^2 cv / 2),  e_t = exp(mu + (gamma + 1/2) cv),  F_t = F e_t,  c = corr / F,  K' = K + corr
    d1 = (ln F_t - ln K') / sd + sd / 2, d2 = d1 - sd, sd = sqrt(cv)
    B_f = N(d1) | N(d1) - 1,  B_k = -N(d2) | N(-d2)
    delta = e_t B_f + c B_k,  dual_delta = B_k,  dual_gamma = phi(d2) / (K' sd),  gamma = (K / F)^2 dual_gamma
    cv == 0: B_f = s 1{s (F_t - K') > 0}, B_k = -B_f, gammas 0;   K' <= 0: call (1, -1), put (0, 0), gammas 0
    value = sum W v / sum W,  error = sqrt(sum (W (v - value))^2) / sum W
mutate= names a deliberate error tests/test_tilted_cond_greeks_host.py must see:
    "no_c_bk"            c B_k dropped from delta
    "no_forward_shift"   the forward's shift gamma cv left out
    "d1_in_dual_gamma"   phi(d1) where phi(d2) belongs
    "unweighted_error"   the error of an unweighted mean: population deviation / sqrt(n_kept)
"""
import numpy as np

import cmc_twin as ct
import tilted_cond_twin as tc

LD = np.longdouble
FIELDS = ("price", "stderr", "delta", "delta_stderr", "dual_delta", "dual_delta_stderr", "gamma", "gamma_stderr", "dual_gamma",
          "dual_gamma_stderr")
QUANTITIES = ("delta", "dual_delta", "gamma", "dual_gamma")
STATS = ("sum_weights", "n_kept", "n_dropped", "n_zero_cv")
MUTATIONS = ("no_c_bk", "no_forward_shift", "d1_in_dual_gamma", "unweighted_error")
SQRT_2PI = np.sqrt(2 * LD(np.pi))


def path_head(mu, cv, forward, gamma, mutate=None):
    """what a path forms once per gamma, long double: (W, e_t, F_t, ln F_t, cv)"""
    m, c_ = np.asarray(mu, dtype=np.float64).astype(LD), np.asarray(cv, dtype=np.float64).astype(LD)
    g, F = LD(gamma), LD(forward)
    w = np.exp(g * m + g * g * c_ / 2)
    lr = m + ((LD(0) if mutate == "no_forward_shift" else g) + LD(0.5)) * c_
    et = np.exp(lr)
    return w, et, F * et, np.log(F) + lr, c_


def phi_l(x):
    """the normal density for long-double x: the exponent -x^2 / 2 in long double, the exponential at its nearest double times the
    first-order term for the remainder (cmc_twin.ndtr_l's device: a long-double exp costs twenty multiplications)"""
    a = -(x * x) / 2
    ad = np.asarray(a, dtype=np.float64)
    return np.exp(ad).astype(LD) * (1 + (a - ad.astype(LD))) / SQRT_2PI


def strike_terms(head, forward, strike, put, corr=0.0, mutate=None):
    """(delta_j, dual_delta_j, dual_gamma_j) per path for the scalar strike, K' = strike + corr, c = corr / forward"""
    _, et, ft, ln_ft, c_ = head
    kp, c = LD(strike) + LD(corr), LD(corr) / LD(forward)
    zero = np.zeros_like(ft)
    if not kp > 0:
        bf = zero if put else zero + 1
        bk = -bf
        dg = zero
    else:
        s = -1 if put else 1
        pos = c_ > 0
        sd = np.sqrt(np.where(pos, c_, LD(1)))
        d1 = (ln_ft - np.log(kp)) / sd + sd / 2
        d2 = d1 - sd
        itm = np.where(s * (ft - kp) > 0, LD(s), LD(0))
        bf = np.where(pos, -ct.ndtr_l(-d1) if put else ct.ndtr_l(d1), itm)
        bk = np.where(pos, ct.ndtr_l(-d2) if put else -ct.ndtr_l(d2), -itm)
        dd = d1 if mutate == "d1_in_dual_gamma" else d2
        dg = np.where(pos, phi_l(dd) / (kp * sd), LD(0))
    delta = et * bf + (0 if mutate == "no_c_bk" else c * bk)
    return delta, bk, dg


def path_terms(mu, cv, forward, strike, put, gamma, corr=0.0, mutate=None):
    """(W, delta_j, dual_delta_j, dual_gamma_j) per path in long double for the scalar strike"""
    head = path_head(mu, cv, forward, gamma, mutate)
    return (head[0],) + strike_terms(head, forward, strike, put, corr, mutate)


def host_shift(forward, strike, put):
    """the host constant of a quote's sums (include/svmc_est.h): s 1{s (F - K) > 0} for delta, its negative for dual delta"""
    s = -1.0 if put else 1.0
    return s if s * (forward - strike) > 0.0 else 0.0


def estimator(mu, cv, forward, strikes, types, gamma, recenter=False, mutate=None, with_price=True):
    """({field of FIELDS: [K] long double}, stats dict of STATS, "corr" and "error_conditioning") of include/svmc_est.h's estimator
    with row f17's price and error (tilted_cond_twin.estimator; left out with with_price=False); types: 'C' | 'P' per strike.
    error_conditioning: {quantity: [K]} -- sum (W d)^2 / sum (W (v - value))^2 with d = v - shift, the header's host shifts: how many
    times larger than their difference the sums are that the device forms an error from.  1 where the shift is the value; large
    where every kept path lies on the other side of the strike than the forward does, or where one weight dominates; inf where the
    error is 0"""
    mu, cv = np.asarray(mu, dtype=np.float64).ravel(), np.asarray(cv, dtype=np.float64).ravel()
    n = mu.size
    shift_forward = mutate != "no_forward_shift"
    prices, errs = [], []
    if with_price:
        prices, errs, _ = tc.estimator(mu, cv, forward, strikes, types, gamma, recenter, shift_forward)
    corr = tc.corr_of(mu, cv, forward, recenter)
    keep = tc.keep_mask(mu, cv, forward, gamma)
    n_kept = int(keep.sum())
    m_, c_ = mu[keep], cv[keep]
    out = {f: [] for f in FIELDS}
    cond = {q: [] for q in QUANTITIES}
    with np.errstate(all="ignore"):
        head = path_head(m_, c_, forward, gamma, mutate)
        w = head[0]
        W = w.sum() if n_kept else LD(0)
        for k, t in zip(np.asarray(strikes, dtype=np.float64).ravel(), np.asarray(types).ravel()):
            put = str(t) == "P"
            terms = strike_terms(head, forward, k, put, corr, mutate)
            sh = host_shift(forward, k, put)
            vals = []
            for name, v, shift in zip(("delta", "dual_delta", "dual_gamma"), terms, (sh, -sh, 0.0)):
                if not n_kept:
                    vals.append((LD(np.nan), LD(np.nan)))
                    cond[name].append(np.nan)
                    continue
                value = (w * v).sum() / W
                var, s1 = ((w * (v - value)) ** 2).sum(), ((w * (v - LD(shift))) ** 2).sum()
                if mutate == "unweighted_error":
                    err = v.std() / np.sqrt(LD(n_kept))
                else:
                    err = np.sqrt(var) / W
                vals.append((value, err))
                cond[name].append(float(s1 / var) if var > 0 else (np.inf if s1 > 0 else 1.0))
            cond["gamma"].append(cond["dual_gamma"][-1])
            r2 = (LD(k) / LD(forward)) ** 2
            for name, (v, s) in zip(("delta", "dual_delta", "dual_gamma"), vals):
                out[name].append(v)
                out[name + "_stderr"].append(s)
            out["gamma"].append(r2 * vals[2][0])
            out["gamma_stderr"].append(r2 * vals[2][1])
    out["price"], out["stderr"] = list(prices), list(errs)
    stats = dict(sum_weights=W, n_kept=n_kept, n_dropped=n - n_kept, n_zero_cv=int(np.sum(c_ == 0.0)), corr=corr,
                 error_conditioning={q: np.array(v) for q, v in cond.items()})
    return {f: np.array(v, dtype=LD) for f, v in out.items()}, stats


def log_return_pdf(mu, cv, x_grid, gamma, mutate=None):
    """the density of the log-return under the kernel without a bandwidth: calls at K_j = exp(x_j), F = 1, recenter=False;
    (pdf, its error, stats)"""
    strikes = np.exp(np.asarray(x_grid, dtype=np.float64))
    g, stats = estimator(mu, cv, 1.0, strikes, ["C"] * strikes.size, gamma, False, mutate)
    return strikes * g["dual_gamma"], strikes * g["dual_gamma_stderr"], stats
