"""
compute_mc_vars_payoff on the GPU (mirror of the reference's utils/mc_payoffs.py:10-88).

Same signature, same return, same errors.  The path vectors are uploaded, reduced by libsvmc's two
deterministic sum kernels (svmc_spot_sums, svmc_payoff_sums) and finalised on the host; K prices come
back.  Inside the chain pricers the state is already resident and this function is not on the path.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from ..engine import (JUMP_SETS_MAX, cond_density_arrays, cond_density_stats_dicts, get_engine, option_type_codes, payoff_finalize, payoff_shifts,
                      tilted_chain_arrays, tilted_greeks_stats_dicts, tilted_stats_dicts, tilted_type_codes)
from ..mc_chain import variable_type_code
from .config import VariableType


def compute_mc_vars_payoff(x0: np.ndarray, sigma0: np.ndarray, qvar0: np.ndarray, ttm: float, forward: float,
                           strikes_ttm: np.ndarray, optiontypes_ttm: np.ndarray, discfactor: float = 1.0,
                           variable_type: VariableType = VariableType.LOG_RETURN
                           ) -> Tuple[np.ndarray, np.ndarray]:
    """sigma0 is accepted for signature symmetry and unused, as in the reference."""
    vt = variable_type_code(variable_type)                       # NotImplementedError for SIGMA
    codes = option_type_codes(optiontypes_ttm)                   # ValueError("unknown option payoff code")
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    strikes = np.ascontiguousarray(strikes_ttm, dtype=np.float64)
    n = x0.shape[0]
    eng = get_engine(n)
    eng.upload(eng.x.ptr, x0)
    if vt == 2:
        eng.upload(eng.qvar.ptr, np.ascontiguousarray(qvar0, dtype=np.float64))
    shifts = payoff_shifts(strikes.ravel(), codes, float(forward), vt)
    ptr, _ = eng.alloc_sums(2 + 3 * strikes.size, "slice")
    eng.spot_sums(eng.x.ptr, float(forward), ptr)
    eng.payoff_sums(eng.x.ptr, eng.qvar.ptr if vt == 2 else None, float(forward), float(ttm), ptr, strikes.ravel(),
                    codes, shifts, vt, ptr + 16)
    sums = eng.download(ptr + 16, 3 * strikes.size)
    prices, stderrs = payoff_finalize(sums, shifts, float(discfactor), float(n))
    return prices.reshape(strikes.shape), stderrs.reshape(strikes.shape)


def compute_mc_vars_payoff_with_gamma(x0: np.ndarray, forward: float, strikes_ttm: np.ndarray, optiontypes_ttm: np.ndarray,
                                      risk_premia_gamma: float, recenter_forward: bool = False, return_stats: bool = False,
                                      variable_type: VariableType = VariableType.LOG_RETURN):
    """option prices under the exponential risk-premia kernel from terminal log-returns x0 (host array), the estimator of
    include/svmc.h's svmc_tilted_payoff_chain: w = exp(gamma x), spot = forward exp(x) - corr (corr = 0, or
    compute_mc_vars_payoff's recentring nanmean(forward exp(x)) - forward with recenter_forward), a path kept iff x, w^2 and
    (w spot)^2 are finite, price = sum w pay / sum w (undiscounted) and its delta-method standard error.  'C' / 'P' only (others:
    ValueError("not implemented")), LOG_RETURN only (NotImplementedError).  Returns (prices, stderrs) in the strikes' shape, and
    with return_stats=True a third item: the dict of engine.TILTED_STATS_FIELDS (normalizer, gamma forward, their errors, the
    effective sample size, n_kept, n_dropped, sum of weights).  Follows compute_mc_vars_payoff's route: upload, reduce on the
    device, K prices back."""
    if variable_type_code(variable_type) != 1:
        raise NotImplementedError(f"variable_type={variable_type}: the risk-premia kernel weights the log-return only")
    codes = tilted_type_codes(optiontypes_ttm)                   # ValueError("not implemented")
    strikes = np.asarray(strikes_ttm, dtype=np.float64)
    ch = tilted_chain_arrays([float(forward)], [strikes], [codes], [float(risk_premia_gamma)])
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    eng = get_engine(x0.shape[0])
    eng.upload(eng.x.ptr, x0)
    prices, stderrs, stats = eng.tilted_payoffs(ch["forwards"], [strikes], [codes], ch["gammas"], bool(recenter_forward))
    if return_stats:
        return prices[0][0], stderrs[0][0], tilted_stats_dicts(stats[0])[0]
    return prices[0][0], stderrs[0][0]


def compute_mc_vars_payoff_conditional(mu: np.ndarray, cv: np.ndarray, ttm: float, forward: float, strikes_ttm: np.ndarray,
                                       optiontypes_ttm: np.ndarray, discfactor: float = 1.0, recenter: bool = True,
                                       return_stats: bool = False):
    """option prices by conditional Monte Carlo from per-path conditional means and variances of the log-return (host arrays), the
    estimator of include/svmc.h's svmc_cmc_payoff_chain: a path is kept iff mu, cv and exp(mu + cv / 2) are finite and cv >= 0;
    per kept path the Black-76 price of F_c = forward exp(mu + cv / 2) against K + corr at total variance cv, corr =
    mean_kept(F_c) - forward (0 with recenter=False); price = discfactor x mean, error = discfactor x population deviation /
    sqrt(n_path).  ttm is accepted for signature symmetry with compute_mc_vars_payoff and unused (cv is a TOTAL variance).  'C' /
    'P' only (others: ValueError("not implemented")).  Returns (prices, stderrs) in the strikes' shape, and with
    return_stats=True the dict of engine.CMC_STATS_FIELDS as a third item."""
    codes = tilted_type_codes(optiontypes_ttm)                   # ValueError("not implemented")
    strikes = np.asarray(strikes_ttm, dtype=np.float64)
    mu = np.ascontiguousarray(mu, dtype=np.float64).ravel()
    cv = np.ascontiguousarray(cv, dtype=np.float64).ravel()
    if mu.size != cv.size or mu.size == 0:
        raise ValueError("mu and cv must be non-empty and of one length")
    eng = get_engine(mu.size)
    eng.upload(eng.x.ptr, mu)
    eng.upload(eng.cv.ptr, cv)
    prices, stderrs, stats = eng.conditional_payoffs([float(forward)], [float(discfactor)], [strikes.ravel()], [codes], bool(recenter))
    out = (prices[0].reshape(strikes.shape), stderrs[0].reshape(strikes.shape))
    return out + (stats[0],) if return_stats else out


def compute_mc_vars_payoff_conditional_with_gamma(mu: np.ndarray, cv: np.ndarray, forward: float, strikes_ttm: np.ndarray,
                                                  optiontypes_ttm: np.ndarray, risk_premia_gamma, recenter: bool = False,
                                                  return_stats: bool = False,
                                                  variable_type: VariableType = VariableType.LOG_RETURN):
    """option prices under the exponential risk-premia kernel by conditional Monte Carlo from per-path conditional means and
    variances of the log-return (host arrays; any model's, cv may differ per path), the estimator of include/svmc_ext.h's
    svmc_tilted_cond_payoff_chain: W = exp(gamma mu + gamma^2 cv / 2), F_t = forward exp(mu + (gamma + 1/2) cv), a path kept iff
    compute_mc_vars_payoff_conditional keeps it and W^2 and (W F_t)^2 are finite, per kept path the Black-76 price of F_t against
    K + corr at total variance cv (corr = compute_mc_vars_payoff_conditional's with recenter, else 0), price = sum W B / sum W
    (undiscounted) and its delta-method standard error.  risk_premia_gamma: one gamma -- (prices, stderrs) in the strikes' shape,
    with return_stats=True also the dict of engine.TILTED_COND_STATS_FIELDS -- or a sequence of up to 16 -- lists of those, one
    entry per gamma, from one upload.  'C' / 'P' only (others: ValueError("not implemented")), LOG_RETURN only
    (NotImplementedError)."""
    if variable_type_code(variable_type) != 1:
        raise NotImplementedError(f"variable_type={variable_type}: the risk-premia kernel weights the log-return only")
    codes = tilted_type_codes(optiontypes_ttm)                   # ValueError("not implemented")
    strikes = np.asarray(strikes_ttm, dtype=np.float64)
    single = np.ndim(risk_premia_gamma) == 0
    ch = tilted_chain_arrays([float(forward)], [strikes], [codes], [float(risk_premia_gamma)] if single else risk_premia_gamma)
    mu = np.ascontiguousarray(mu, dtype=np.float64).ravel()
    cv = np.ascontiguousarray(cv, dtype=np.float64).ravel()
    if mu.size != cv.size or mu.size == 0:
        raise ValueError("mu and cv must be non-empty and of one length")
    eng = get_engine(mu.size)
    eng.upload(eng.x.ptr, mu)
    eng.upload(eng.cv.ptr, cv)
    prices, stderrs, stats = eng.tilted_conditional_payoffs(ch["forwards"], [strikes], [codes], ch["gammas"], bool(recenter))
    out = ([p[0] for p in prices], [e[0] for e in stderrs])
    if return_stats:
        out = out + ([tilted_stats_dicts(st)[0] for st in stats],)
    return tuple(o[0] for o in out) if single else out


def compute_mc_vars_payoff_jump_sets(a: np.ndarray, variances, gammas, forward: float, strikes_ttm: np.ndarray,
                                     optiontypes_ttm: np.ndarray, recenter: bool = False, return_stats: bool = False):
    """option prices under the exponential risk-premia kernel for MANY sets (variance v_q, gamma g_q) from ONE host row a with
    x | a ~ N(a - v / 2, v), v the same on every path (the Hawkes jump-diffusion's rows at sigma = 0; any model of that form), the
    estimator of include/svmc_est.h's svmc_jump_sets_payoff_chain: compute_mc_vars_payoff_conditional_with_gamma on
    (a - v_q / 2, v_q) at gamma g_q for every q, from one upload and one pass.  variances, gammas: sequences of one length (any
    number: calls of engine.JUMP_SETS_MAX).  Returns (prices, stderrs), each [set] in the strikes' shape, and with
    return_stats=True a third item, [set] dicts of engine.TILTED_COND_STATS_FIELDS with "corr" added.  'C' / 'P' only (others:
    ValueError("not implemented")); undiscounted."""
    codes = tilted_type_codes(optiontypes_ttm)                   # ValueError("not implemented")
    strikes = np.asarray(strikes_ttm, dtype=np.float64)
    v = np.atleast_1d(np.asarray(variances, dtype=np.float64)).ravel()
    g = np.atleast_1d(np.asarray(gammas, dtype=np.float64)).ravel()
    if v.size != g.size or v.size == 0:
        raise ValueError("variances and gammas must be non-empty and of one length")
    if not (np.all(np.isfinite(v)) and np.all(v >= 0.0)):
        raise ValueError("variances must be finite and not negative")
    if not np.all(np.isfinite(g)):
        raise ValueError("risk-premia gammas must be finite")
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    if a.size == 0:
        raise ValueError("a must be non-empty")
    eng = get_engine(a.size)
    eng.upload(eng.x.ptr, a)
    prices, stderrs, stats = [], [], []
    for q0 in range(0, v.size, JUMP_SETS_MAX):
        sl = slice(q0, q0 + JUMP_SETS_MAX)
        p, e, st, corr = eng.jump_sets_payoffs([float(forward)], [strikes], [codes], v[sl, None], g[sl], bool(recenter))
        prices += [x[0] for x in p]
        stderrs += [x[0] for x in e]
        stats += [dict(tilted_stats_dicts(x)[0], corr=float(corr[0])) for x in st]
    return (prices, stderrs, stats) if return_stats else (prices, stderrs)


def compute_mc_vars_greeks_conditional_with_gamma(mu: np.ndarray, cv: np.ndarray, forward: float, strikes_ttm: np.ndarray,
                                                  optiontypes_ttm: np.ndarray, risk_premia_gamma, recenter: bool = False,
                                                  return_stats: bool = False,
                                                  variable_type: VariableType = VariableType.LOG_RETURN):
    """compute_mc_vars_payoff_conditional_with_gamma with the derivatives of its prices in the forward and the strike
    (include/svmc_est.h's svmc_tilted_cond_greeks_chain; host arrays of any model's per-path (mu, cv)): a dict in the strikes'
    shape with the ten keys of engine.CMC_GREEKS_FIELDS -- price, stderr (that function's), delta, dual_delta, gamma, dual_gamma,
    each with its _stderr; undiscounted -- and with return_stats=True "stats", the dict of engine.TILTED_COND_GREEKS_STATS_FIELDS.
    risk_premia_gamma: one gamma -- the dict -- or a sequence of up to 16 -- a list of dicts, one per gamma, from one upload.
    'C' / 'P' only (others: ValueError("not implemented")), LOG_RETURN only (NotImplementedError)."""
    if variable_type_code(variable_type) != 1:
        raise NotImplementedError(f"variable_type={variable_type}: the risk-premia kernel weights the log-return only")
    codes = tilted_type_codes(optiontypes_ttm)                   # ValueError("not implemented")
    strikes = np.asarray(strikes_ttm, dtype=np.float64)
    single = np.ndim(risk_premia_gamma) == 0
    ch = tilted_chain_arrays([float(forward)], [strikes], [codes], [float(risk_premia_gamma)] if single else risk_premia_gamma)
    mu = np.ascontiguousarray(mu, dtype=np.float64).ravel()
    cv = np.ascontiguousarray(cv, dtype=np.float64).ravel()
    if mu.size != cv.size or mu.size == 0:
        raise ValueError("mu and cv must be non-empty and of one length")
    eng = get_engine(mu.size)
    eng.upload(eng.x.ptr, mu)
    eng.upload(eng.cv.ptr, cv)
    prices, stderrs, stats = eng.tilted_conditional_payoffs(ch["forwards"], [strikes], [codes], ch["gammas"], bool(recenter))
    greeks, gstats = eng.tilted_conditional_greeks(ch["forwards"], [strikes], [codes], ch["gammas"], bool(recenter))
    out = []
    for p, e, g, st, gst in zip(prices, stderrs, greeks, stats, gstats):
        d = dict(price=p[0], stderr=e[0], **{name: rows[0] for name, rows in g.items()})
        if return_stats:
            d["stats"] = tilted_greeks_stats_dicts(np.concatenate([st, gst[:, 3:4]], axis=1))[0]
        out.append(d)
    return out[0] if single else out


def compute_mc_vars_pdf_conditional(mu: np.ndarray, cv, x_grid: np.ndarray, gammas=None, return_stderr: bool = False,
                                    return_stats: bool = False):
    """the mixture density of the log-return at x_grid from per-path conditional means and variances (host arrays of any model;
    cv per path or one scalar for all), the estimator of include/svmc_est.h's svmc_cond_density_chain: every path kept by
    compute_mc_vars_payoff_conditional's rule with cv > 0 adds its Gaussian N(x; mu_j, cv_j) -- no bandwidth -- and under the
    exponential risk-premia kernel exp(gamma x) the path's weight W_j = exp(gamma mu_j + gamma^2 cv_j / 2) times its Gaussian shifted
    by gamma cv_j; pdf = sum / sum_j W_j.  One exponential per (path, point) whatever the number of gammas.  gammas=None: the density
    itself (gamma 0) in x_grid's shape; a sequence of up to 16 gammas: [gamma][x].  Not normalised: it integrates to the weight
    share of the kept paths with cv > 0.  A gamma at which a kept path's squared weight overflows returns NaN (its statistics say
    how many: n_weight_dropped); compute_mc_vars_greeks_conditional_with_gamma's dual_gamma still serves it.  Returns pdf, then
    with return_stderr=True its standard error in the same shape, then with return_stats=True the dict of engine.CD_STATS_FIELDS
    (a list of them, one per gamma, with gammas given)."""
    single = gammas is None
    mu = np.ascontiguousarray(mu, dtype=np.float64).ravel()
    cv = np.asarray(cv, dtype=np.float64)
    cv = np.full(mu.size, float(cv)) if cv.ndim == 0 else np.ascontiguousarray(cv).ravel()
    if mu.size != cv.size or mu.size == 0:
        raise ValueError("mu and cv must be non-empty and of one length (or cv a scalar)")
    x = np.asarray(x_grid, dtype=np.float64)
    ch = cond_density_arrays([x], [0.0] if single else gammas)         # ValueError before any engine is asked for
    eng = get_engine(mu.size)
    eng.upload(eng.x.ptr, mu)
    eng.upload(eng.cv.ptr, cv)
    pdf, err, stats = eng.conditional_densities([x], ch["gammas"])
    p, e = np.array([g[0] for g in pdf]), np.array([g[0] for g in err])
    st = [cond_density_stats_dicts(s)[0] for s in stats]
    out = (p[0] if single else p,)
    if return_stderr:
        out += (e[0] if single else e,)
    if return_stats:
        out += (st[0] if single else st,)
    return out[0] if len(out) == 1 else out


def compute_mc_vars_greeks_conditional(mu: np.ndarray, cv: np.ndarray, ttm: float, forward: float, strikes_ttm: np.ndarray,
                                       optiontypes_ttm: np.ndarray, discfactor: float = 1.0, recenter: bool = True,
                                       return_stats: bool = False) -> dict:
    """compute_mc_vars_payoff_conditional with the derivatives of its prices in the forward and the strike (include/svmc.h's
    svmc_cmc_greeks_chain) from host arrays of one expiry: a dict, in the strikes' shape, of price, stderr, delta, delta_stderr,
    dual_delta, dual_delta_stderr, gamma, gamma_stderr, dual_gamma, dual_gamma_stderr, and with return_stats=True "stats", the dict
    of engine.CMC_GREEKS_STATS_FIELDS.  ttm is unused (cv is a TOTAL variance).  'C' / 'P' only (others: ValueError("not
    implemented"))."""
    codes = tilted_type_codes(optiontypes_ttm)                   # ValueError("not implemented")
    strikes = np.asarray(strikes_ttm, dtype=np.float64)
    mu = np.ascontiguousarray(mu, dtype=np.float64).ravel()
    cv = np.ascontiguousarray(cv, dtype=np.float64).ravel()
    if mu.size != cv.size or mu.size == 0:
        raise ValueError("mu and cv must be non-empty and of one length")
    eng = get_engine(mu.size)
    eng.upload(eng.x.ptr, mu)
    eng.upload(eng.cv.ptr, cv)
    fields, stats = eng.conditional_greeks([float(forward)], [float(discfactor)], [strikes.ravel()], [codes], bool(recenter))
    out = {name: rows[0].reshape(strikes.shape) for name, rows in fields.items()}
    if return_stats:
        out["stats"] = stats[0]
    return out


def compute_mc_vars_sens_conditional(mu_up: np.ndarray, cv_up: np.ndarray, mu_dn: np.ndarray, cv_dn: np.ndarray, step: float,
                                     forward: float, strikes: np.ndarray, types: np.ndarray, discfactor: float = 1.0,
                                     recenter: bool = True):
    """the central difference of two conditional estimates ON THE SAME RANDOMS and the error of that difference (include/svmc.h's
    svmc_cmc_sens_chain) from host arrays of one expiry: (mu_up, cv_up) the job at theta + step, (mu_dn, cv_dn)
    the job at theta - step.  Each job is recentred by its own kept-path mean; a pair is kept iff the path is kept in both jobs;
    with recenter=True the error carries the delta-method term of the two recentring means.  Returns (sens, sens_stderr, n_pairs)
    in the strikes' shape (n_pairs as integers).  'C' / 'P' only (others: ValueError("not implemented"))."""
    codes = tilted_type_codes(types)                             # ValueError("not implemented")
    k = np.asarray(strikes, dtype=np.float64)
    rows = [np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (mu_up, cv_up, mu_dn, cv_dn)]
    if rows[0].size == 0 or any(a.size != rows[0].size for a in rows):
        raise ValueError("mu_up, cv_up, mu_dn and cv_dn must be non-empty and of one length")
    if not (np.isfinite(step) and step > 0.0):
        raise ValueError("step must be positive and finite")
    sens, _ = get_engine(rows[0].size).conditional_sens([float(forward)], [float(discfactor)], [k.ravel()], [codes], [float(step)],
                                                        bool(recenter), host_rows=[[[a]] for a in rows])
    return sens[0, 0].reshape(k.shape), sens[0, 1].reshape(k.shape), sens[0, 2].astype(np.int64).reshape(k.shape)


def compute_mc_vars_greeks(x0: np.ndarray, forward: float, strikes_ttm: np.ndarray, optiontypes_ttm: np.ndarray,
                           discfactor: float = 1.0, x_up=(), x_dn=(), steps=()) -> dict:
    """the Greeks tail of include/svmc.h's svmc_greeks_payoff_chain on host arrays of one expiry: x0 the base job's terminal
    log-returns, x_up[p] / x_dn[p] those of the jobs at theta_p + steps[p] / theta_p - steps[p] ON THE SAME RANDOMS (the paired
    differences are meaningless otherwise).  Every job is recentred by its own kept-path mean of exp(x).  Returns, in the strikes'
    shape: delta, delta_stderr (pathwise forward delta), dual_delta, dual_delta_stderr, n_itm, and lists over p of sens,
    sens_stderr, n_pairs.  'C' / 'P' only (others: ValueError("not implemented")).  Follows compute_mc_vars_payoff's route: upload,
    reduce on the device, the figures back."""
    codes = tilted_type_codes(optiontypes_ttm)                   # ValueError("not implemented")
    strikes = np.asarray(strikes_ttm, dtype=np.float64)
    x0 = np.ascontiguousarray(x0, dtype=np.float64).ravel()
    h = np.atleast_1d(np.asarray(steps, dtype=np.float64)).ravel()
    if not (len(x_up) == len(x_dn) == h.size):
        raise ValueError("one up row, one dn row and one step per sensitivity")
    if x0.size == 0:
        raise ValueError("x0 must not be empty")
    out = get_engine(x0.size).greeks_payoffs([float(forward)], [float(discfactor)], [strikes.ravel()], [codes], h,
                                             host_rows=([x0], [[u] for u in x_up], [[d] for d in x_dn]))
    shaped = lambda a: a.reshape(strikes.shape)                  # noqa: E731
    res = {k: shaped(out[k][0]) for k in ("delta", "delta_stderr", "dual_delta", "dual_delta_stderr")}
    res["n_itm"] = shaped(out["n_itm"][0]).astype(np.int64)
    res["sens"] = [shaped(p[0]) for p in out["sens"]]
    res["sens_stderr"] = [shaped(p[0]) for p in out["sens_stderr"]]
    res["n_pairs"] = [shaped(p[0]).astype(np.int64) for p in out["n_pairs"]]
    return res
