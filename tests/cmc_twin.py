"""
CPU twin of the conditional Monte Carlo chain pricers (csrc/svmc_cmc.hip, include/svmc.h), shared by
tests/golden/make_golden_cmc.py, tests/test_cmc_host.py and tests/test_gpu_cmc.py.

Stream (csrc/svmc_rng.h, tag 8): ONE normal per step; step s (chain-global) takes word s & 3 of Philox call s >> 2, turned into
N(0,1) by the stream's inverse CDF (hawkes_twin.normal_from_words).

Recursions: the REFERENCE's step as the reference writes it (pricers/logsv_pricer.py:1037-1045, pricers/heston_pricer.py:372-379),
not the kernels' regrouping, with the volatility's driver substituted: LogSV beta w0 + volvol w1 = vartheta sqrt(dt) b, Heston
rho w0 + rho_1 w1 = sqrt(dt) b, and the return's conditional mean and variance accumulated in place of x:
    mu += alpha/2 eta^2 sigma^2 dt + rho eta sigma sqrt(dt) b,   cv += (1 - rho^2) eta^2 sigma^2 dt
(LogSV: 1 - rho^2 formed as volvol^2 / vartheta^2, rho = beta / vartheta, both 0 and 1 at vartheta = 0).  In NumPy (np_*) and in
mpmath (mp_*, any precision).

Estimator: include/svmc.h's, in numpy.longdouble with the keep decisions taken in double; the normal CDF is scipy's ndtr at the
argument's nearest double, corrected to first order for the long-double remainder (its own error is scipy's, about 1e-16 relative).
"""
import numpy as np

import hawkes_twin as ht

TAG = 8
FLOOR = 1e-4
LD = np.longdouble


# ---- stream ---------------------------------------------------------------------------------------------------------------------
def step_words(seed, n, steps, offset, call_id=0, path0=0):
    """the word of every (step, path): [steps][n] uint32"""
    c0 = offset >> 2
    w = np.stack(ht.stream_words(seed, call_id, TAG, path0, n, c0, ((offset + steps - 1) >> 2) - c0 + 1))     # [4][calls][n]
    st = np.arange(offset, offset + steps)
    return w[st & 3, (st >> 2) - c0, :]


def normals(seed, n, steps, offset, call_id=0, path0=0, exact=True):
    """[steps][n] unscaled N(0,1); exact=False evaluates the cubic with plain multiply-adds (statistics only: 1e-16 off the stream)"""
    w = step_words(seed, n, steps, offset, call_id, path0)
    if exact:
        return ht.normal_from_words(w)
    m, p0, p1 = ht.icdf_table()
    t = w.view(np.int32).astype(np.float64)
    j = ((t.view(np.uint64) >> np.uint64(32)).astype(np.uint32) >> np.uint32(20 - m)) & np.uint32(p0.shape[0] - 1)
    a = np.abs(t)
    return np.copysign(((p1[j, 1] * a + p1[j, 0]) * a + p0[j, 1]) * a + p0[j, 0], t)


# ---- the recursions in NumPy ------------------------------------------------------------------------------------------------------
def logsv_rho_factor(beta, volvol):
    """(vartheta, rho, 1 - rho^2 as volvol^2 / vartheta^2) -- (0, 0, 1) at vartheta = 0"""
    vartheta2 = beta * beta + volvol * volvol
    vartheta = np.sqrt(vartheta2)
    if vartheta > 0.0:
        return vartheta, beta / vartheta, (volvol * volvol) / vartheta2
    return 0.0, 0.0, 1.0


def np_logsv(start, dt, p, eta, spot, B, mutate=None):
    """(mu, cv, sigma, qvar) after B.shape[0] steps from start = (mu, cv, sigma, qvar) arrays.  mutate: a deliberate error for
    tests/test_cmc_host.py -- "rho_sign" | "cv_no_factor" """
    mu, cv, s, q = (np.array(a, dtype=np.float64) for a in start)
    sdt = np.sqrt(dt)
    theta, k1, k2, beta, volvol = (p[k] for k in ("theta", "kappa1", "kappa2", "beta", "volvol"))
    alpha, adj = (-1.0, 0.0) if spot else (1.0, beta * eta)
    vartheta, rho, factor = logsv_rho_factor(beta, volvol)
    if mutate == "rho_sign":
        rho = -rho
    if mutate == "cv_no_factor":
        factor = 1.0
    vartheta2, eta2 = beta * beta + volvol * volvol, eta * eta
    L = np.log(s)
    for b in B:
        w = sdt * b
        s2dt = eta2 * s * s * dt
        mu = mu + alpha * 0.5 * s2dt + rho * (eta * s * w)
        cv = cv + factor * s2dt
        L = L + ((k1 * theta / s - k1) + k2 * (theta - s) + adj * s - 0.5 * vartheta2) * dt + vartheta * w
        s = np.exp(L)
        q = q + 0.5 * (s2dt + eta2 * s * s * dt)
    return mu, cv, s, q


def np_heston(start, dt, p, B, mutate=None):
    """(mu, cv, v, qvar) after B.shape[0] Euler steps with the reference's floor"""
    mu, cv, v, q = (np.array(a, dtype=np.float64) for a in start)
    sdt = np.sqrt(dt)
    theta, kappa, rho, volvol = (p[k] for k in ("theta", "kappa", "rho", "volvol"))
    rho_1 = np.sqrt(1.0 - rho * rho)
    factor = rho_1 * rho_1
    if mutate == "rho_sign":
        rho = -rho
    if mutate == "cv_no_factor":
        factor = 1.0
    for b in B:
        w = sdt * b
        s = np.sqrt(v)
        s2dt = v * dt
        mu = mu - 0.5 * s2dt + rho * (s * w)
        cv = cv + factor * s2dt
        q = q + s2dt
        v = v + kappa * (theta - v) * dt + s * volvol * w
        v = np.maximum(v, FLOOR)
    return mu, cv, v, q


# the plain two-Brownian steps on the same conventions (W0, W1 unscaled): what the conditional estimator is compared with
def np_logsv_plain(x, s, dt, p, eta, W0, W1):
    sdt = np.sqrt(dt)
    theta, k1, k2, beta, volvol = (p[k] for k in ("theta", "kappa1", "kappa2", "beta", "volvol"))
    vartheta2, eta2 = beta * beta + volvol * volvol, eta * eta
    L = np.log(s)
    for z0, z1 in zip(W0, W1):
        w0, w1 = sdt * z0, sdt * z1
        x = x - 0.5 * (eta2 * s * s * dt) + eta * s * w0
        L = L + ((k1 * theta / s - k1) + k2 * (theta - s) - 0.5 * vartheta2) * dt + beta * w0 + volvol * w1
        s = np.exp(L)
    return x, s


def np_heston_plain(x, v, dt, p, W0, W1):
    sdt = np.sqrt(dt)
    theta, kappa, rho, volvol = (p[k] for k in ("theta", "kappa", "rho", "volvol"))
    rho_1 = np.sqrt(1.0 - rho * rho)
    for z0, z1 in zip(W0, W1):
        w0, w1 = sdt * z0, sdt * z1
        s = np.sqrt(v)
        x = x - 0.5 * (v * dt) + s * w0
        v = np.maximum(v + kappa * (theta - v) * dt + s * volvol * (rho * w0 + rho_1 * w1), FLOOR)
    return x, v


# ---- the recursions in mpmath -----------------------------------------------------------------------------------------------------
def mp_logsv(mp, start, dt, p, eta, spot, B, snaps):
    """{steps: [4][n] of mpf} at mpmath's current precision, and the first fragile step per path (none: LogSV has no decision)"""
    F = mp.mpf
    n = B.shape[1]
    dt, eta = F(dt), F(eta)
    sdt = mp.sqrt(dt)
    theta, k1, k2, beta, volvol = (F(p[k]) for k in ("theta", "kappa1", "kappa2", "beta", "volvol"))
    alpha, adj = (F(-1), F(0)) if spot else (F(1), beta * eta)
    vartheta2, eta2 = beta * beta + volvol * volvol, eta * eta
    vartheta = mp.sqrt(vartheta2)
    rho, factor = (beta / vartheta, volvol * volvol / vartheta2) if vartheta > 0 else (F(0), F(1))
    out = {s: [[None] * n for _ in range(4)] for s in snaps}
    for j in range(n):
        mu, cv, s, q = (F(float(start[i][j])) for i in range(4))
        L = mp.log(s)
        for t in range(max(snaps)):
            w = sdt * F(float(B[t, j]))
            s2dt = eta2 * s * s * dt
            mu = mu + alpha * F(0.5) * s2dt + rho * eta * s * w
            cv = cv + factor * s2dt
            L = L + ((k1 * theta / s - k1) + k2 * (theta - s) + adj * s - F(0.5) * vartheta2) * dt + vartheta * w
            s = mp.exp(L)
            q = q + F(0.5) * (s2dt + eta2 * s * s * dt)
            if t + 1 in out:
                for i, u in enumerate((mu, cv, s, q)):
                    out[t + 1][i][j] = u
    return out, np.zeros(n, dtype=np.int64)


def mp_heston(mp, start, dt, p, B, snaps, fragile_rel=1e-9):
    """... fragile: the new variance came within fragile_rel (relative) of the floor at that step"""
    F = mp.mpf
    n = B.shape[1]
    dt = F(dt)
    sdt = mp.sqrt(dt)
    theta, kappa, rho, volvol = (F(p[k]) for k in ("theta", "kappa", "rho", "volvol"))
    rho1sq, floor = 1 - rho * rho, F(FLOOR)
    out = {s: [[None] * n for _ in range(4)] for s in snaps}
    frag = np.zeros(n, dtype=np.int64)
    for j in range(n):
        mu, cv, v, q = (F(float(start[i][j])) for i in range(4))
        for t in range(max(snaps)):
            w = sdt * F(float(B[t, j]))
            s = mp.sqrt(v)
            s2dt = v * dt
            mu = mu - F(0.5) * s2dt + rho * s * w
            cv = cv + rho1sq * s2dt
            q = q + s2dt
            v = v + kappa * (theta - v) * dt + s * volvol * w
            if abs(v - floor) <= fragile_rel * floor and not frag[j]:
                frag[j] = t + 1
            v = max(v, floor)
            if t + 1 in out:
                for i, u in enumerate((mu, cv, v, q)):
                    out[t + 1][i][j] = u
    return out, frag


# ---- tests/golden/cmc_steps.npz ---------------------------------------------------------------------------------------------------
import os  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cmc_steps.npz")
STEP_CONSTANTS = {"logsv": ("theta", "kappa1", "kappa2", "beta", "volvol", "eta", "dt"), "heston": ("theta", "kappa", "rho", "volvol", "dt")}


def case_normals(case):
    return normals(case["seed"], case["n"], case["steps"], case["offset"])


def restate(case, B, scaled=None):
    """the NumPy restatement's terminal state [4][n] on a fixture case; scaled = (name, factor): that one step constant multiplied"""
    p, dt, eta = dict(case["params"]), case["dt"], case.get("eta", 1.0)
    if scaled is not None:
        name, f = scaled
        if name == "dt":
            dt = dt * f
        elif name == "eta":
            eta = eta * f
        else:
            p[name] = p[name] * f
    start = [np.full(case["n"], v) for v in case["start"]]
    with np.errstate(all="ignore"):
        if case["gen"] == "logsv":
            return np.stack(np_logsv(start, dt, p, eta, case["spot"], B))
        return np.stack(np_heston(start, dt, p, B))


# ---- the estimator ----------------------------------------------------------------------------------------------------------------
def keep_mask(mu, cv):
    """the keep rule, decided in double: mu, cv and exp(mu + cv / 2) finite, cv >= 0"""
    mu, cv = np.asarray(mu, dtype=np.float64), np.asarray(cv, dtype=np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(mu + 0.5 * cv)
        return np.isfinite(mu) & np.isfinite(cv) & (cv >= 0.0) & np.isfinite(e)


def ndtr_l(x):
    """Phi(x) for long-double x: scipy's ndtr at the nearest double plus the first-order term for the remainder"""
    from scipy.special import ndtr
    xd = np.asarray(x, dtype=np.float64)
    rem = np.asarray(x, dtype=LD) - xd.astype(LD)
    pdf = np.exp(-0.5 * xd * xd) / np.sqrt(2.0 * np.pi)
    return ndtr(xd).astype(LD) + pdf.astype(LD) * rem


def black_l(fc, ln_fc, cv, kp, put):
    """per path, long double: the undiscounted Black-76 price of fc against the scalar strike kp at total variance cv (kept paths)"""
    if not kp > 0:
        return np.zeros_like(fc) if put else fc - kp
    intrinsic = np.maximum(kp - fc, LD(0)) if put else np.maximum(fc - kp, LD(0))
    pos = cv > 0
    sd = np.sqrt(np.where(pos, cv, LD(1)))
    d1 = (ln_fc - np.log(LD(kp))) / sd + sd / 2
    d2 = d1 - sd
    bs = kp * ndtr_l(-d2) - fc * ndtr_l(-d1) if put else fc * ndtr_l(d1) - kp * ndtr_l(d2)
    return np.where(pos, bs, intrinsic)


def estimator(mu, cv, forward, strikes, types, discfactor=1.0, recenter=True):
    """(prices [K], stderrs [K], stats dict) of include/svmc.h's estimator; types: 'C' | 'P' per strike"""
    mu, cv = np.asarray(mu, dtype=np.float64), np.asarray(cv, dtype=np.float64)
    n = mu.size
    keep = keep_mask(mu, cv)
    m, c = mu[keep].astype(LD), cv[keep].astype(LD)
    h = m + c / 2
    e = np.exp(h)
    F = LD(forward)
    fc, ln_fc = F * e, np.log(F) + h
    n_kept = int(keep.sum())
    mean_e = (e[0] + (e - e[0]).mean()) if n_kept else LD(np.nan)
    corr = (F * mean_e - F) if recenter else LD(0)
    prices, errs = [], []
    for k, t in zip(np.asarray(strikes, dtype=np.float64).ravel(), np.asarray(types).ravel()):
        pay = black_l(fc, ln_fc, c, LD(k) + corr, str(t) == "P")
        if n_kept:
            d = pay - pay[0]                                   # the sums' shift (include/svmc.h): identical paths leave exact zeros
            prices.append(float(LD(discfactor) * (pay[0] + d.mean())))
            errs.append(float(LD(discfactor) * d.std() / np.sqrt(LD(n))))
        else:
            prices.append(np.nan), errs.append(np.nan)
    stats = dict(forward_mc=float(F * mean_e), forward_mc_stderr=float(abs(F) * (e - e[0]).std() / np.sqrt(LD(n))) if n_kept else np.nan,
                 corr=float(corr), n_kept=n_kept, n_dropped=n - n_kept)
    return np.array(prices), np.array(errs), stats


def plain_estimator(x, forward, strikes, types, discfactor=1.0):
    """compute_mc_vars_payoff on terminal log-returns x (recentred spots), double: (prices, stderrs)"""
    spot = forward * np.exp(x)
    spot = spot - (np.nanmean(spot) - forward)
    prices, errs = [], []
    for k, t in zip(np.asarray(strikes).ravel(), np.asarray(types).ravel()):
        pay = np.maximum(k - spot, 0.0) if str(t) == "P" else np.maximum(spot - k, 0.0)
        prices.append(discfactor * np.nanmean(pay))
        errs.append(discfactor * np.nanstd(pay) / np.sqrt(x.size))
    return np.array(prices), np.array(errs)


def chain_grids(ttms, nb_steps_per_year):
    """[(nb_steps, dt)] per expiry, each slice starting at the previous expiry (utils/funcs.py:44-47)"""
    out, t0 = [], 0.0
    for ttm in ttms:
        d = ttm - t0
        nb = int(d * nb_steps_per_year) + 1
        out.append((nb, d if nb == 1 else d / nb))
        t0 = ttm
    return out
