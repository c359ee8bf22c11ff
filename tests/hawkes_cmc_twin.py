"""
CPU twin of the conditional Monte Carlo stepping of the Hawkes jump-diffusion, in NumPy and in mpmath, shared by
tests/golden/make_golden_hawkes_cmc.py and tests/test_hawkes_cmc_host.py.  It is the specification a device kernel is to be held
to; the library has no such kernel yet, and nothing here calls the library.

Given a path's jumps the discretised log-return of the reference's step (pricers/hawkes_jd_pricer.py:753-774) is Gaussian -- its
diffusion sigma w0 has a constant sigma and is independent of both jump processes and both intensities -- so a path carries the
conditional mean mu and the variance is the same number for every path.

Streams (the layout csrc/svmc_rng.h's counters allow; tags 0 to 8 are in use): tag 9 carries the jump uniforms, TWO steps per Philox
call -- chain-global step s reads words 2 (s & 1) and 2 (s & 1) + 1 of the call at index s >> 1 as u_p, u_m = (r + 1/2) 2^-32; tag
10 carries the jump sizes at call index s, words 0 and 1 (E = -ln((r + 1/2) 2^-32)) as stream 7's, to be drawn lazily where a side
jumps and here for every step.  The index is the chain-global step, so a chain sliced or continued differently sees the same bits,
also where a slice boundary falls between the two steps of one call; the draws are independent of the plain pricer's (streams 6
and 7) at the same (seed, call id).  Philox and the words come from hawkes_twin; the estimator on (mu, cv) is cmc_twin's.

Recursion: hawkes_twin.simulate_terminal without the diffusion's normal -- per step, from the intensities at its start,
    jump_p = J_P 1{lambda_p dt > -ln u_p},  jump_m = J_M 1{lambda_m dt > -ln u_m}
    mu += ((mu_drift - sigma^2 / 2) dt - comp_p dt lambda_p) - comp_m dt lambda_m, then + jump_p + jump_m
    lambda_p, lambda_m: the plain step's two statements
and the variance is no state of a path: cv_i = cv_{i-1} + nb_steps_i (sigma sigma dt_i), one double per expiry (host_cv).
"""
import os

import numpy as np

import hawkes_twin as ht

UNIFORM_TAG, JUMP_TAG = 9, 10
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hawkes_cmc_steps.npz")
STEP_CONSTANTS = ("mu", "sigma", "shift_p", "mean_p", "shift_m", "mean_m", "theta_p", "kappa_p", "beta1_p", "beta2_p", "theta_m", "kappa_m",
                  "beta1_m", "beta2_m", "dt")


# ---- the chain of the statistical checks (tests/test_hawkes_cmc_host.py item 5) ------------------------------------------------------
STAT_N = 1 << 16
STAT_TTMS = (1.0 / 52.0, 1.0 / 12.0, 0.25)
STAT_SPY = 480                                 # 10 + 31 + 81 steps: at most 120 per expiry
STAT_MONEYNESS = (-1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5)      # ln(K / F) in total standard deviations of the expiry
STAT_SEED = 2026
Z_BOUND = 4.5


def total_std(p, ttm):
    """the standard deviation of the log-return over ttm with both intensities at their long-run levels: sigma^2 plus, per side,
    theta E[J^2], E[J^2] = shift^2 + 2 shift mean + 2 mean^2 for J = shift + mean E, E a unit exponential"""
    j2_p = p["shift_p"] ** 2 + 2.0 * p["shift_p"] * p["mean_p"] + 2.0 * p["mean_p"] ** 2
    j2_m = p["shift_m"] ** 2 + 2.0 * p["shift_m"] * p["mean_m"] + 2.0 * p["mean_m"] ** 2
    return float(np.sqrt(ttm * (p["sigma"] ** 2 + p["theta_p"] * j2_p + p["theta_m"] * j2_m)))


def stat_chain(p):
    """(chain keywords of the pricers at forward 1, per expiry the total standard deviation): per expiry calls then puts at
    K = exp(k sd), k in STAT_MONEYNESS"""
    sds = [total_std(p, t) for t in STAT_TTMS]
    strikes = [np.exp(np.array(STAT_MONEYNESS) * sd) for sd in sds]
    m = len(STAT_MONEYNESS)
    chain = dict(ttms=np.array(STAT_TTMS), forwards=np.ones(3), discfactors=np.array([0.999, 0.996, 0.99]),
                 strikes_ttms=[np.concatenate([k, k]) for k in strikes], optiontypes_ttms=[np.array(["C"] * m + ["P"] * m)] * 3)
    return chain, sds


# ---- streams ----------------------------------------------------------------------------------------------------------------------
def uniform_words(seed, n, steps, offset, call_id=0, path0=0, swap_halves=False):
    """(w_p, w_m), each [steps][n] uint32: the two words of every (step, path) on stream 9.  swap_halves: the even step reads the
    call's words 2, 3 and the odd step its words 0, 1 -- the deliberate error of tests/test_hawkes_cmc_host.py"""
    c0 = offset >> 1
    w = np.stack(ht.stream_words(seed, call_id, UNIFORM_TAG, path0, n, c0, ((offset + steps - 1) >> 1) - c0 + 1))   # [4][calls][n]
    st = np.arange(offset, offset + steps)
    half = 2 * (st & 1)
    if swap_halves:
        half = 2 - half
    return w[half, (st >> 1) - c0, :], w[half + 1, (st >> 1) - c0, :]


def draws(seed, n, steps, offset, call_id=0, path0=0, swap_halves=False):
    """the draws of `steps` steps from the chain-global step `offset`, arrays [steps][n]: the jump uniforms u_p, u_m and the exact
    uniforms v_p, v_m behind the unit exponentials of the jump sizes"""
    w_p, w_m = uniform_words(seed, n, steps, offset, call_id, path0, swap_halves)
    e = ht.stream_words(seed, call_id, JUMP_TAG, path0, n, offset, steps)
    return dict(u_p=ht.uniform_from_words(w_p), u_m=ht.uniform_from_words(w_m), v_p=ht.uniform_from_words(e[0]),
                v_m=ht.uniform_from_words(e[1]))


# ---- the recursion ----------------------------------------------------------------------------------------------------------------
def np_steps(state, dt, p, d, stats=None):
    """(mu, lambda_p, lambda_m) after d["u_p"].shape[0] steps of size dt from state = (mu, lambda_p, lambda_m) arrays"""
    m, lp, lm = (np.array(a, dtype=np.float64) for a in state)
    comp_p_dt = dt * (np.exp(p["shift_p"]) / (1.0 - p["mean_p"]) - 1.0)
    comp_m_dt = dt * (np.exp(p["shift_m"]) / (1.0 - p["mean_m"]) - 1.0)
    drift_dt = (p["mu"] - 0.5 * p["sigma"] * p["sigma"]) * dt
    J_P = p["shift_p"] + p["mean_p"] * -np.log(d["v_p"])
    J_M = p["shift_m"] - (-p["mean_m"]) * -np.log(d["v_m"])
    E_P, E_M = -np.log(d["u_p"]), -np.log(d["u_m"])
    for e_p, e_m, j_p, j_m in zip(E_P, E_M, J_P, J_M):
        hit_p, hit_m = lp * dt > e_p, lm * dt > e_m
        jump_p, jump_m = np.where(hit_p, j_p, 0.0), np.where(hit_m, j_m, 0.0)
        if stats is not None:
            stats["jumps_p"] = stats.get("jumps_p", 0) + hit_p.astype(np.int64)
            stats["jumps_m"] = stats.get("jumps_m", 0) + hit_m.astype(np.int64)
        drift = (drift_dt - comp_p_dt * lp) - comp_m_dt * lm
        m = ((m + drift) + jump_p) + jump_m
        load_p = p["beta1_p"] * jump_p + p["beta2_p"] * jump_m
        load_m = p["beta1_m"] * jump_p + p["beta2_m"] * jump_m
        lp = (lp + p["kappa_p"] * dt * (p["theta_p"] - lp)) + load_p
        lm = (lm + p["kappa_m"] * dt * (p["theta_m"] - lm)) + load_m
    return m, lp, lm


def host_cv(sigma, nb_steps, dts, cv_start=0.0):
    """cv_i = cv_{i-1} + nb_steps_i (sigma sigma dt_i) in double, in slice order: row f16's host formula"""
    out, cv = [], float(cv_start)
    for nb, dt in zip(nb_steps, dts):
        cv = cv + float(nb) * ((float(sigma) * float(sigma)) * float(dt))
        out.append(cv)
    return np.array(out)


def np_chain(p, seed, n, nb_steps, dts, offset=0, call_id=0, path0=0, state=None, scaled=None, swap_halves=False, stats=None):
    """[(mu, lambda_p, lambda_m)] per expiry of a chain of slices (nb_steps[i] steps of size dts[i]) from `state` (default: the
    origin (0, lambda_p, lambda_m)) at the chain-global step `offset`.  scaled = (name, factor): that one step constant multiplied
    (every dt for "dt"; "mu", which is 0 in the fixture's sets, has factor - 1 added instead); stats (a list, one dict per slice
    appended): per-path jump counts within the slice"""
    p, dts = dict(p), [float(v) for v in dts]
    if scaled is not None:
        name, f = scaled
        if name == "dt":
            dts = [v * f for v in dts]
        elif name == "mu":                                    # 0 in the fixture's sets: moved by f - 1, not scaled
            p["mu"] = p["mu"] + (f - 1.0)
        else:
            p[name] = p[name] * f
    st = (np.zeros(n), np.full(n, p["lambda_p"]), np.full(n, p["lambda_m"])) if state is None else state
    out, s = [], int(offset)
    for nb, dt in zip(nb_steps, dts):
        d = draws(seed, n, int(nb), s, call_id, path0, swap_halves)
        slice_stats = {} if stats is not None else None
        with np.errstate(all="ignore"):
            st = np_steps(st, dt, p, d, slice_stats)
        if stats is not None:
            stats.append(slice_stats)
        out.append(tuple(a.copy() for a in st))
        s += int(nb)
    return out


# ---- the recursion in mpmath ------------------------------------------------------------------------------------------------------
def mp_chain(mp, p, seed, n, nb_steps, dts, offset=0, fragile_rel=1e-9):
    """the same chain at mpmath's current precision from the origin: ([expiry][3][n] of mpf, fragile [expiry][n] bool, jumps
    [expiry][2][n] int -- the jumps of each side within the slice).  A path is fragile at an expiry when, at some step up to it, a
    jump test came within fragile_rel (relative) of its threshold.  -ln u >= 1 - u, so the logarithm is taken only where 1 - u does
    not exceed lambda dt by more than 1e-6 relative: beyond that there is no jump and no fragile test."""
    F = mp.mpf
    P = {k: F(float(v)) for k, v in p.items()}
    d_all, s = [], int(offset)
    for nb in nb_steps:
        d_all.append(draws(seed, n, int(nb), s))
        s += int(nb)
    half, one = F(0.5), F(1)
    m_exp = len(nb_steps)
    out = [[[None] * n for _ in range(3)] for _ in range(m_exp)]
    frag = np.zeros((m_exp, n), dtype=bool)
    jumps = np.zeros((m_exp, 2, n), dtype=np.int64)
    consts = []
    for dt in dts:
        dt = F(float(dt))
        consts.append((dt, (P["mu"] - half * P["sigma"] * P["sigma"]) * dt, dt * (mp.exp(P["shift_p"]) / (one - P["mean_p"]) - one),
                       dt * (mp.exp(P["shift_m"]) / (one - P["mean_m"]) - one), P["kappa_p"] * dt, P["kappa_m"] * dt))
    for j in range(n):
        m, lp, lm = F(0), P["lambda_p"], P["lambda_m"]
        fr = False
        for i in range(m_exp):
            dt, drift_dt, comp_p, comp_m, kp_dt, km_dt = consts[i]
            d = d_all[i]
            one_minus = (1.0 - d["u_p"][:, j], 1.0 - d["u_m"][:, j])         # exact in double
            for t in range(int(nb_steps[i])):
                hp, hm = lp * dt, lm * dt
                jp = jm = None
                if one_minus[0][t] <= float(hp) * (1.0 + 1e-6):
                    e = -mp.log(F(float(d["u_p"][t, j])))
                    fr = fr or abs(hp - e) <= fragile_rel * e
                    if hp > e:
                        jp = P["shift_p"] + P["mean_p"] * -mp.log(F(float(d["v_p"][t, j])))
                        jumps[i, 0, j] += 1
                if one_minus[1][t] <= float(hm) * (1.0 + 1e-6):
                    e = -mp.log(F(float(d["u_m"][t, j])))
                    fr = fr or abs(hm - e) <= fragile_rel * e
                    if hm > e:
                        jm = P["shift_m"] - (-P["mean_m"]) * -mp.log(F(float(d["v_m"][t, j])))
                        jumps[i, 1, j] += 1
                m = m + (drift_dt - comp_p * lp - comp_m * lm)
                lp_new = lp + kp_dt * (P["theta_p"] - lp)
                lm_new = lm + km_dt * (P["theta_m"] - lm)
                if jp is not None:
                    m = m + jp
                    lp_new, lm_new = lp_new + P["beta1_p"] * jp, lm_new + P["beta1_m"] * jp
                if jm is not None:
                    m = m + jm
                    lp_new, lm_new = lp_new + P["beta2_p"] * jm, lm_new + P["beta2_m"] * jm
                lp, lm = lp_new, lm_new
            out[i][0][j], out[i][1][j], out[i][2][j] = m, lp, lm
            frag[i, j] = fr
    return out, frag, jumps
