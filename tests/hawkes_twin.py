"""
CPU twin of the Hawkes jump-diffusion generator (csrc/svmc_hawkes.hip), in NumPy.

It materialises the generator's random streams -- Philox4x32-7 vectorised, the stream's piecewise-cubic inverse normal CDF
evaluated with an exactly rounded emulated fma -- and restates simulate_hawkesjd_terminal of the reference
(pricers/hawkes_jd_pricer.py:715-776) in the reference's own order of operations.  tests/golden/make_golden_hawkes.py feeds the
same draws to the unmodified reference; tests/test_hawkes_golden.py holds this twin to those fixtures and its pieces to the C
oracle, and tests/test_gpu_hawkes.py holds the device to the fixtures.

Stream layout (csrc/svmc_rng.h): Philox4x32-7, key = seed, counter = (path_lo, path_hi, step, stream | call_id << 8) with the
chain-global step index.  Stream 6: word 0 -> N(0,1), words 1, 2 -> u_p, u_m = (r + 1/2) 2^-32.  Stream 7 (drawn on the device
only where a side jumps): E_p = -ln((r0 + 1/2) 2^-32), E_m = -ln((r1 + 1/2) 2^-32).
"""
from __future__ import annotations

import os
import re
from typing import Dict, Tuple

import numpy as np

from oracle.oracle import np_payoff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ICDF_HEADER = os.path.join(ROOT, "stochvolmodels_amd", "csrc", "svmc_icdf_table.h")
HAWKES_STREAM, HAWKES_JUMP_STREAM = 6, 7
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
PARAM_NAMES = ("mu", "sigma", "shift_p", "mean_p", "shift_m", "mean_m", "lambda_p", "theta_p", "kappa_p", "beta1_p", "beta2_p",
               "lambda_m", "theta_m", "kappa_m", "beta1_m", "beta2_m")


# ---- Philox4x32 ----------------------------------------------------------------------------------------------------------
def philox4x32(c0, c1, c2, c3, k0: int, k1: int, rounds: int = 7) -> Tuple[np.ndarray, ...]:
    """Philox4x32-`rounds` of the counter words (arrays, broadcast together) under the key (k0, k1)"""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(rounds):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK32]
        k0 = (k0 + np.uint64(W0)) & MASK32
        k1 = (k1 + np.uint64(W1)) & MASK32
    return tuple(v.astype(np.uint32) for v in c)


def stream_words(seed: int, call_id: int, stream: int, path0: int, n_path: int, step0: int, nb_steps: int):
    """the four words of every (step, path) call of one stream: arrays [nb_steps, n_path]"""
    path = np.arange(path0, path0 + n_path, dtype=np.uint64)[None, :]
    step = np.arange(step0, step0 + nb_steps, dtype=np.uint64)[:, None]
    return philox4x32(path & MASK32, path >> np.uint64(32), step, np.uint64(stream | (call_id << 8)), seed & 0xFFFFFFFF,
                      (seed >> 32) & 0xFFFFFFFF)


# ---- exactly rounded fma in NumPy (Boldo & Melquiond, "Emulation of FMA and correctly rounded sums", IEEE TC 2008) -------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _round_to_odd_sum(a, b):
    s, e = _two_sum(a, b)
    even = (s.view(np.int64) & 1) == 0
    bump = (e != 0) & even
    return np.where(bump, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)


def fma(a, b, c):
    """a * b + c with one rounding (finite, non-underflowing operands), elementwise"""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(a, b, c))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, uh)
    return th + _round_to_odd_sum(tl, ul)


# ---- the stream's inverse normal CDF -------------------------------------------------------------------------------------
_TABLE = None


def icdf_table() -> Tuple[int, np.ndarray, np.ndarray]:
    """(M, piece0 [S, 2], piece1 [S, 2]) of the committed table (raw form: the cubic in |t|)"""
    global _TABLE
    if _TABLE is None:
        text = open(ICDF_HEADER).read()
        m = int(re.search(r"#define SVMC_ICDF_M (\d+)", text).group(1))
        assert "#define SVMC_ICDF_RAW 1" in text and "#define SVMC_ICDF_DEG 3" in text and "#define SVMC_ICDF_HALF_LATTICE 0" in text

        def piece(name):
            body = re.search(r"#define " + name + r" \\\n((?:.*\\\n)*.*)\n", text).group(1)   # the continued lines
            vals = [float.fromhex(v) for v in re.findall(r"[-+]?0x[0-9a-fA-F.]+p[-+]?\d+", body)]
            return np.array(vals, dtype=np.float64).reshape(-1, 2)

        _TABLE = (m, piece("SVMC_ICDF_PIECE0_INIT"), piece("SVMC_ICDF_PIECE1_INIT"))
    return _TABLE


def normal_from_words(w) -> np.ndarray:
    """z(w): sign(t) P_j(|t|) with t = (int32) w -- svmc_math.h normal_icdf32 / the oracle's svo_normal_from_word"""
    m, p0, p1 = icdf_table()
    t = np.asarray(w, dtype=np.uint32).view(np.int32).astype(np.float64)
    hi = (t.view(np.uint64) >> np.uint64(32)).astype(np.uint32)
    j = (hi >> np.uint32(20 - m)) & np.uint32(p0.shape[0] - 1)
    a = np.abs(t)
    p = fma(p1[j, 1], a, p1[j, 0])
    p = fma(p, a, p0[j, 1])
    p = fma(p, a, p0[j, 0])
    return np.copysign(p, t)


def uniform_from_words(w) -> np.ndarray:
    """(w + 1/2) 2^-32, exact"""
    return (np.asarray(w, dtype=np.uint32).astype(np.float64) + 0.5) * 2.0 ** -32


def hawkes_draws(seed: int, call_id: int, path0: int, n_path: int, step0: int, nb_steps: int) -> Dict[str, np.ndarray]:
    """the unscaled draws of nb_steps steps from the chain-global step step0, arrays [nb_steps, n_path]: z, u_p, u_m and the
    unit exponentials e_p, e_m of the jump sizes (what the device draws lazily, here for every step)"""
    r = stream_words(seed, call_id, HAWKES_STREAM, path0, n_path, step0, nb_steps)
    e = stream_words(seed, call_id, HAWKES_JUMP_STREAM, path0, n_path, step0, nb_steps)
    return dict(z=normal_from_words(r[0]), u_p=uniform_from_words(r[1]), u_m=uniform_from_words(r[2]),
                e_p=-np.log(uniform_from_words(e[0])), e_m=-np.log(uniform_from_words(e[1])))


# ---- the model -----------------------------------------------------------------------------------------------------------
def time_grid(ttm: float, nb_steps_per_year: int) -> Tuple[int, float]:
    nb = int(ttm * nb_steps_per_year) + 1
    return nb, ttm / nb


def simulate_terminal(ttm, x0, lambda_p0, lambda_m0, params: dict, seed: int, call_id: int = 0, path0: int = 0, step0: int = 0,
                      nb_steps_per_year: int = 1800, stats: dict = None):
    """simulate_hawkesjd_terminal (:715-776) on this stream: the reference's statements, vectorised over paths"""
    p = params
    n = x0.shape[0]
    nb_steps, dt = time_grid(ttm, nb_steps_per_year)
    d = hawkes_draws(seed, call_id, path0, n, step0, nb_steps)
    W0 = np.sqrt(dt) * d["z"]
    U_P = -np.log(d["u_p"]) / dt
    U_M = -np.log(d["u_m"]) / dt
    J_P = p["shift_p"] + p["mean_p"] * d["e_p"]
    J_M = p["shift_m"] - (-p["mean_m"]) * d["e_m"]
    compensator_p_dt = dt * (np.exp(p["shift_p"]) / (1.0 - p["mean_p"]) - 1.0)
    compensator_m_dt = dt * (np.exp(p["shift_m"]) / (1.0 - p["mean_m"]) - 1.0)
    drift_dt = (p["mu"] - 0.5 * p["sigma"] * p["sigma"]) * dt
    for w0, u_p, u_m, j_p, j_m in zip(W0, U_P, U_M, J_P, J_M):
        diffusion = drift_dt - compensator_p_dt * lambda_p0 - compensator_m_dt * lambda_m0 + p["sigma"] * w0
        jump_p = np.where(lambda_p0 > u_p, j_p, 0.0)
        jump_m = np.where(lambda_m0 > u_m, j_m, 0.0)
        if stats is not None:
            stats["jumps_p"] = stats.get("jumps_p", 0) + int(np.count_nonzero(lambda_p0 > u_p))
            stats["jumps_m"] = stats.get("jumps_m", 0) + int(np.count_nonzero(lambda_m0 > u_m))
            stats["both"] = stats.get("both", 0) + int(np.count_nonzero((lambda_p0 > u_p) & (lambda_m0 > u_m)))
        x0 = x0 + diffusion + jump_p + jump_m
        load_p = p["beta1_p"] * jump_p + p["beta2_p"] * jump_m
        load_m = p["beta1_m"] * jump_p + p["beta2_m"] * jump_m
        lambda_p0 = lambda_p0 + p["kappa_p"] * (p["theta_p"] - lambda_p0) * dt + load_p
        lambda_m0 = lambda_m0 + p["kappa_m"] * (p["theta_m"] - lambda_m0) * dt + load_m
    return x0, lambda_p0, lambda_m0, nb_steps


def mc_chain(ttms, forwards, discfactors, strikes_ttms, types_ttms, params: dict, n_path: int, seed: int, call_id: int = 0,
             nb_steps_per_year: int = 1800, keep: int = 0, stats: dict = None):
    """hawkesjd_mc_chain_pricer (:643-711) on this stream: (prices, stderrs, [state of the first `keep` paths per expiry])"""
    x = np.zeros(n_path)
    lp = params["lambda_p"] * np.ones(n_path)
    lm = params["lambda_m"] * np.ones(n_path)
    t0, step0 = 0.0, 0
    prices, stderrs, states = [], [], []
    for ttm, f, df, k, t in zip(ttms, forwards, discfactors, strikes_ttms, types_ttms):
        x, lp, lm, nb = simulate_terminal(ttm - t0, x, lp, lm, params, seed, call_id, 0, step0, nb_steps_per_year, stats)
        step0 += nb
        t0 = ttm
        pr, sd = np_payoff(x, x, ttm, f, np.asarray(k), np.asarray(t), df)   # compute_mc_vars_payoff, LOG_RETURN
        prices.append(pr)
        stderrs.append(sd)
        states.append(np.stack([x[:keep], lp[:keep], lm[:keep]]))
    return prices, stderrs, states
