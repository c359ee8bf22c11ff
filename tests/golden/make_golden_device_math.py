"""
Generate tests/golden/device_math.npz, the high-precision references of tests/test_gpu_device_math.py that are too slow to
evaluate in the test itself.  Everything is evaluated here in mpmath at 40 significant digits from the formulas alone (no
reference code, no GPU):

    python tests/golden/make_golden_device_math.py

  heston_*   the closed-form Heston log-MGF of heston_mgf_grid_kernel (csrc/svmc_analytic.hip; the expressions of the
             reference's heston_pricer.py:183-214, started from a_t0 = b_t0 = 0) for every parameter set of HESTON_SETS at
             every maturity of HESTON_TTMS, on the LOG_RETURN phi grid of the set (get_phi_grid at the pricer's vol_scaler for
             the shortest maturity, stored as heston_vol_scaler) and on every PSI_STRIDE-th point of the Q_VAR psi grid.
             NaN where the formula divides by zero (zeta = 0).
  black_*    Black-76 quotes with their exact implied vol: the price of each (F, K, T, discfactor, type, vol) formed in mpmath
             and rounded to double -- for IC / IP the price of the inverse option, i.e. the vanilla price over the forward --
             and, per quote, the undiscounted time value per unit forward, the relative conditioning of the inversion,
             cond = 2^-53 (P + F N(d1) + K N(d2)) / (vega vol) -- the relative vol error that one rounding of the quoted price
             P, of the moneyness log(F / K) (whose price derivative is K N(d2)) or of the price's two terms accounts for; the
             terms are those of the side the solver works on, the out-of-the-money one -- and the smaller of that side's two
             probabilities N(+-d1), N(+-d2) (below 1e-300 the double evaluation underflows).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import mpmath as mp  # noqa: E402
import numpy as np  # noqa: E402

from stochvolmodels_amd.utils.mgf_pricer import get_phi_grid, get_psi_grid  # noqa: E402

mp.mp.dps = 40

# (v0, theta, kappa, rho, volvol)
HESTON_SETS = {
    "base": (0.04, 0.04, 4.0, -0.5, 0.4),           # tests/golden/analytic.npz heston_base_params
    "btc": (0.8, 1.0, 2.0, 0.0, 2.0),               # heston_btc_params (BTC_HESTON_PARAMS)
    "feller": (0.09, 0.05, 0.8, -0.7, 1.5),         # 2 kappa theta = 0.08 < volvol^2 = 2.25
    "volvol_small": (0.04, 0.06, 1.5, -0.3, 0.01),
    "kappa_tiny": (0.05, 0.05, 1e-3, -0.4, 0.5),
    "kappa_big": (0.05, 0.04, 50.0, -0.4, 0.5),
    "rho_minus": (0.04, 0.04, 2.0, -0.99, 0.6),
    "rho_plus": (0.04, 0.04, 2.0, 0.99, 0.6),
}
HESTON_TTMS = np.array([1.0 / 365.0, 0.25, 5.0, 30.0])
PSI_STRIDE = 40


def heston_vol_scaler(v0: float) -> float:
    """heston_chain_pricer's vol_scaler for a chain whose first expiry is the shortest maturity here"""
    return float(np.minimum(0.3, np.sqrt(v0 * HESTON_TTMS[0])))


def heston_grids(name: str):
    v0 = HESTON_SETS[name][0]
    phi = get_phi_grid(is_spot_measure=True, vol_scaler=heston_vol_scaler(v0))
    psi_q = get_psi_grid()[::PSI_STRIDE]
    return (np.concatenate([phi, np.zeros_like(psi_q)]), np.concatenate([np.zeros_like(phi), psi_q]))


def heston_log_mgf_mp(ph, ps, ttm, v0, theta, kappa, rho, volvol):
    ph, ps, ttm = mp.mpc(ph), mp.mpc(ps), mp.mpf(ttm)
    v0, theta, kappa, rho, volvol = (mp.mpf(float(a)) for a in (v0, theta, kappa, rho, volvol))
    volvol2 = volvol * volvol
    b1 = rho * volvol * ph + kappa
    b0 = ph * (ph + 1) / 2 - ps
    zeta = mp.sqrt(b1 * b1 - 2 * volvol2 * b0)
    if zeta == 0:
        return complex(np.nan, np.nan)
    exp_zeta = mp.exp(-ttm * zeta)
    psi_p, psi_m = zeta - b1, zeta + b1
    c_p, c_m = psi_p / (2 * zeta), psi_m / (2 * zeta)
    den = c_p * exp_zeta + c_m
    if den == 0:
        return complex(np.nan, np.nan)
    b_t1 = -(psi_p * c_m - psi_m * c_p * exp_zeta) / (volvol2 * den)
    a_t1 = -(theta * kappa / volvol2) * (ttm * psi_p + 2 * mp.log(den))
    return complex(a_t1 + v0 * b_t1)


def g_heston(out: dict) -> None:
    names = list(HESTON_SETS)
    out["heston_names"] = np.array(names)
    out["heston_params"] = np.array([HESTON_SETS[n] for n in names])
    out["heston_ttms"] = HESTON_TTMS
    out["heston_vol_scaler"] = np.array([heston_vol_scaler(HESTON_SETS[n][0]) for n in names])
    out["heston_psi_stride"] = np.array(PSI_STRIDE)
    for name in names:
        phi, psi = heston_grids(name)
        v0, theta, kappa, rho, volvol = HESTON_SETS[name]
        lm = np.empty((HESTON_TTMS.size, phi.size), dtype=np.complex128)
        for i, ttm in enumerate(HESTON_TTMS):
            lm[i] = [heston_log_mgf_mp(a, b, ttm, v0, theta, kappa, rho, volvol) for a, b in zip(phi, psi)]
        out[f"heston_log_mgf_{name}"] = lm
        print(name, "non-finite:", int(np.sum(~np.isfinite(lm))), flush=True)


def black_mp(F, K, sqrt_t, vol, is_call):
    """undiscounted Black-76 price, vega, the sum of the price's two terms and the smaller of its two probabilities"""
    F, K, sv = mp.mpf(F), mp.mpf(K), mp.mpf(vol) * mp.mpf(sqrt_t)
    d1 = mp.log(F / K) / sv + sv / 2
    d2 = d1 - sv
    s = 1 if is_call else -1
    n1, n2 = mp.ncdf(s * d1), mp.ncdf(s * d2)
    vega = F * mp.npdf(d1) * mp.mpf(sqrt_t)
    return s * (F * n1 - K * n2), vega, F * n1 + K * n2, min(n1, n2)


BLACK_TTMS = (1.0 / 365.0, 1.0 / 52.0, 0.25, 1.0, 5.0, 30.0)
BLACK_VOLS = (1e-6 * (1 + 1e-6), 1e-3, 0.01, 0.2, 1.0, 3.0, 9.9)
BLACK_M = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0, 8.0, -8.0)     # log(K / F) in standard deviations vol sqrt(T)
TAIL_M = (12.0, -12.0, 20.0, -20.0, 30.0, -30.0, 37.0, -37.0)


def g_black(out: dict) -> None:
    rows = []                        # F, K, T, df, code, vol
    for F in (1.0, 100.0):
        for df in (1.0, 0.5):
            for T in BLACK_TTMS:
                for vol in BLACK_VOLS:
                    for m in BLACK_M:
                        K = float(F * np.exp(m * vol * np.sqrt(T)))
                        for code in (0, 1):
                            rows.append((F, K, T, df, code, vol))
                        if F == 100.0 and df == 0.5:
                            for code in (2, 3):
                                rows.append((F, K, T, df, code, vol))
            for T in (1.0 / 365.0, 1.0, 30.0):                                      # the far tails: prices down to 1e-300
                for vol in (0.01, 0.2, 1.0):
                    for m in TAIL_M:
                        K = float(F * np.exp(m * vol * np.sqrt(T)))
                        for code in (0, 1):
                            rows.append((F, K, T, df, code, vol))
    rows = np.array(rows)
    price, tv, cond, prob = (np.empty(len(rows)) for _ in range(4))
    for i, (F, K, T, df, code, vol) in enumerate(rows):
        call = code in (0, 2)
        p = black_mp(F, K, np.sqrt(T), vol, call)[0]
        otm, vega, terms, pr = black_mp(F, K, np.sqrt(T), vol, K >= F)         # the time value: the out-of-the-money side
        quote = df * p / F if code >= 2 else df * p
        price[i] = float(quote)
        tv[i] = float(otm / F)
        cond[i] = float(mp.mpf(2) ** -53 * (p + terms) / (vega * mp.mpf(vol))) if vega > 0 else np.inf
        prob[i] = float(pr)
    out["black_F"], out["black_K"], out["black_T"], out["black_df"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    out["black_code"], out["black_vol"] = rows[:, 4].astype(np.int8), rows[:, 5]
    out["black_price"], out["black_time_value"], out["black_cond"], out["black_min_prob"] = price, tv, cond, prob
    print("black quotes:", len(rows), " min price", float(price[price > 0].min()), flush=True)


def main() -> None:
    out = {}
    g_black(out)
    g_heston(out)
    path = os.path.join(HERE, "device_math.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
