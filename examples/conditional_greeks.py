"""
Delta and gamma of one option chain from the conditional Monte Carlo estimator, with their errors, beside the pathwise delta of the
plain estimator; and the simulated density of the log-return three ways on one grid.

Given the path of the volatility's driver the discretised log-return is Gaussian, so a path contributes a Black-76 price and its
closed-form derivatives: the delta has the conditional price's variance reduction, and the gamma -- a density estimate at the strike
on the plain estimator, which has none -- comes with an error too.  The pathwise delta runs on another random stream: the two
columns are independent estimates of one number.

The density: K x dual gamma at K = exp(x) is the simulated density of the log-return WITHOUT a bandwidth, printed beside the Fourier
density (logsv_pdfs, bin masses divided by the step) and the Gaussian kernel estimate of the plain paths (terminal_value_kdes).

    python examples/conditional_greeks.py [--paths 100000] [--seed 7]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stochvolmodels_amd as sv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    p = sv.LOGSV_BTC_PARAMS
    ttms, k = np.array([1 / 12, 0.25, 0.5, 1.0]), np.linspace(0.7, 1.3, 13)
    forwards, dfs = np.ones(4), np.ones(4)
    types = [np.where(k < 1.0, "P", "C")] * 4
    etas = p.get_vol_backbone_etas(ttms=ttms)
    cond = sv.logsv_mc_chain_greeks_conditional(ttms, forwards, dfs, [k] * 4, types, v0=p.sigma0, theta=p.theta, kappa1=p.kappa1,
                                                kappa2=p.kappa2, beta=p.beta, volvol=p.volvol, vol_backbone_etas=etas,
                                                nb_path=a.paths, seed=a.seed)
    plain = sv.logsv_mc_chain_greeks(p, ttms, forwards, dfs, [k] * 4, types, wrt=(), nb_path=a.paths, seed=a.seed)
    for i, ttm in enumerate(ttms):
        print(f"\nttm {ttm:.4f}")
        print("  strike type      price  +-        delta  +-        gamma  +-        pathwise delta  +-      error ratio")
        for j, strike in enumerate(k):
            print(f"  {strike:6.3f} {types[i][j]:>4}  {cond['price'][i][j]:9.6f} {cond['stderr'][i][j]:.1e}  {cond['delta'][i][j]:+8.5f} "
                  f"{cond['delta_stderr'][i][j]:.1e}  {cond['gamma'][i][j]:8.4f} {cond['gamma_stderr'][i][j]:.1e}  "
                  f"{plain['delta'][i][j]:+8.5f}       {plain['delta_stderr'][i][j]:.1e}  "
                  f"{plain['delta_stderr'][i][j] / cond['delta_stderr'][i][j]:6.1f}")

    ttm, x = 0.25, np.linspace(-0.6, 0.4, 21)
    pricer = sv.LogSVPricer()
    pdf, err = pricer.get_log_return_mc_pdf_conditional(p, ttm, x, nb_path=a.paths, seed=a.seed, return_stderr=True)
    fourier = pricer.logsv_pdfs(p, ttm, x) / (x[1] - x[0])
    kde = pricer.terminal_value_kdes(p, ttm, nb_path=a.paths, seed=a.seed,
                                     space_grids={sv.VariableType.LOG_RETURN: x})[sv.VariableType.LOG_RETURN]
    print(f"\ndensity of the log-return at ttm {ttm}")
    print("       x   conditional  +-        Fourier    kernel estimate")
    for j, xj in enumerate(x):
        print(f"  {xj:+6.3f}  {pdf[j]:10.5f}  {err[j]:.1e}  {fourier[j]:10.5f}  {np.ravel(kde)[j]:10.5f}")


if __name__ == "__main__":
    main()
