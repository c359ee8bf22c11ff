"""
The sensitivity of one option chain to the start volatility -- vega in its model form -- from the conditional Monte Carlo estimator,
with the error of the difference, beside the plain estimator's.

Both difference two prices at sigma0 +- h on common random numbers, stepped by one launch, and report the error of that DIFFERENCE
from the per-path paired differences.  The conditional estimator has no indicator in it: a path contributes a Black-76 price, which
is smooth in the parameters.  The two run on different random streams: the columns are independent estimates of one number.

    python examples/conditional_vega.py [--paths 100000] [--seed 7] [--model logsv|heston]
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
    ap.add_argument("--model", choices=("logsv", "heston"), default="logsv")
    a = ap.parse_args()
    ttms, k = np.array([1 / 12, 0.25, 0.5, 1.0]), np.linspace(0.7, 1.3, 13)
    forwards, dfs = np.ones(4), np.ones(4)
    types = [np.where(k < 1.0, "P", "C")] * 4
    if a.model == "logsv":
        p, name = sv.LOGSV_BTC_PARAMS, "sigma0"
        cond = sv.logsv_mc_chain_greeks_conditional(ttms, forwards, dfs, [k] * 4, types, v0=p.sigma0, theta=p.theta, kappa1=p.kappa1,
                                                    kappa2=p.kappa2, beta=p.beta, volvol=p.volvol,
                                                    vol_backbone_etas=p.get_vol_backbone_etas(ttms=ttms), nb_path=a.paths, seed=a.seed,
                                                    wrt=(name,))
        plain = sv.logsv_mc_chain_greeks(p, ttms, forwards, dfs, [k] * 4, types, wrt=(name,), nb_path=a.paths, seed=a.seed)
    else:
        p, name = sv.HestonParams(v0=0.64, theta=0.8, kappa=2.0, rho=-0.4, volvol=1.2), "v0"
        cond = sv.heston_mc_chain_greeks_conditional(ttms, forwards, dfs, [k] * 4, types, v0=p.v0, theta=p.theta, kappa=p.kappa, rho=p.rho,
                                                     volvol=p.volvol, nb_path=a.paths, seed=a.seed, wrt=(name,))
        plain = sv.heston_mc_chain_greeks(p, ttms, forwards, dfs, [k] * 4, types, wrt=(name,), nb_path=a.paths, seed=a.seed)
    for i, ttm in enumerate(ttms):
        print(f"\nttm {ttm:.4f}")
        print(f"  strike type      price  +-        d price / d {name}: conditional  +-      plain  +-      error ratio   pairs")
        for j, strike in enumerate(k):
            ce, pe = cond["sens_stderr"][name][i][j], plain["sens_stderr"][name][i][j]
            print(f"  {strike:6.3f} {types[i][j]:>4}  {cond['price'][i][j]:9.6f} {cond['stderr'][i][j]:.1e}  "
                  f"{cond['sens'][name][i][j]:+22.6f}  {ce:.1e}  {plain['sens'][name][i][j]:+9.6f}  {pe:.1e}  {pe / ce:8.1f}  "
                  f"{cond['n_pairs'][name][i][j]:7d}")


if __name__ == "__main__":
    main()
