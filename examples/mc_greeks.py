"""
Monte Carlo deltas and sigma0 sensitivities of one option chain, with their errors.

The base parameters and the pair sigma0 +- h are stepped by one launch on one random stream, so the difference of the two bumped
prices is a common-random-numbers estimate: its error, from the per-path paired differences, is orders below what two independent
prices would give.  The delta is the pathwise derivative of the plain estimator in the forward.

Beside them, as a HOST composition, the minimum-variance delta  delta + (beta / F) d price / d sigma0  of the LogSV dynamics
(d sigma = ... + beta sigma dW0: a move of the forward carries beta / F of it into the volatility).  It is printed WITHOUT an
error: the two figures come from the same paths and are correlated, and the call returns no covariance between them.

    python examples/mc_greeks.py [--paths 100000] [--seed 7]
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
    forwards = np.ones(4)
    types = [np.where(k < 1.0, "P", "C")] * 4
    out = sv.logsv_mc_chain_greeks(p, ttms, forwards, np.ones(4), [k] * 4, types, wrt=("sigma0",), nb_path=a.paths, seed=a.seed)
    for i, ttm in enumerate(ttms):
        print(f"\nttm {ttm:.4f}")
        print("  strike type      price  +-        delta  +-        dual delta  +-        d/dsigma0  +-        pairs    min-var delta (no error)")
        for j, strike in enumerate(k):
            sens = out["sens"]["sigma0"][i][j]
            mv = out["delta"][i][j] + p.beta / forwards[i] * sens
            print(f"  {strike:6.3f} {types[i][j]:>4}  {out['price'][i][j]:9.6f} {out['stderr'][i][j]:.1e}  {out['delta'][i][j]:+8.5f} "
                  f"{out['delta_stderr'][i][j]:.1e}  {out['dual_delta'][i][j]:+9.5f}  {out['dual_delta_stderr'][i][j]:.1e}  "
                  f"{sens:+9.6f} {out['sens_stderr']['sigma0'][i][j]:.1e}  {out['n_pairs']['sigma0'][i][j]:7d}  {mv:+8.5f}")


if __name__ == "__main__":
    main()
