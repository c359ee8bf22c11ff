"""
Plain and conditional Monte Carlo prices of one option chain under the Hawkes jump-diffusion, side by side, and the bandwidth-free
density of the log-return beside the Fourier one.

The model's diffusion sigma w0 is independent of its jumps and intensities: given a path's jumps the discretised log-return is
Gaussian with the variance sigma^2 T on every path, so the conditional pricer averages a Black-76 price per path instead of a payoff
-- the same expectation for the same discretised model, a smaller error, no normal drawn.  The two columns come from independent
random streams (the plain pricer draws streams 6 and 7, the conditional one 9 and 10), so they differ by noise.  The density column
is K dual_gamma at K = exp(x), times the grid's spacing, beside the bin masses of hawkesjd_pdf_under_risk_kernel at gamma 0.

    python examples/hawkes_conditional_mc.py [--paths 100000] [--seed 7]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stochvolmodels_amd as sv  # noqa: E402
from stochvolmodels_amd.pricers.hawkes_jd_pricer import hawkesjd_mc_chain_pricer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    ttms = np.array([1 / 52, 1 / 12, 0.25])
    k = np.round(np.arange(0.8, 1.2001, 0.05), 2)
    chain = dict(ttms=ttms, forwards=np.ones(3), discfactors=np.ones(3), strikes_ttms=[k] * 3,
                 optiontypes_ttms=[np.where(k < 1.0, "P", "C")] * 3, nb_path=a.paths)
    params = sv.HawkesJDParams()
    kw = params.to_dict()
    pp, pe = hawkesjd_mc_chain_pricer(seed=a.seed, **chain, **kw)
    cp, ce, stats = sv.hawkesjd_mc_chain_pricer_conditional(seed=a.seed, return_stats=True, **chain, **kw)
    for i, ttm in enumerate(ttms):
        st = stats[i]
        print(f"\nttm {ttm:.4f}: mean F_c {st['forward_mc']:.6f} +- {st['forward_mc_stderr']:.1e}, corr {st['corr']:+.2e}, "
              f"kept {st['n_kept']}, dropped {st['n_dropped']}")
        print("  strike type      plain    +-          conditional  +-          variance ratio")
        for j, strike in enumerate(k):
            ratio = (pe[i][j] / ce[i][j]) ** 2 if ce[i][j] > 0 else float("inf")
            print(f"  {strike:6.2f} {chain['optiontypes_ttms'][i][j]:>4}  {pp[i][j]:10.6f} {pe[i][j]:.2e}    {cp[i][j]:10.6f}   {ce[i][j]:.2e}    {ratio:8.1f}")
    ttm, x = 1 / 12, np.linspace(-0.6, 0.6, 25)
    pdf, err = sv.HawkesJDPricer().get_log_return_mc_pdf_conditional(params, ttm, x, nb_path=a.paths, seed=a.seed, return_stderr=True)
    fourier = sv.hawkesjd_pdf_under_risk_kernel(params, 0.0, ttm, x)
    dx = x[1] - x[0]
    print(f"\nlog-return density at ttm {ttm:.4f}, as masses of bins of width {dx:.3f}")
    print("       x   conditional MC  +-          Fourier")
    for xj, d, e, f in zip(x, pdf * dx, err * dx, fourier):
        print(f"  {xj:+6.3f}   {d:12.6e}  {e:.1e}    {f:12.6e}")


if __name__ == "__main__":
    main()
