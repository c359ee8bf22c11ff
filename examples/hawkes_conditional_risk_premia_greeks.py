"""
The paper's slice of the Hawkes jump-diffusion under the exponential risk-premia kernel exp(gamma x): the Greeks of the conditional
Monte Carlo price under the kernel with their errors, and the density of the log-return under the kernel three
ways -- the conditional estimator's, which needs no bandwidth, the weighted kernel density estimate (row f9) and the Fourier density.

Given a path's jumps the log-return is Gaussian, x ~ N(mu, sigma^2 T); the weight exp(gamma mu + gamma^2 cv / 2) depends on neither the
forward nor the strike, so delta, dual delta, gamma and dual gamma are weighted means of per-path Black-76 derivatives at the forward
shifted by gamma cv, and K dual_gamma at K = exp(x) is the density.  Everything is undiscounted and at forward 1.

    python examples/hawkes_conditional_risk_premia_greeks.py [--paths 100000] [--seed 7] [--gammas -1 1]
"""
import argparse
import dataclasses
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stochvolmodels_amd as sv  # noqa: E402
from stochvolmodels_amd.pricers.hawkes_jd_pricer import hawkesjd_pdf_under_risk_kernel  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--gammas", type=float, nargs="+", default=[-1.0, 1.0])
    a = ap.parse_args()
    ttm = 1.0 / 12.0
    k = np.linspace(0.5, 1.5, 20)
    chain = dict(ttms=np.array([ttm]), forwards=np.array([1.0]), discfactors=np.array([1.0]), strikes_ttms=[k],
                 optiontypes_ttms=[np.where(k <= 1.0, "P", "C")])
    params, pricer = sv.HawkesJDParams(), sv.HawkesJDPricer()
    kw = params.to_dict()
    kw.pop("risk_premia_gamma")
    greeks = sv.hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas(risk_premia_gammas=a.gammas, nb_path=a.paths, seed=a.seed,
                                                                             return_stats=True, **chain, **kw)
    x = np.linspace(-0.5, 0.5, 21)
    pdf, err = pricer.get_log_return_mc_pdf_conditional_under_risk_kernel(params, ttm, x, a.gammas, nb_path=a.paths, seed=a.seed,
                                                                          return_stderr=True)
    kde = pricer.get_log_return_mc_pdf_device(ttm, params, x, nb_path=a.paths, seed=a.seed, risk_premia_gamma=a.gammas)
    for g, gamma in enumerate(a.gammas):
        d, st = greeks[g], greeks[g]["stats"][0]
        print(f"\ngamma {gamma:+.2f}: kept {st['n_kept']} of {a.paths} paths, effective sample size / n {st['effective_sample_size'] / a.paths:.3f}")
        print("  strike type      price  +-            delta  +-        dual delta  +-            gamma  +-        F delta + K dual delta")
        for j, strike in enumerate(k):
            print(f"  {strike:6.3f} {chain['optiontypes_ttms'][0][j]:>4} {d['price'][0][j]:10.6f}  {d['stderr'][0][j]:.1e}  "
                  f"{d['delta'][0][j]:+10.6f}  {d['delta_stderr'][0][j]:.1e}  {d['dual_delta'][0][j]:+10.6f}  {d['dual_delta_stderr'][0][j]:.1e}  "
                  f"{d['gamma'][0][j]:10.6f}  {d['gamma_stderr'][0][j]:.1e}  {d['delta'][0][j] + strike * d['dual_delta'][0][j]:10.6f}")
        # the Fourier routine returns bin masses: all three are shown normalised on the grid
        ref = hawkesjd_pdf_under_risk_kernel(dataclasses.replace(params, risk_premia_gamma=gamma), gamma, ttm, x)
        norm = lambda v: np.asarray(v) / np.sum(v)      # noqa: E731
        print("        x   conditional  +- (relative)   weighted KDE   Fourier    (each normalised on the grid)")
        for j, xj in enumerate(x):
            print(f"  {xj:+7.3f}   {norm(pdf[g])[j]:10.6f}   {err[g][j] / pdf[g][j]:.1e}       {norm(kde[g])[j]:10.6f}  {norm(ref)[j]:10.6f}")


if __name__ == "__main__":
    main()
