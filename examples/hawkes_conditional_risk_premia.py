"""
The paper's slice of the Hawkes jump-diffusion under the exponential risk-premia kernel exp(gamma x), three ways side by side: the
Fourier pricer under the kernel, the plain Monte Carlo under it and the conditional Monte Carlo under it (row f17).

Given a path's jumps the log-return is Gaussian, x ~ N(mu, sigma^2 T), and the Esscher identity turns the weighted payoff of a path
into the weight exp(gamma mu + gamma^2 cv / 2) -- no diffusion noise in it -- times a Black-76 price at the forward shifted by gamma cv.
The two Monte Carlo columns come from independent random streams (6 and 7; 9 and 10), so they differ by noise; both are undiscounted
and at forward 1, where the Fourier pricer prices the same payoff.

    python examples/hawkes_conditional_risk_premia.py [--paths 100000] [--seed 7] [--gammas -1 1]
"""
import argparse
import dataclasses
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stochvolmodels_amd as sv  # noqa: E402
from stochvolmodels_amd.pricers.hawkes_jd_pricer import hawkesjd_chain_pricer_with_risk_premia  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--gammas", type=float, nargs="+", default=[-1.0, 1.0])
    a = ap.parse_args()
    k = np.linspace(0.5, 1.5, 20)
    chain = dict(ttms=np.array([1.0 / 12.0]), forwards=np.array([1.0]), discfactors=np.array([1.0]), strikes_ttms=[k],
                 optiontypes_ttms=[np.where(k <= 1.0, "P", "C")])
    params = sv.HawkesJDParams()
    kw = params.to_dict()
    kw.pop("risk_premia_gamma")
    common = dict(risk_premia_gammas=a.gammas, nb_path=a.paths, seed=a.seed, return_forwards=True, **chain, **kw)
    pp, pe, pf = sv.hawkesjd_mc_chain_pricer_with_risk_premia_gammas(**common)
    cp, ce, cf = sv.hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas(**common)
    for g, gamma in enumerate(a.gammas):
        ref, (norm, gfwd) = hawkesjd_chain_pricer_with_risk_premia(model_params=dataclasses.replace(params, risk_premia_gamma=gamma),
                                                                   return_forwards=True, **chain)
        ps, cs = pf[g][2][0], cf[g][2][0]
        print(f"\ngamma {gamma:+.2f}: normalizer Fourier {norm[0]:.6f}, plain {ps[0]:.6f} +- {ps[1]:.1e}, conditional {cs[0]:.6f} +- {cs[1]:.1e}")
        print(f"            gamma forward Fourier {gfwd[0]:.6f}, plain {ps[2]:.6f} +- {ps[3]:.1e}, conditional {cs[2]:.6f} +- {cs[3]:.1e}")
        print(f"            effective sample size / n: plain {ps[4] / a.paths:.3f}, conditional {cs[4] / a.paths:.3f}")
        print("  strike type    Fourier      plain    +-          conditional  +-          error^2 ratio")
        for j, strike in enumerate(k):
            ratio = (pe[g][0][j] / ce[g][0][j]) ** 2 if ce[g][0][j] > 0 else float("inf")
            print(f"  {strike:6.3f} {chain['optiontypes_ttms'][0][j]:>4}  {ref[0][j]:10.6f} {pp[g][0][j]:10.6f} {pe[g][0][j]:.2e}    "
                  f"{cp[g][0][j]:10.6f}   {ce[g][0][j]:.2e}    {ratio:8.2f}")


if __name__ == "__main__":
    main()
