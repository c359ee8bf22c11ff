"""
The impermanent-loss profile of a concentrated-liquidity range under the LogSV model: the loss of a position of 10^6 notional
over [2000, 2400] opened at 2200, ten days out, at 101 forwards -- the Fourier pricer (one ODE launch and one slice launch for
the whole profile, where the reference's np.vectorize form re-solves the ODEs per forward) beside the Monte Carlo estimate on
one resident path set, with the pieces the loss is hedged by: a put and a digital put at the lower end, a call and a digital
call at the upper end and the square-root payoff between them.  The parameter set is the one of the reference's
papers/il_hedging/run_logsv_for_il_payoff.py; its volvol of 3.27 is where the second-order expansion starts to show, and all
forwards share one path set, so the z column drifts together (a few standard errors at 400 000 paths).

    python examples/il_hedging.py [--paths 400000] [--seed 1] [--ttm-days 10]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import stochvolmodels_amd as sv  # noqa: E402

PARAMS = sv.LogSvParams(sigma0=0.4861785891939535, theta=0.6176006871606874, kappa1=1.955809653686808, kappa2=1.978367101612294,
                        beta=-0.26916969112829325, volvol=3.265815229306317)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=400000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ttm-days", type=float, default=10.0)
    args = ap.parse_args()
    ttm, p0, pa, pb = args.ttm_days / 365.0, 2200.0, 2000.0, 2400.0
    forwards = np.linspace(1800.0, 2600.0, 101)
    fourier, pieces = sv.logsv_il_pricer_vector(PARAMS, ttm, forwards, p0, pa, pb, return_pieces=True)
    mc, stderr, extra = sv.LogSVPricer().model_mc_il_payoff(PARAMS, ttm, forwards, p0, pa, pb, nb_path=args.paths, seed=args.seed,
                                                            return_pieces=True)
    print(f"impermanent loss of [{pa:.0f}, {pb:.0f}] opened at {p0:.0f}, notional 1e6, ttm {ttm:.4f}; Monte Carlo on {extra['n_kept']} paths")
    print(" forward    Fourier IL       MC IL     stderr      z     put(pa)   call(pb)  dig.put  dig.call  sqrt piece")
    for i, f in enumerate(forwards):
        z = (fourier[i] - mc[i]) / stderr[i]
        print(f" {f:7.1f}  {fourier[i]:12.3f} {mc[i]:12.3f} {stderr[i]:9.3f} {z:7.2f}  {pieces['put'][i]:9.4f} {pieces['call'][i]:9.4f} "
              f"{pieces['digital_put'][i]:8.5f} {pieces['digital_call'][i]:8.5f} {pieces['square_root'][i]:10.6f}")
    print(f"largest |Fourier - MC| / stderr over the profile: {np.max(np.abs(fourier - mc) / stderr):.2f}")


if __name__ == "__main__":
    main()
