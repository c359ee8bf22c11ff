"""
The data of the paper's two-panel figure on jump risk premia (F. Liu, N. Packham, A. Sepp 2025): one-month implied-vol smiles of
the Hawkes jump-diffusion under the statistical measure (gamma = 0) and under the exponential risk-premia kernel exp(gamma x),
gamma = +1 in one panel and gamma = -1 in the other -- Monte Carlo, all three measures from ONE stepping launch
(hawkesjd_mc_chain_pricer_with_risk_premia_gammas), next to the Fourier pricer under the kernel.  No path leaves the device;
the implied vols are the package's host inversion against each measure's gamma forward.  --densities adds the data of a third
panel: the density of the one-month log-return under gamma = -1, the statistical measure and gamma = +1, simulated (the
exp(gamma x)-weighted kernel density estimate of the resident paths, get_log_return_mc_pdf_device(risk_premia_gamma=)) beside
the Fourier density under the kernel (hawkesjd_pdf_under_risk_kernel), both normalised to sum to one over the grid.

    python examples/risk_premia_mc.py [--paths 100000] [--seed 1] [--steps-per-year 1800] [--densities] [--density-points 41]
"""
import argparse
import dataclasses
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import stochvolmodels_amd as sv  # noqa: E402
from stochvolmodels_amd.engine import get_engine  # noqa: E402
from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps-per-year", type=int, default=hp.NB_STEPS_PER_YEAR)
    ap.add_argument("--densities", action="store_true", help="also print the simulated and Fourier densities of x")
    ap.add_argument("--density-points", type=int, default=41)
    args = ap.parse_args()
    params = sv.HawkesJDParams()
    strikes = np.linspace(0.5, 1.5, 20)
    chain = sv.OptionChain(ttms=np.array([1.0 / 12.0]), forwards=np.array([1.0]), discfactors=np.array([1.0]),
                           strikes_ttms=(strikes,), optiontypes_ttms=(np.where(strikes <= 1.0, "P", "C"),), ids=None)
    kw = params.to_dict()
    kw.pop("risk_premia_gamma")
    gammas = [0.0, 1.0, -1.0]
    eng = get_engine(args.paths)
    eng.start_kernel_timing()
    prices, stderrs, fwds = hp.hawkesjd_mc_chain_pricer_with_risk_premia_gammas(
        ttms=chain.ttms, forwards=chain.forwards, discfactors=chain.discfactors, strikes_ttms=chain.strikes_ttms,
        optiontypes_ttms=chain.optiontypes_ttms, risk_premia_gammas=gammas, nb_path=args.paths, seed=args.seed,
        nb_steps_per_year=args.steps_per_year, return_forwards=True, **kw)
    launches = eng.stop_kernel_timing()
    print(f"stepping launches: {({k: len(v) for k, v in launches.items()})}, {args.paths} paths, {args.steps_per_year} steps per year")
    vols = {g: chain.compute_model_ivols_from_chain_data(model_prices=prices[i], forwards=fwds[i][1])[0] for i, g in enumerate(gammas)}
    for panel, gamma in (("left", 1.0), ("right", -1.0)):
        g = gammas.index(gamma)
        normalizers, gamma_forwards, stats = fwds[g]
        fourier, (f_norm, f_gfwd) = hp.hawkesjd_chain_pricer_with_risk_premia(
            model_params=dataclasses.replace(params, risk_premia_gamma=gamma), ttms=chain.ttms, forwards=chain.forwards,
            discfactors=chain.discfactors, strikes_ttms=chain.strikes_ttms, optiontypes_ttms=chain.optiontypes_ttms,
            return_forwards=True)
        f_vols = chain.compute_model_ivols_from_chain_data(model_prices=fourier, forwards=f_gfwd)[0]
        print(f"\n{panel} panel: gamma = {gamma:+.0f}   normalizer MC {normalizers[0]:.6f} +- {stats[0, 1]:.6f} (Fourier {f_norm[0]:.6f})   "
              f"gamma forward MC {gamma_forwards[0]:.6f} +- {stats[0, 3]:.6f} (Fourier {f_gfwd[0]:.6f})   "
              f"effective sample size {stats[0, 4]:.0f} of {int(stats[0, 5])} kept paths")
        print(" strike type  vol(gamma=0)  vol(gamma) MC  vol(gamma) Fourier  price MC       stderr      price Fourier")
        for k, t, v0, v1, vf, p, e, pf in zip(strikes, chain.optiontypes_ttms[0], vols[0.0], vols[gamma], f_vols, prices[g][0],
                                              stderrs[g][0], fourier[0]):
            print(f" {k:6.4f}  {t}    {v0:11.4f}  {v1:13.4f}  {vf:18.4f}  {p:12.6e}  {e:10.3e}  {pf:12.6e}")
    if args.densities:
        print_densities(params, float(chain.ttms[0]), args)


def print_densities(params, ttm, args):
    """third panel: simulated and Fourier densities of x for gamma in {-1, None, +1} on one grid, as masses summing to one"""
    pricer = sv.HawkesJDPricer()
    x_grid = np.linspace(-0.6, 0.4, args.density_points)
    kw = dict(ttm=ttm, params=params, x_grid=x_grid, nb_path=args.paths, seed=args.seed, nb_steps_per_year=args.steps_per_year)
    plain = pricer.get_log_return_mc_pdf_device(**kw)
    tilted, stats = pricer.get_log_return_mc_pdf_device(risk_premia_gamma=[-1.0, 1.0], return_stats=True, **kw)
    mc = {-1.0: tilted[0], None: plain, 1.0: tilted[1]}
    fourier = {}
    for gamma in (-1.0, None, 1.0):
        f = hp.hawkesjd_pdf_under_risk_kernel(params, 0.0 if gamma is None else gamma, ttm, x_grid)
        fourier[gamma] = f / np.nansum(f)
    print(f"\nthird panel: density of x at ttm = {ttm:.4f}, masses on {x_grid.size} points; effective sample size "
          f"{stats[0]['neff']:.0f} (gamma = -1), {stats[1]['neff']:.0f} (gamma = +1) of {stats[0]['n_kept']} kept paths")
    print("       x   MC(gamma=-1)  Fourier(-1)   MC(none)  Fourier(none)   MC(gamma=+1)  Fourier(+1)")
    for i, x in enumerate(x_grid):
        print(f" {x:7.4f}  {mc[-1.0][i]:12.6e} {fourier[-1.0][i]:12.6e} {mc[None][i]:12.6e} {fourier[None][i]:12.6e} "
              f"{mc[1.0][i]:12.6e} {fourier[1.0][i]:12.6e}")


if __name__ == "__main__":
    main()
