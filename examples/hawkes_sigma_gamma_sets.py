"""
Every (sigma, gamma) of a Hawkes chain on ONE set of jump paths.

In the conditional step of the Hawkes jump-diffusion the jump decisions, the jump sizes and both intensities depend on neither sigma nor
the risk-premia gamma, and sigma enters a path's conditional mean only through the deterministic -sigma^2 dt / 2 of every step.  So one
stepping launch at sigma = 0 leaves rows a_j with x_T | jumps ~ N(a_j - v / 2, v), v = sigma^2 T one number per expiry, and every
(sigma, gamma) is a tail on those rows (svmc_jump_sets_payoff_chain, include/svmc_est.h): no second stepping launch.

Two uses:
  1. a (sigma, gamma) surface of one option: hawkesjd_jump_rows once, HawkesJumpRows.price_sets for the whole grid;
  2. a calibration of (sigma, gamma) with estimator="conditional": the stepping is paid once, every objective evaluation is a tail.
     The market is the model's own prices at (sigma*, gamma*) on these paths, so the objective is zero there.

    python examples/hawkes_sigma_gamma_sets.py [--paths 100000] [--seed 7]
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
    params = sv.HawkesJDParams()
    model = params.to_dict()
    model.pop("risk_premia_gamma")
    model.pop("sigma")

    # ---- 1. the surface of one put: one month, K = 0.9 F ------------------------------------------------------------------------------
    ttms, forwards = np.array([1.0 / 12.0]), np.array([1.0])
    strikes, types = [np.array([0.9])], [np.array(["P"])]
    sigmas, gammas = np.linspace(0.2, 0.8, 7), np.linspace(-3.0, 3.0, 7)
    rows = sv.hawkesjd_jump_rows(ttms, nb_path=a.paths, seed=a.seed, **model)          # the ONLY stepping launch of this section
    grid_s, grid_g = np.meshgrid(sigmas, gammas, indexing="ij")
    prices, stderrs = rows.price_sets(grid_s.ravel(), grid_g.ravel(), forwards, strikes, types)      # 49 sets: four calls of up to 16
    surface = np.array([p[0][0] for p in prices]).reshape(grid_s.shape)
    worst = max(e[0][0] for e in stderrs)
    print(f"put K = 0.9 F, one month, {a.paths} paths, undiscounted; largest standard error {worst:.1e}")
    print("  sigma \\ gamma " + " ".join(f"{g:+9.2f}" for g in gammas))
    for i, s in enumerate(sigmas):
        print(f"  {s:13.2f} " + " ".join(f"{v:9.6f}" for v in surface[i]))
    rows.free()

    # ---- 2. a calibration on the same idea ------------------------------------------------------------------------------------------
    ttms = np.array([1.0 / 52.0, 1.0 / 12.0])
    k = [np.array([0.9, 0.95, 1.0, 1.05, 1.1]), np.array([0.8, 0.9, 1.0, 1.1, 1.2])]
    t = [np.where(x <= 1.0, "P", "C") for x in k]
    true = (0.4, -2.0)
    mc = dict(nb_path=a.paths, seed=a.seed)
    pricer = sv.HawkesJDPricer()
    blank = sv.OptionChain(ttms=ttms, forwards=np.ones(2), discfactors=np.ones(2), strikes_ttms=k, optiontypes_ttms=t,
                           bid_ivs=[np.full(5, 0.5)] * 2, ask_ivs=[np.full(5, 0.5)] * 2, ids=np.array(["1w", "1m"]))
    p, _, fw = pricer.model_mc_price_chain_conditional_sets(blank, params, [true[0]], [true[1]], return_forwards=True, **mc)
    vols = blank.compute_model_ivols_from_chain_data(model_prices=p[0], forwards=fw[0][1])          # against the gamma forwards
    market = sv.OptionChain(ttms=ttms, forwards=np.ones(2), discfactors=np.ones(2), strikes_ttms=k, optiontypes_ttms=t,
                            bid_ivs=[v.copy() for v in vols], ask_ivs=[v.copy() for v in vols], ids=np.array(["1w", "1m"]))
    start = sv.HawkesJDParams(sigma=0.6, risk_premia_gamma=1.0)
    fit = pricer.calibrate_risk_premia_gamma_to_chain(market, start, estimator="conditional", print_iter=False, disp=False, **mc)
    last = pricer.last_calibration
    print(f"\ncalibration with estimator='conditional': market at (sigma, gamma) = {true}, start (0.6, 1.0)")
    print(f"  fit ({fit.sigma:.6f}, {fit.risk_premia_gamma:.6f}), objective {last['objective']:.3e}, {last['nit']} iterates, "
          f"{last['n_eval']} evaluations, {last['n_stepping_calls']} stepping call")
    print("  (the optimizer's options are the reference's: its forward-difference step 0.025 bounds how close SLSQP gets)")


if __name__ == "__main__":
    main()
