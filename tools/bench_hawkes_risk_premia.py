#!/usr/bin/env python
"""
Measurement of the Hawkes risk-premia kernel on the reference's BTC test chain (4 expiries, 49 quotes, forward-normalised
strikes; tests/golden/hawkes_risk_premia.npz), params0 = HawkesJDParams() with lambda_p = 50, lambda_m = 5 and gamma = 0, as
in the reference's papers/jump_risk_premia_clustered_jumps/calibrate_chain.py.  Writes profiles/hawkes_risk_premia_bench.json
and prints it as ONE JSON line:

  pricing_ms        one hawkesjd_chain_pricer_with_risk_premia (one forwards launch, an advance and an inversion launch per
                    expiry, one download), median, at gamma = 1
  forwards_ms       hawkesjd_forwards_under_risk_kernel alone on the chain's 4 expiries (one launch, its buffers and the
                    download), median
  objective_ms      one objective evaluation (the pricing + the host Black inversion against the gamma forwards), median
  gradient_batch_ms one 3-set batch (the base point and the 2 bumped vectors of SLSQP's forward difference at eps 0.025)
                    through hawkesjd_chain_pricer_with_risk_premia_batch, median; gradient_3_single_ms the same 3 points
                    one call at a time
  calibration       calibrate_risk_premia_gamma_to_chain at the reference's maxiter=100, is_vega_weighted=False: wall time,
                    objective evaluations, gradient batches, exit status, fit -- batched gradient (the default) and SLSQP's own
                    differencing (batched_gradient=False)
  reference_cpu     the unmodified reference's runs from the fixture, timed on one CPU core when the fixture was made: a CPU
                    figure of the reference, not of this library

    python tools/bench_hawkes_risk_premia.py [--reps 20]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
    from stochvolmodels_amd.data.option_chain import OptionChain
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    import hawkes_twin as twin

    f = np.load(os.path.join(ROOT, "tests", "golden", "hawkes_risk_premia.npz"))
    m = f["ttms"].size
    chain = OptionChain(ttms=f["ttms"], forwards=f["forwards"], discfactors=f["discfactors"],
                        strikes_ttms=[f[f"strikes_{i}"] for i in range(m)], optiontypes_ttms=[f[f"types_{i}"] for i in range(m)],
                        bid_ivs=[f[f"bid_{i}"] for i in range(m)], ask_ivs=[f[f"ask_{i}"] for i in range(m)], ids=None)

    def params0():
        p = hp.HawkesJDParams(**dict(zip(twin.PARAM_NAMES, (float(v) for v in f["calib_params0"]))))
        p.risk_premia_gamma = 0.0
        return p
    pricer = hp.HawkesJDPricer()
    kw = dict(ttms=chain.ttms, forwards=chain.forwards, discfactors=chain.discfactors, strikes_ttms=chain.strikes_ttms,
              optiontypes_ttms=chain.optiontypes_ttms)
    p1 = params0()
    p1.risk_premia_gamma = 1.0
    out = {"chain": "BTC test chain, 4 expiries, 49 options, forward-normalised", "reps": reps}
    out["pricing_ms"] = median_ms(lambda: hp.hawkesjd_chain_pricer_with_risk_premia(model_params=p1, **kw), reps)
    out["forwards_ms"] = median_ms(lambda: hp.hawkesjd_forwards_under_risk_kernel(p1, 1.0, chain.ttms, chain.forwards), reps)
    objective = pricer.risk_premia_calibration_objective(chain, params0(), is_vega_weighted=False, print_iter=False)
    x0 = np.array([0.45, 1.0 / 8.0])
    out["objective_ms"] = median_ms(lambda: objective(x0), reps)
    h = objective.fd_steps(x0)
    points = [x0] + [x0 + np.eye(2)[i] * h[i] for i in range(2)]
    sets = []
    for x in points:
        p = params0()
        sets.append(hp.unpack_risk_premia_vector(x, p))
    out["n_sets"] = len(sets)
    out["gradient_batch_ms"] = median_ms(lambda: hp.hawkesjd_chain_pricer_with_risk_premia_batch(params_list=sets, **kw), reps)
    out["gradient_3_single_ms"] = median_ms(
        lambda: [hp.hawkesjd_chain_pricer_with_risk_premia(model_params=p, **kw) for p in sets], reps)

    out["calibration"] = {}
    for tag, batched in (("batched_gradient", True), ("plain", False)):
        pricer.calibrate_risk_premia_gamma_to_chain(chain, params0(), is_vega_weighted=False, print_iter=False, disp=False,
                                                    batched_gradient=batched)                                     # warm
        t0 = time.perf_counter()
        fit = pricer.calibrate_risk_premia_gamma_to_chain(chain, params0(), is_vega_weighted=False, print_iter=False,
                                                          disp=False, batched_gradient=batched)
        wall = time.perf_counter() - t0
        info = pricer.last_calibration
        out["calibration"][tag] = {"wall_s": wall, "n_eval": info["n_eval"], "n_gradient_batches": info["n_gradient_batches"],
                                   "nit": info["nit"], "status": info["status"], "objective": info["objective"],
                                   "fit": {"sigma": float(fit.sigma), "risk_premia_gamma": float(fit.risk_premia_gamma)}}
    out["reference_cpu"] = {tag: {"wall_s": float(f[f"cal_{tag}_wall_s"]), "nfev": int(f[f"cal_{tag}_nfev"]),
                                  "nit": int(f[f"cal_{tag}_nit"]), "status": int(f[f"cal_{tag}_status"]),
                                  "maxiter": int(f[f"cal_{tag}_maxiter"]), "objective": float(f[f"cal_{tag}_fun"])}
                            for tag in ("default_chain", "default_slice", "tight_chain", "tight_slice")
                            if f"cal_{tag}_x" in f.files}
    out["reference_cpu"]["pricing_s"] = {"default": float(f["prices_default_1_wall_s"]), "tight": float(f["prices_tight_1_wall_s"])}
    out["reference_cpu"]["label"] = "unmodified reference, one CPU core of the build container, at fixture generation"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "hawkes_risk_premia_bench.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
