#!/usr/bin/env python
"""
Measurement of the Hawkes calibration (HawkesJDPricer.calibrate_model_params_to_chain) on the reference's BTC test chain
(4 expiries, 49 quotes, forward-normalised strikes; tests/golden/hawkes_calibration.npz), params0 = HawkesJDParams().  Writes
profiles/hawkes_calibration_bench.json and prints it as ONE JSON line:

  objective_ms      one objective evaluation (one Fourier chain pricing on the device + the host Black inversion), median
  pricing_ms        hawkesjd_chain_pricer alone at the start vector, median
  gradient_batch_ms one 9-set batch (the base point and 8 bumped vectors of SLSQP's forward difference) through
                    hawkesjd_chain_pricer_batch, median; gradient_ms the whole ImpliedVolObjective.gradient call
  gradient_9_single_ms  the same 9 points priced one call at a time, median
  calibration       wall time, objective evaluations, gradient batches, final objective: batched gradient (the default)
                    and SLSQP's own differencing (batched_gradient=False)
  reference_cpu     the unmodified reference's full calibrations from the fixture (SciPy default and tightened solve_ivp),
                    timed on one CPU core when the fixture was made: a CPU figure of the reference, not of this library

    python tools/bench_hawkes_calibration.py [--reps 20]
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

    f = np.load(os.path.join(ROOT, "tests", "golden", "hawkes_calibration.npz"))
    m = f["ttms"].size
    chain = OptionChain(ttms=f["ttms"], forwards=f["forwards"], discfactors=f["discfactors"],
                        strikes_ttms=[f[f"strikes_{i}"] for i in range(m)], optiontypes_ttms=[f[f"types_{i}"] for i in range(m)],
                        bid_ivs=[f[f"bid_{i}"] for i in range(m)], ask_ivs=[f[f"ask_{i}"] for i in range(m)], ids=None)
    params0 = hp.HawkesJDParams(**dict(zip(twin.PARAM_NAMES, (float(v) for v in f["params0"]))))
    pricer = hp.HawkesJDPricer()
    objective = pricer.calibration_objective(chain, params0)
    x0 = hp.calibration_start_vector(params0)
    h = objective.fd_steps(x0)
    points = [x0 + np.eye(x0.size)[i] * h[i] for i in range(x0.size)] + [x0]
    sets = [hp.unpack_calibration_vector(p, params0) for p in points]
    kw = dict(ttms=chain.ttms, forwards=chain.forwards, discfactors=chain.discfactors, strikes_ttms=chain.strikes_ttms,
              optiontypes_ttms=chain.optiontypes_ttms)
    out = {"chain": "BTC test chain, 4 expiries, 49 options, forward-normalised", "reps": reps, "n_sets": len(points)}
    out["objective_ms"] = median_ms(lambda: objective(x0), reps)
    out["pricing_ms"] = median_ms(lambda: hp.hawkesjd_chain_pricer(model_params=sets[-1], **kw), reps)
    out["gradient_batch_ms"] = median_ms(lambda: hp.hawkesjd_chain_pricer_batch(params_list=sets, **kw), reps)

    def gradient():
        objective._last = (None, None)                       # price the base point inside the batch, as at a fresh iterate
        objective.gradient(x0)
    out["gradient_ms"] = median_ms(gradient, reps)
    out["gradient_9_single_ms"] = median_ms(lambda: [hp.hawkesjd_chain_pricer(model_params=p, **kw) for p in sets], reps)

    out["calibration"] = {}
    for tag, batched in (("batched_gradient", True), ("plain", False)):
        pricer.calibrate_model_params_to_chain(chain, params0, disp=False, batched_gradient=batched)       # warm
        t0 = time.perf_counter()
        fit = pricer.calibrate_model_params_to_chain(chain, params0, disp=False, batched_gradient=batched)
        wall = time.perf_counter() - t0
        info = pricer.last_calibration
        out["calibration"][tag] = {"wall_s": wall, "n_eval": info["n_eval"], "n_gradient_batches": info["n_gradient_batches"],
                                   "objective": info["objective"], "success": info["success"],
                                   "fit": {k: float(getattr(fit, k)) for k in ("sigma", "mean_p", "mean_m", "theta_p",
                                                                               "theta_m", "kappa_p", "beta1_p", "beta1_m")}}
    out["reference_cpu"] = {tag: {"wall_s": float(f[f"{tag}_wall_s"]), "nfev": int(f[f"{tag}_nfev"]), "nit": int(f[f"{tag}_nit"]),
                                  "objective": float(f[f"{tag}_fun"])} for tag in ("default", "tight")}
    out["reference_cpu"]["label"] = "unmodified reference, one CPU core of the build container, at fixture generation"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "hawkes_calibration_bench.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
