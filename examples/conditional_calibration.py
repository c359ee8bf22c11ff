"""
Fit the LogSV model to one option chain with the plain and with the conditional Monte Carlo calibration engine, side by side
(DESIGN.md rows f3 and f15).

Both engines freeze one random stream and hand SLSQP the implied vols of every iterate: the plain engine from payoffs, the
conditional one from per-path Black-76 prices -- an order of magnitude less noise at equal paths, and a smooth function under the
forward differences of the gradient.  An evaluation of either is one replayed graph with the implied vols as its last kernel.  The
market vols are the model's own (the conditional estimator at --paths x 16 on another seed), so the parameters to find are known.

    python examples/conditional_calibration.py [--paths 8192] [--seed 10]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stochvolmodels_amd as sv  # noqa: E402

NAMES = ("sigma0", "theta", "kappa1", "beta", "volvol")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=8192)
    ap.add_argument("--seed", type=int, default=10)
    a = ap.parse_args()
    ttms, k = np.array([1 / 12, 0.25, 0.5, 1.0]), np.linspace(0.7, 1.3, 13)
    chain = dict(ttms=ttms, forwards=np.ones(4), discfactors=np.ones(4), strikes_ttms=[k] * 4,
                 optiontypes_ttms=[np.where(k < 1.0, "P", "C")] * 4)
    p = sv.LOGSV_BTC_PARAMS
    true = sv.LogSvParams(sigma0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=None, beta=p.beta, volvol=p.volvol)
    market = sv.logsv_mc_chain_pricer_conditional_sets([true], nb_path=16 * a.paths, seed=a.seed + 1, return_ivols=True, **chain)[0][2]
    option_chain = sv.OptionChain(ids=np.array([f"t{i}" for i in range(4)]), bid_ivs=market, ask_ivs=market, **chain)
    start = sv.LogSvParams(**{n: 1.15 * getattr(true, n) for n in NAMES}, kappa2=None)
    print(f"{'':24s}" + "".join(f"{n:>10s}" for n in NAMES) + "   objective   n_eval  seconds")
    print(f"{'true':24s}" + "".join(f"{getattr(true, n):10.4f}" for n in NAMES))
    print(f"{'start':24s}" + "".join(f"{getattr(start, n):10.4f}" for n in NAMES))
    for label, kw in (("plain, frozen stream", dict(device_randoms=True)), ("conditional", dict(estimator="conditional"))):
        pricer = sv.LogSVPricer()
        t0 = time.perf_counter()
        fit = pricer.calibrate_model_params_to_chain(option_chain, start, calibration_engine=sv.CalibrationEngine.MC, nb_path=a.paths,
                                                     nb_steps=360, seed=a.seed, disp=False, **kw)
        dt = time.perf_counter() - t0
        last = pricer.last_calibration
        print(f"{label:24s}" + "".join(f"{getattr(fit, n):10.4f}" for n in NAMES) + f"   {last['objective']:.3e}   {last['n_eval']:6d}  {dt:7.3f}")


if __name__ == "__main__":
    main()
