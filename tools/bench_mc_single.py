"""
Warm wall time of ONE call of the three single Monte Carlo chain pricers on one GPU (logsv_mc_chain_pricer, heston_mc_chain_pricer,
hawkesjd_mc_chain_pricer): the 4 x 13 chain of tools/bench_mc_many.py at 360 steps per year, nb_path in {2^16, 10^5}.  These calls
are latency-bound (about 0.1 ms at 2^16 paths for LogSV), so the figure moves with the interpreter time of the Python dispatch in
front of the fused C driver: the tool for an A/B of a change to that dispatch (profiles/mc_host_driver_ab.txt).

Per case: warm-up calls, then the median of --reps timed calls (10, as the sibling tools), and the median of --long-reps calls
(200), which is the steadier figure.

    python tools/bench_mc_single.py [--out FILE.json] [--reps 10] [--long-reps 200]        # rows on stdout; --out also writes them
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import stochvolmodels_amd as sv                                        # noqa: E402
from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp          # noqa: E402

SPY = 360


def chain_4x13():
    ttms = np.array([1 / 12, 0.25, 0.5, 1.0])
    k = np.linspace(0.7, 1.3, 13)
    return dict(ttms=ttms, forwards=np.ones(4), discfactors=np.ones(4), strikes_ttms=[k.copy() for _ in ttms],
                optiontypes_ttms=[np.asarray(np.where(k < 1.0, "P", "C")) for _ in ttms])


def pricers(ch, nb_path):
    lp, he, hk = sv.LOGSV_BTC_PARAMS, sv.HestonParams(), hp.HawkesJDParams().to_dict()
    hk.pop("risk_premia_gamma")
    return {
        "logsv": lambda: sv.logsv_mc_chain_pricer(v0=lp.sigma0, theta=lp.theta, kappa1=lp.kappa1, kappa2=lp.kappa2, beta=lp.beta,
                                                  volvol=lp.volvol, vol_backbone_etas=np.ones(4), nb_path=nb_path,
                                                  nb_steps_per_year=SPY, seed=7, **ch),
        "heston": lambda: sv.heston_mc_chain_pricer(v0=he.v0, theta=he.theta, kappa=he.kappa, rho=he.rho, volvol=he.volvol,
                                                    nb_path=nb_path, nb_steps_per_year=SPY, seed=7, **ch),
        "hawkesjd": lambda: hp.hawkesjd_mc_chain_pricer(nb_path=nb_path, nb_steps_per_year=SPY, seed=7, **ch, **hk),
    }


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--long-reps", type=int, default=200)
    a = ap.parse_args()
    ch = chain_4x13()
    rows = []
    for nb_path in (1 << 16, 100_000):
        for model, fn in pricers(ch, nb_path).items():
            for _ in range(5):
                fn()
            row = {"model": model, "nb_path": nb_path, "call_ms": round(median_ms(fn, a.reps), 4),
                   "call_ms_long": round(median_ms(fn, a.long_reps), 4), "reps": a.reps, "long_reps": a.long_reps}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out is None:
        return
    with open(a.out, "w") as fh:
        json.dump({"what": "one warm call of the single MC chain pricers (tools/bench_mc_single.py)",
                   "chain": "4 x 13 (ttms 1/12, 1/4, 1/2, 1; strikes 0.7-1.3), 360 steps/yr", "rows": rows}, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
