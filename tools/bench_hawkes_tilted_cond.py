#!/usr/bin/env python
"""
Measurement of conditional Monte Carlo under the risk-premia kernel (libsvmc_ext.so's tilted_cond_payoff_kernel on
the rows of hawkes_chain_cond_kernel) against row f8's plain estimator under the kernel, on the BTC test chain of
profiles/hawkes_bench.json (4 expiries, 49 options, 780 steps at 1800 per year; tests/golden/hawkes_analytic.npz), default
HawkesJDParams, at 10^5 and 2^20 paths, with 1 gamma (-1) and 5 gammas (-3, -1, 0, 0.5, 3).  Medians of --reps (10) calls after 3
warm-up calls, the host clock around a call that returns synchronised.  Row f8's code is the parent commit's, untouched: its times are
measured here, in the same process.  Writes ONE JSON object to --out (default profiles/hawkes_tilted_cond_bench.json) and prints it:

  mc[n][G].conditional / plain   whole-call ms of hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas (two C calls) and of
                hawkesjd_mc_chain_pricer_with_risk_premia_gammas (one), and the tail alone on resident rows: tilted_conditional_payoffs
                and tilted_payoffs (each with its download and synchronise)
  mc[n][G].time_ratio, tail_ratio   conditional / plain
  mc[n][G].gamma[g]               per quote (plain error / conditional error)^2 at --seed: min, median, max; the effective sample sizes
                per expiry; cost_at_equal_error = time_ratio / error-squared ratio (above 1: the conditional call costs MORE per unit of
                error than row f8's), at the median and at the worst quote

    python tools/bench_hawkes_tilted_cond.py [--reps 10] [--seed 2025] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (100000, 1 << 20)
GAMMA_SETS = ([-1.0], [-3.0, -1.0, 0.0, 0.5, 3.0])


def chain_and_params():
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    f = np.load(os.path.join(ROOT, "tests", "golden", "hawkes_analytic.npz"))
    m = f["ttms"].size
    chain = dict(ttms=f["ttms"], forwards=f["forwards"], discfactors=f["discfactors"], strikes_ttms=[f[f"strikes_{i}"] for i in range(m)],
                 optiontypes_ttms=[f[f"types_{i}"] for i in range(m)])
    p = hp.HawkesJDParams()
    return chain, {k: getattr(p, k) for k in hp.PARAM_NAMES}


def median_ms(call, reps):
    for _ in range(3):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hawkes_tilted_cond_bench.json"))
    a = ap.parse_args()
    from stochvolmodels_amd import build as svbuild
    from stochvolmodels_amd.engine import get_engine, tilted_type_codes
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    chain, kw = chain_and_params()
    m = chain["ttms"].size
    codes = [tilted_type_codes(t) for t in chain["optiontypes_ttms"]]
    out = {"chain": "BTC test chain, 4 expiries, 49 options", "steps": 780, "steps_per_year": 1800, "reps": a.reps, "seed": a.seed,
           "kernel_metadata": json.load(open(svbuild.EXT_ISA_JSON))["metadata"], "mc": {}}
    for n in SIZES:
        eng = get_engine(n)
        out["mc"][str(n)] = {}
        for gammas in GAMMA_SETS:
            common = dict(risk_premia_gammas=gammas, nb_path=n, **chain, **kw)
            row = {"conditional": {}, "plain": {}, "gamma": {}}
            row["plain"]["call_ms"] = median_ms(lambda: hp.hawkesjd_mc_chain_pricer_with_risk_premia_gammas(**common), a.reps)
            row["conditional"]["call_ms"] = median_ms(lambda: hp.hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas(**common),
                                                      a.reps)
            # both tails on the rows the conditional call left in the engine's snapshots: row f8's reads the mu rows [0, m) as its x
            row["plain"]["tail_ms"] = median_ms(lambda: eng.tilted_payoffs(chain["forwards"], chain["strikes_ttms"], codes, gammas, False,
                                                                           snap_rows=list(range(m))), a.reps)
            row["conditional"]["tail_ms"] = median_ms(lambda: eng.tilted_conditional_payoffs(
                chain["forwards"], chain["strikes_ttms"], codes, gammas, False, mu_rows=list(range(m)), cv_rows=list(range(m, 2 * m))), a.reps)
            row["time_ratio"] = row["conditional"]["call_ms"] / row["plain"]["call_ms"]
            row["tail_ratio"] = row["conditional"]["tail_ms"] / row["plain"]["tail_ms"]
            _, ce, cf = hp.hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas(seed=a.seed, return_forwards=True, **common)
            _, pe, pf = hp.hawkesjd_mc_chain_pricer_with_risk_premia_gammas(seed=a.seed, return_forwards=True, **common)
            for g, gamma in enumerate(gammas):
                with np.errstate(all="ignore"):
                    vr = (np.concatenate(pe[g]) / np.concatenate(ce[g])) ** 2
                ok = np.isfinite(vr)
                row["gamma"][str(gamma)] = {
                    "error_squared_ratio": {"min": float(np.min(vr[ok])), "median": float(np.median(vr[ok])), "max": float(np.max(vr[ok])),
                                            "per_quote": [round(float(v), 3) if np.isfinite(v) else None for v in vr]},
                    "effective_sample_size": {"plain": [float(v) / n for v in pf[g][2][:, 4]], "conditional": [float(v) / n for v in cf[g][2][:, 4]]},
                    "cost_at_equal_error": {"median": row["time_ratio"] / float(np.median(vr[ok])), "worst_quote": row["time_ratio"] / float(np.min(vr[ok]))}}
            out["mc"][str(n)][str(len(gammas))] = row
    text = json.dumps(out)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
