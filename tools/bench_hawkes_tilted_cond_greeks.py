#!/usr/bin/env python
"""
Measurement of the conditional Monte Carlo Greeks under the risk-premia kernel (libsvmc_est.so's
tilted_cond_greeks_kernel on the rows of hawkes_chain_cond_kernel) on the BTC test chain of profiles/hawkes_tilted_cond_bench.json
(4 expiries, 49 options, 780 steps at 1800 per year; tests/golden/hawkes_analytic.npz), default HawkesJDParams, at 10^5 and 2^20
paths, with 1 gamma (-1) and 5 gammas (-3, -1, 0, 0.5, 3).  Medians of --reps (10) calls after 3 warm-up calls, the host clock around
a call that returns synchronised.  The pricing calls are the parent commit's code, untouched: their times are measured here, in the
same process.  Writes ONE JSON object to --out (default profiles/hawkes_tilted_cond_greeks_bench.json) and prints it:

  mc[n][G].greeks_call_ms        hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas: one stepping call, the two tails
  mc[n][G].greeks_tail_ms, payoff_tail_ms   tilted_conditional_greeks and tilted_conditional_payoffs alone on resident rows
  mc[n][G].pricing_call_ms, three_pricing_calls_ms   hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas once, and at F,
                F + h, F - h: the parent commit's alternative, a central difference in F that returns no error and no gamma
  mc[n][G].vs_three_calls, vs_one_call, tail_vs_payoff_tail   the ratios
  kt[KT][n][G]                   the Greeks tail with SVMC_TCG_KT strikes per group, each build in a process of its own (--kt-lib KT=FILE
                takes a prebuilt library; without it the variant is compiled into a temporary directory), with its kernel metadata
  density[n]                     a 200-point density for 5 gammas: get_log_return_mc_pdf_conditional_under_risk_kernel against
                get_log_return_mc_pdf_device(risk_premia_gamma=), one month
  plain_fd_delta[gamma]          per quote, the variance over --fd-seeds (32) seeds of the plain estimator's central-difference delta
                under the kernel (three hawkesjd_mc_chain_pricer_with_risk_premia_gammas calls on common random numbers, h = 1e-2 F)
                over the mean squared reported error of this delta, at 10^5 paths: min, median, max

    python tools/bench_hawkes_tilted_cond_greeks.py [--reps 10] [--seed 2025] [--kt-lib 8=FILE] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (100000, 1 << 20)
GAMMA_SETS = ([-1.0], [-3.0, -1.0, 0.0, 0.5, 3.0])
KTS = (2, 4, 8)


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


def tail_times(reps):
    """{n: {G: ms}} of the Greeks tail alone, on the rows one conditional pricing call leaves, with the library _lib.load_est() finds"""
    from stochvolmodels_amd.engine import get_engine, tilted_type_codes
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    chain, kw = chain_and_params()
    m = chain["ttms"].size
    codes = [tilted_type_codes(t) for t in chain["optiontypes_ttms"]]
    out = {}
    for n in SIZES:
        eng = get_engine(n)
        hp.hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas(risk_premia_gammas=[0.0], nb_path=n, seed=1, **chain, **kw)
        out[str(n)] = {str(len(g)): median_ms(lambda: eng.tilted_conditional_greeks(
            chain["forwards"], chain["strikes_ttms"], codes, g, False, mu_rows=list(range(m)), cv_rows=list(range(m, 2 * m))), reps)
            for g in GAMMA_SETS}
    return out


def kt_comparison(kt_libs, reps):
    """the Greeks tail at each SVMC_TCG_KT, every build loaded by a fresh process through SVMC_EST_LIB"""
    from stochvolmodels_amd import build as svbuild
    out = {}
    with tempfile.TemporaryDirectory(prefix="svmc_tcg_kt_") as tmp:
        for kt in KTS:
            lib = kt_libs.get(kt)
            if lib is None:
                lib = os.path.join(tmp, f"libsvmc_est_kt{kt}.so")
                svbuild.build_side(lib, lib + ".isa.json", svbuild.EST_SRC, False, extra=(f"-DSVMC_TCG_KT={kt}",))
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--tail-only", "--reps", str(reps)],
                                 env=dict(os.environ, SVMC_EST_LIB=os.path.abspath(lib)), capture_output=True, text=True, timeout=300)
            if res.returncode != 0:
                raise RuntimeError(f"KT={kt}: {res.stdout}{res.stderr}")
            out[str(kt)] = json.loads(res.stdout.strip().splitlines()[-1])
            if os.path.exists(lib + ".isa.json"):
                meta = json.load(open(lib + ".isa.json"))["metadata"]
                out[str(kt)]["kernel"] = next(v for k, v in meta.items() if "tilted_cond_greeks_kernelI" in k)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--fd-seeds", type=int, default=32)
    ap.add_argument("--kt-lib", action="append", default=[], help="KT=FILE: a prebuilt libsvmc_est.so with -DSVMC_TCG_KT=KT")
    ap.add_argument("--tail-only", action="store_true", help="print the Greeks tail's times of the loaded library and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hawkes_tilted_cond_greeks_bench.json"))
    a = ap.parse_args()
    if a.tail_only:
        print(json.dumps(tail_times(a.reps)))
        return
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import build as svbuild
    from stochvolmodels_amd.engine import get_engine, tilted_type_codes
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    chain, kw = chain_and_params()
    m = chain["ttms"].size
    codes = [tilted_type_codes(t) for t in chain["optiontypes_ttms"]]
    rows = dict(mu_rows=list(range(m)), cv_rows=list(range(m, 2 * m)))
    h_rel = 1e-2
    bumped = [dict(chain, forwards=chain["forwards"] * s) for s in (1.0, 1.0 + h_rel, 1.0 - h_rel)]
    out = {"chain": "BTC test chain, 4 expiries, 49 options", "steps": 780, "steps_per_year": 1800, "reps": a.reps, "seed": a.seed,
           "kernel_metadata": json.load(open(svbuild.EST_ISA_JSON))["metadata"], "mc": {}}
    for n in SIZES:
        eng = get_engine(n)
        out["mc"][str(n)] = {}
        for gammas in GAMMA_SETS:
            common = dict(risk_premia_gammas=gammas, nb_path=n, **kw)
            price = hp.hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas
            row = {"greeks_call_ms": median_ms(lambda: hp.hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas(**common, **chain), a.reps),
                   "pricing_call_ms": median_ms(lambda: price(**common, **chain), a.reps),
                   "three_pricing_calls_ms": median_ms(lambda: [price(seed=a.seed, **common, **c) for c in bumped], a.reps)}
            row["greeks_tail_ms"] = median_ms(lambda: eng.tilted_conditional_greeks(chain["forwards"], chain["strikes_ttms"], codes, gammas, False,
                                                                                    **rows), a.reps)
            row["payoff_tail_ms"] = median_ms(lambda: eng.tilted_conditional_payoffs(chain["forwards"], chain["strikes_ttms"], codes, gammas, False,
                                                                                     **rows), a.reps)
            row["vs_three_calls"] = row["greeks_call_ms"] / row["three_pricing_calls_ms"]
            row["vs_one_call"] = row["greeks_call_ms"] / row["pricing_call_ms"]
            row["tail_vs_payoff_tail"] = row["greeks_tail_ms"] / row["payoff_tail_ms"]
            out["mc"][str(n)][str(len(gammas))] = row
    out["kt"] = kt_comparison({int(s.split("=")[0]): s.split("=", 1)[1] for s in a.kt_lib}, a.reps)
    # the density: 200 points, 5 gammas, one month
    pricer, params, x, g5 = sv.HawkesJDPricer(), hp.HawkesJDParams(), np.linspace(-0.6, 0.6, 200), GAMMA_SETS[1]
    out["density"] = {}
    for n in SIZES:
        cond = median_ms(lambda: pricer.get_log_return_mc_pdf_conditional_under_risk_kernel(params, 1.0 / 12.0, x, g5, nb_path=n), a.reps)
        kde = median_ms(lambda: pricer.get_log_return_mc_pdf_device(1.0 / 12.0, params, x, nb_path=n, risk_premia_gamma=g5), a.reps)
        out["density"][str(n)] = {"conditional_ms": cond, "weighted_kde_ms": kde, "ratio": cond / kde}
    # the plain estimator's finite-difference delta under the kernel against this delta, per quote, at 10^5 paths
    n, g5 = SIZES[0], GAMMA_SETS[1]
    fd, err2 = [], []
    for s in range(a.fd_seeds):
        common = dict(risk_premia_gammas=g5, nb_path=n, seed=a.seed + s, **kw)
        p0, up, dn = (hp.hawkesjd_mc_chain_pricer_with_risk_premia_gammas(**common, **c)[0] for c in bumped)
        fd.append([np.concatenate([(u - d) / (2.0 * h_rel * f) for u, d, f in zip(up[g], dn[g], chain["forwards"])]) for g in range(len(g5))])
        gk = hp.hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas(**common, **chain)
        err2.append([np.concatenate(gk[g]["delta_stderr"]) ** 2 for g in range(len(g5))])
    fd, err2 = np.array(fd), np.array(err2)
    out["plain_fd_delta"] = {"paths": n, "seeds": a.fd_seeds, "relative_step": h_rel}
    for g, gamma in enumerate(g5):
        ratio = fd[:, g].var(axis=0, ddof=1) / err2[:, g].mean(axis=0)
        out["plain_fd_delta"][str(gamma)] = {"min": float(ratio.min()), "median": float(np.median(ratio)), "max": float(ratio.max()),
                                             "per_quote": [round(float(v), 2) for v in ratio]}
    text = json.dumps(out)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
