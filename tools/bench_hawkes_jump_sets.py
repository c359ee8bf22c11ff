#!/usr/bin/env python
"""
Measurement of the many-sets estimator on one set of jump rows (libsvmc_est.so's jump_sets_payoff_kernel on the
rows of hawkes_chain_cond_kernel at sigma = 0) against what a user has without it -- one
hawkesjd_mc_chain_pricer_conditional_with_risk_premia call per (sigma, gamma) -- on the BTC test chain of profiles/hawkes_bench.json
(4 expiries, 49 options, 780 steps at 1800 per year; tests/golden/hawkes_analytic.npz), default HawkesJDParams, at 10^5 and 2^20
paths.  Medians of --reps (10) calls after 3 warm-up calls, the host clock around a call that returns synchronised.  Writes ONE JSON
object to --out (default profiles/hawkes_jump_sets_bench.json) and prints it:

  mc[n].stepping_ms              hawkesjd_jump_rows: the stepping launch, the copy into the handle's buffer, a synchronise
  mc[n].sets[Q].price_sets_ms    ONE HawkesJumpRows.price_sets of Q = 1, 3, 16 sets (sigma in [0.3, 0.6], gamma in [-2, 2])
  mc[n].sets[Q].existing_calls_ms   Q calls of hawkesjd_mc_chain_pricer_conditional_with_risk_premia, each with its stepping
  mc[n].sets[Q].existing_tails_ms   Q calls of engine.tilted_conditional_payoffs at one gamma on resident rows: the existing tails WITHOUT
                                 their stepping
  mc[n].sets[Q].vs_calls, vs_tails   price_sets_ms over each
  calibration                    a 100-iterate calibrate_risk_premia_gamma_to_chain on the quoted chain of
                                 tests/golden/hawkes_risk_premia.npz (4 expiries, its mid vols) from (0.45, -1) in the two modes
                                 (estimator="fourier" | "conditional" at 10^5 paths): seconds, evaluations, the fitted (sigma, gamma),
                                 the final objective -- reported, not asserted
  layouts[KT,ST][n][Q]           the tail alone (engine.jump_sets_payoffs on resident rows) with SVMC_JS_KT strikes per group, a block
                                 per set (ST = 1), each build loaded by a process of its own through SVMC_EST_LIB, with the payoff
                                 kernel's metadata (VGPRs; waves per SIMD = 512 // VGPRs, at most 8).  --layout-lib KT,ST=FILE takes a
                                 prebuilt library -- of any build: the committed file's ST > 1 rows were measured with a tile of sets
                                 per block that is not kept; without any, the widths of LAYOUTS are compiled into a temporary directory.

    python tools/bench_hawkes_jump_sets.py [--reps 10] [--layout-lib 8,1=FILE ...] [--no-layouts] [--no-calibration] [--out FILE]
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
SET_COUNTS = (1, 3, 16)
LAYOUTS = (8, 4, 2)                                        # SVMC_JS_KT


def chain_and_params():
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    f = np.load(os.path.join(ROOT, "tests", "golden", "hawkes_analytic.npz"))
    m = f["ttms"].size
    chain = dict(ttms=f["ttms"], forwards=f["forwards"], discfactors=f["discfactors"], strikes_ttms=[f[f"strikes_{i}"] for i in range(m)],
                 optiontypes_ttms=[f[f"types_{i}"] for i in range(m)])
    p = hp.HawkesJDParams()
    return chain, {k: getattr(p, k) for k in hp.PARAM_NAMES}, f


def sets_of(q):
    return np.linspace(0.3, 0.6, q) if q > 1 else np.array([0.45]), np.linspace(-2.0, 2.0, q) if q > 1 else np.array([-1.0])


def median_ms(call, reps):
    for _ in range(3):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(wall))


def payoff_metadata(md):
    return {k: dict(v, waves_per_simd=min(8, 512 // max(int(v["vgpr"]), 1))) for k, v in md.items() if "jump_sets_" in k}


def tail_times(reps):
    """the tail alone on resident rows, per path count and set count: what a layout changes"""
    from stochvolmodels_amd.engine import tilted_type_codes
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    chain, kw, _ = chain_and_params()
    model = {k: v for k, v in kw.items() if k != "sigma"}
    codes = [tilted_type_codes(t) for t in chain["optiontypes_ttms"]]
    out = {}
    for n in SIZES:
        rows = hp.hawkesjd_jump_rows(chain["ttms"], nb_path=n, seed=2025, **model)
        out[str(n)] = {}
        for q in SET_COUNTS:
            s, g = sets_of(q)
            var = np.array([rows.variances(x) for x in s])
            out[str(n)][str(q)] = median_ms(lambda: rows.engine.jump_sets_payoffs(chain["forwards"], chain["strikes_ttms"], codes, var, g, False,
                                                                                  a_ptrs=rows.row_ptrs()), reps)
        rows.free()
    return out


def layout_comparison(libs, reps):
    from stochvolmodels_amd import build as svbuild
    out = {}
    with tempfile.TemporaryDirectory(prefix="svmc_js_layouts_") as tmp:
        if not libs:
            for kt in LAYOUTS:
                lib = os.path.join(tmp, f"libsvmc_est_k{kt}.so")
                svbuild.build_side(lib, lib + ".isa.json", svbuild.EST_SRC, False, extra=(f"-DSVMC_JS_KT={kt}",))
                libs.append((f"{kt},1", lib))
        for label, lib in libs:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--tail-only", "--reps", str(reps)],
                                 env=dict(os.environ, SVMC_EST_LIB=os.path.abspath(lib)), capture_output=True, text=True, timeout=300)
            if res.returncode != 0:
                raise RuntimeError(f"{label}: {res.stdout}{res.stderr}")
            out[label] = {"tail_ms": json.loads(res.stdout.strip().splitlines()[-1])}
            if os.path.exists(lib + ".isa.json"):
                md = json.load(open(lib + ".isa.json"))["metadata"]
                out[label]["payoff_kernel"] = {k: v for k, v in payoff_metadata(md).items() if "payoff" in k}
    return out


def calibration(f, n, seed):
    """the 100-iterate fit of (sigma, gamma) to the chain's own mid vols in the two modes"""
    import stochvolmodels_amd as sv
    f = np.load(os.path.join(ROOT, "tests", "golden", "hawkes_risk_premia.npz"))        # the quoted chain of the Fourier calibration's tests
    m = f["ttms"].size
    chain = sv.OptionChain(ttms=f["ttms"], forwards=f["forwards"], discfactors=f["discfactors"], strikes_ttms=[f[f"strikes_{i}"] for i in range(m)],
                           optiontypes_ttms=[f[f"types_{i}"] for i in range(m)], bid_ivs=[f[f"bid_{i}"] for i in range(m)],
                           ask_ivs=[f[f"ask_{i}"] for i in range(m)], ids=None)
    pricer, out = sv.HawkesJDPricer(), {}
    for mode, extra in (("fourier", {}), ("conditional", dict(estimator="conditional", nb_path=n, seed=seed))):
        params0 = sv.HawkesJDParams(risk_premia_gamma=-1.0)
        t0 = time.perf_counter()
        fit = pricer.calibrate_risk_premia_gamma_to_chain(chain, params0, maxiter=100, print_iter=False, disp=False, **extra)
        last = pricer.last_calibration
        out[mode] = dict(seconds=time.perf_counter() - t0, sigma=float(fit.sigma), gamma=float(fit.risk_premia_gamma),
                         objective=float(last["objective"]), nit=last["nit"], n_eval=last["n_eval"], status=last["status"],
                         n_gradient_batches=last["n_gradient_batches"], n_stepping_calls=last.get("n_stepping_calls"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--layout-lib", action="append", default=[], help="KT,ST=FILE: a prebuilt libsvmc_est.so")
    ap.add_argument("--no-layouts", action="store_true")
    ap.add_argument("--no-calibration", action="store_true")
    ap.add_argument("--tail-only", action="store_true", help="print the tail's times of the loaded library and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hawkes_jump_sets_bench.json"))
    a = ap.parse_args()
    if a.tail_only:
        print(json.dumps(tail_times(a.reps)))
        return
    from stochvolmodels_amd import build as svbuild
    from stochvolmodels_amd.engine import get_engine, tilted_type_codes
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    chain, kw, f = chain_and_params()
    model = {k: v for k, v in kw.items() if k != "sigma"}
    m = chain["ttms"].size
    codes = [tilted_type_codes(t) for t in chain["optiontypes_ttms"]]
    out = {"chain": "BTC test chain, 4 expiries, 49 options", "steps": 780, "steps_per_year": 1800, "reps": a.reps, "seed": a.seed,
           "kernel_metadata": payoff_metadata(json.load(open(svbuild.EST_ISA_JSON))["metadata"]), "mc": {}}
    for n in SIZES:
        eng = get_engine(n)
        row = {"sets": {}}

        def step():
            hp.hawkesjd_jump_rows(chain["ttms"], nb_path=n, **model).free()
        row["stepping_ms"] = median_ms(step, a.reps)
        rows = hp.hawkesjd_jump_rows(chain["ttms"], nb_path=n, seed=a.seed, **model)
        for q in SET_COUNTS:
            s, g = sets_of(q)
            r = {}
            r["price_sets_ms"] = median_ms(lambda: rows.price_sets(s, g, chain["forwards"], chain["strikes_ttms"], chain["optiontypes_ttms"]), a.reps)

            def existing_calls():
                for sigma, gamma in zip(s, g):
                    hp.hawkesjd_mc_chain_pricer_conditional_with_risk_premia(risk_premia_gamma=float(gamma), nb_path=n, **chain,
                                                                             **dict(kw, sigma=float(sigma)))
            r["existing_calls_ms"] = median_ms(existing_calls, a.reps)
            # the existing tail on the rows its own stepping left in the engine's snapshots (mu in [0, m), cv in [m, 2m))
            hp.hawkesjd_mc_chain_pricer_conditional_with_risk_premia(risk_premia_gamma=-1.0, nb_path=n, seed=a.seed, **chain, **kw)

            def existing_tails():
                for gamma in g:
                    eng.tilted_conditional_payoffs(chain["forwards"], chain["strikes_ttms"], codes, [float(gamma)], False,
                                                   mu_rows=list(range(m)), cv_rows=list(range(m, 2 * m)))
            r["existing_tails_ms"] = median_ms(existing_tails, a.reps)
            r["vs_calls"] = r["price_sets_ms"] / r["existing_calls_ms"]
            r["vs_tails"] = r["price_sets_ms"] / r["existing_tails_ms"]
            row["sets"][str(q)] = r
        rows.free()
        out["mc"][str(n)] = row
    if not a.no_calibration:
        out["calibration"] = calibration(f, SIZES[0], a.seed)
    if not a.no_layouts:
        out["layouts"] = layout_comparison([tuple(s.split("=", 1)) for s in a.layout_lib], a.reps)
    text = json.dumps(out)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
