#!/usr/bin/env python
"""
Measurement of conditional Monte Carlo for the Hawkes jump-diffusion (csrc/svmc_hawkes.hip
hawkes_chain_cond_kernel) against the plain pricer, on the BTC test chain of profiles/hawkes_bench.json (4 expiries, 49 options, 780
steps at 1800 per year; tests/golden/hawkes_analytic.npz), default HawkesJDParams, at 10^5 and 2^20 paths.  Medians of --reps (10)
calls after 3 warm-up calls, the host clock around a call that returns synchronised; the stepping launch's time from the session's HIP
events (svmc_session_time_stepping).  Writes ONE JSON object to --out (default profiles/hawkes_cmc_bench.json) and prints it:

  mc[n].conditional / plain / greeks   whole-call ms and the stepping launch's ms of hawkesjd_mc_chain_pricer_conditional,
                hawkesjd_mc_chain_pricer and hawkesjd_mc_chain_greeks_conditional, in this one process
  mc[n].time_ratio                     conditional call ms / plain call ms;  stepping_ratio the same of the stepping launches
  mc[n].variance_ratio                 per quote (plain error / conditional error)^2 at --seed, with its median and its values at the
                quotes nearest the forward; cost_at_equal_error = time_ratio / variance ratio (below 1: the conditional call is the
                cheaper way to a given error), per quote, median and nearest the forward
  block_ab      the stepping launch at 256-thread blocks (the build) against --block-ab LIB, a library built from the same sources
                with -DSVMC_HAWKES_COND_BLOCK=512: each in a child process of its own (SVMC_LIB), medians of --reps

    python tools/bench_hawkes_cmc.py [--reps 10] [--seed 2025] [--out FILE] [--block-ab build/libsvmc_cond_block512.so]

The A/B library is built as the library is, with the one define added:
    hipcc <stochvolmodels_amd.build.flags()> -DSVMC_HAWKES_COND_BLOCK=512 stochvolmodels_amd/csrc/*.hip -o build/libsvmc_cond_block512.so
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (100000, 1 << 20)
KERNELS = {"conditional": "hawkes_chain_cond_kernel", "greeks": "hawkes_chain_cond_kernel", "plain": "hawkesjd_chain_rng_kernel"}


def chain_and_params():
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    f = np.load(os.path.join(ROOT, "tests", "golden", "hawkes_analytic.npz"))
    m = f["ttms"].size
    chain = dict(ttms=f["ttms"], forwards=f["forwards"], discfactors=f["discfactors"], strikes_ttms=[f[f"strikes_{i}"] for i in range(m)],
                 optiontypes_ttms=[f[f"types_{i}"] for i in range(m)])
    p = hp.HawkesJDParams()
    return chain, {k: getattr(p, k) for k in hp.PARAM_NAMES}


def routes():
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    return {"conditional": hp.hawkesjd_mc_chain_pricer_conditional, "plain": hp.hawkesjd_mc_chain_pricer,
            "greeks": hp.hawkesjd_mc_chain_greeks_conditional}


def timed(route, name, n, reps, chain, kw):
    """(median whole-call ms, median stepping-launch ms) of `reps` calls after 3 warm-up calls"""
    from stochvolmodels_amd.engine import get_engine
    for _ in range(3):
        route(nb_path=n, **chain, **kw)
    eng = get_engine(n)
    wall, step = [], []
    for _ in range(reps):
        eng.start_kernel_timing()
        t0 = time.perf_counter()
        route(nb_path=n, **chain, **kw)
        wall.append(1e3 * (time.perf_counter() - t0))
        step += eng.stop_kernel_timing().get(KERNELS[name], [])
    return float(np.median(wall)), float(np.median(step))


def stepping_only(reps):
    """the child of the block A/B: the conditional stepping launch's ms per size, on whichever library SVMC_LIB names"""
    chain, kw = chain_and_params()
    out = {}
    for n in SIZES:
        call_ms, step_ms = timed(routes()["conditional"], "conditional", n, reps, chain, kw)
        out[str(n)] = {"call_ms": call_ms, "stepping_ms": step_ms}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hawkes_cmc_bench.json"))
    ap.add_argument("--block-ab", default=None)
    ap.add_argument("--stepping-only", action="store_true")
    a = ap.parse_args()
    if a.stepping_only:
        return stepping_only(a.reps)
    from stochvolmodels_amd import build as svbuild
    chain, kw = chain_and_params()
    meta = json.load(open(svbuild.ISA_JSON))["metadata"]
    regs = {k: v for k, v in meta.items() if "hawkes_chain_cond_kernel" in k or "hawkesjd_chain_rng_kernel" in k}
    out = {"chain": "BTC test chain, 4 expiries, 49 options", "steps": 780, "steps_per_year": 1800, "reps": a.reps, "seed": a.seed,
           "kernel_metadata": regs, "mc": {}}
    forwards = chain["forwards"]
    near = [int(np.argmin(np.abs(np.log(k / f)))) for k, f in zip(chain["strikes_ttms"], forwards)]
    offs = np.concatenate([[0], np.cumsum([k.size for k in chain["strikes_ttms"]])])
    near_flat = [int(offs[i] + j) for i, j in enumerate(near)]
    for n in SIZES:
        row = {}
        for name, route in routes().items():
            call_ms, step_ms = timed(route, name, n, a.reps, chain, kw)
            row[name] = {"call_ms": call_ms, "stepping_ms": step_ms}
        row["time_ratio"] = row["conditional"]["call_ms"] / row["plain"]["call_ms"]
        row["stepping_ratio"] = row["conditional"]["stepping_ms"] / row["plain"]["stepping_ms"]
        _, ce = routes()["conditional"](nb_path=n, seed=a.seed, **chain, **kw)
        _, pe = routes()["plain"](nb_path=n, seed=a.seed, **chain, **kw)
        with np.errstate(all="ignore"):
            vr = (np.concatenate(pe) / np.concatenate(ce)) ** 2
        ok = np.isfinite(vr)
        row["variance_ratio"] = {"per_quote": [round(float(v), 3) if np.isfinite(v) else None for v in vr],
                                 "median": float(np.median(vr[ok])), "min": float(np.min(vr[ok])), "max": float(np.max(vr[ok])),
                                 "nearest_the_forward": [float(vr[j]) for j in near_flat]}
        row["cost_at_equal_error"] = {"median": row["time_ratio"] / row["variance_ratio"]["median"],
                                      "nearest_the_forward": [row["time_ratio"] / float(vr[j]) for j in near_flat],
                                      "worst_quote": row["time_ratio"] / row["variance_ratio"]["min"]}
        out["mc"][str(n)] = row
    if a.block_ab:
        ab = {}
        for label, lib in (("block_256", None), ("block_512", os.path.abspath(a.block_ab))):
            env = dict(os.environ)
            env.pop("SVMC_LIB", None)
            if lib is not None:
                env["SVMC_LIB"] = lib
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--stepping-only", "--reps", str(a.reps)], env=env,
                               capture_output=True, text=True, timeout=240)
            if r.returncode != 0:
                raise SystemExit(f"{label}: the child failed ({r.returncode}):\n{r.stdout[-1000:]}{r.stderr[-2000:]}")
            ab[label] = json.loads(r.stdout.strip().splitlines()[-1])
        out["block_ab"] = ab
    text = json.dumps(out)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
