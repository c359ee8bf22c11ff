"""
The conditional Monte Carlo calibration objective (logsv_mc_chain_pricer_conditional_sets) against what a user
had before it, and what its smaller noise buys a calibration.  LogSV, LOGSV_BTC_PARAMS, the 4 x 13 chain of tools/bench_mc_many.py
at 360 steps per year (364 steps).

 evaluation   time per objective evaluation (prices AND implied vols of n_sets parameter sets on one stream), n_sets 1 and 6, paths
              8 192, 2^14 and 10^5: the new call against the two routes of the commit before it -- n_sets single
              logsv_mc_chain_pricer_conditional calls plus the host implied-vol routine, and logsv_mc_chain_pricer_conditional_many
              on n_sets same-seed jobs plus the host routine -- and against the plain estimator's frozen-stream graph (row f3) at the
              same path count.  The gate: the new call's median below the minimum of either earlier route at n_sets = 6.
 noise        the spread over 32 seeds of the objective value at LOGSV_BTC_PARAMS (market vols: the mean conditional vols of the 32
              seeds at 10^5 paths): plain at 10^5 paths, conditional at 10^5 / 16 and at 10^5, each next to its time per evaluation.
 calibration  a whole PARAMS5 calibration from a 15 % moved start with each engine at the path counts of about equal spread.
 --trace      only 50 evaluations of six sets at 10^5 paths, for a kernel trace of the new call.

Warm-up calls of every side, then REPS rounds that alternate the sides in one process, each side timed by the host clock (every
call returns synchronised).

    python tools/bench_cmc_calibration.py [--out profiles/cmc_calibration_bench.json] [--reps 10] [--trace]
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
from stochvolmodels_amd.data.option_chain import black_ivols_native   # noqa: E402
from stochvolmodels_amd.pricers.logsv_pricer import (draw_fixed_randoms_on_device, logsv_mc_chain_pricer_fixed_randoms,  # noqa: E402
                                                     logsv_mc_chain_pricer_fixed_randoms_batch)

SPY = 360


def chain():
    t4, k13 = np.array([1 / 12, 0.25, 0.5, 1.0]), np.linspace(0.7, 1.3, 13)
    return dict(ttms=t4, forwards=np.ones(4), discfactors=np.ones(4), strikes_ttms=[k13.copy() for _ in t4],
                optiontypes_ttms=[np.where(k13 < 1.0, "P", "C") for _ in t4])


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def bumped_sets(n_sets):
    """LOGSV_BTC_PARAMS and its forward-difference neighbours: the sets of an optimizer iterate"""
    p = sv.LOGSV_BTC_PARAMS
    base = dict(sigma0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2, beta=p.beta, volvol=p.volvol)
    out = [sv.LogSvParams(**base)]
    for name in ("sigma0", "theta", "kappa1", "beta", "volvol")[:n_sets - 1]:
        out.append(sv.LogSvParams(**dict(base, **{name: base[name] + 1.5e-8})))
    return out


def host_vols(prices, ch):
    return [black_ivols_native(np.ravel(p), float(t), float(f), k, ty, float(d))
            for p, t, f, k, ty, d in zip(prices, ch["ttms"], ch["forwards"], ch["strikes_ttms"], ch["optiontypes_ttms"], ch["discfactors"])]


def kw_of(p, ch):
    return dict(v0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2, beta=p.beta, volvol=p.volvol,
                vol_backbone_etas=p.get_vol_backbone_etas(ttms=ch["ttms"]))


def timed(sides, reps, warm=3):
    for f in sides.values():
        for _ in range(warm):
            f()
    wall = {k: [] for k in sides}
    order = list(sides)
    for r in range(reps):
        for k in (order if r % 2 == 0 else order[::-1]):
            t0 = time.perf_counter()
            sides[k]()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    return wall


def run_evaluation(n, n_sets, reps):
    ch, plist, seed = chain(), bumped_sets(n_sets), 10
    resident = draw_fixed_randoms_on_device(ttms=ch["ttms"], nb_path=n, nb_steps_per_year=SPY, seed=seed)

    def singles():
        return [host_vols(sv.logsv_mc_chain_pricer_conditional(nb_path=n, nb_steps_per_year=SPY, seed=seed, **ch, **kw_of(p, ch))[0], ch)
                for p in plist]

    def many():
        out = sv.logsv_mc_chain_pricer_conditional_many(plist, nb_path=n, nb_steps_per_year=SPY, seeds=[seed] * n_sets, **ch)
        return [host_vols(pr, ch) for pr, _ in out]

    def plain():
        if n_sets == 1:
            return logsv_mc_chain_pricer_fixed_randoms(W0s=resident, W1s=None, dts=None, return_ivols=True, **ch, **kw_of(plist[0], ch))
        return logsv_mc_chain_pricer_fixed_randoms_batch(params_list=plist, W0s=resident, return_ivols=True, **ch)

    sides = {
        "sets": lambda: sv.logsv_mc_chain_pricer_conditional_sets(plist, nb_path=n, nb_steps_per_year=SPY, seed=seed, return_ivols=True, **ch),
        "single_calls_plus_host_vols": singles,
        "many_plus_host_vols": many,
        "plain_frozen_graph": plain,
    }
    try:
        wall = timed(sides, reps)
    finally:
        resident.free()
    med = {k: statistics.median(v) for k, v in wall.items()}
    parent_min = min(min(wall["single_calls_plus_host_vols"]), min(wall["many_plus_host_vols"]))
    out = dict(case=f"n{n}_sets{n_sets}", n_path=n, n_sets=n_sets, steps=364, quotes=52, reps=reps,
               **{k + "_ms": spread(v) for k, v in wall.items()},
               sets_over_single_calls=med["sets"] / med["single_calls_plus_host_vols"], sets_over_many=med["sets"] / med["many_plus_host_vols"],
               sets_over_plain_frozen=med["sets"] / med["plain_frozen_graph"],
               gate_sets_median_below_parent_minimum=bool(med["sets"] < parent_min))
    print(f"{out['case']}: sets {med['sets']:.3f} ms; {n_sets} single calls + host vols {med['single_calls_plus_host_vols']:.3f} ms; many + host "
          f"vols {med['many_plus_host_vols']:.3f} ms; plain frozen graph {med['plain_frozen_graph']:.3f} ms; gate "
          f"{out['gate_sets_median_below_parent_minimum']}", flush=True)
    return out


def cond_vols(p, n, seed, ch):
    return np.concatenate(sv.logsv_mc_chain_pricer_conditional_sets([p], nb_path=n, nb_steps_per_year=SPY, seed=seed, return_ivols=True, **ch)[0][2])


def plain_vols(p, n, seed, ch):
    resident = draw_fixed_randoms_on_device(ttms=ch["ttms"], nb_path=n, nb_steps_per_year=SPY, seed=seed)
    try:
        return np.concatenate(logsv_mc_chain_pricer_fixed_randoms(W0s=resident, W1s=None, dts=None, return_ivols=True, **ch, **kw_of(p, ch))[2])
    finally:
        resident.free()


def run_noise(reps, n_big=100000, n_seeds=32):
    ch, p = chain(), sv.LOGSV_BTC_PARAMS
    n_small = n_big // 16
    seeds = [3000 + s for s in range(n_seeds)]
    big = np.array([cond_vols(p, n_big, s, ch) for s in seeds])
    market = np.nanmean(big, axis=0)
    obj = lambda v: float(np.nansum(np.square(v - market)))           # noqa: E731
    rows = {}
    for name, fn, n in (("plain", plain_vols, n_big), ("conditional_small", cond_vols, n_small), ("conditional", cond_vols, n_big)):
        vals = [obj(v) for v in (big if name == "conditional" else [fn(p, n, s, ch) for s in seeds])]
        resident = draw_fixed_randoms_on_device(ttms=ch["ttms"], nb_path=n, nb_steps_per_year=SPY, seed=10) if name == "plain" else None
        side = (lambda: logsv_mc_chain_pricer_fixed_randoms(W0s=resident, W1s=None, dts=None, return_ivols=True, **ch, **kw_of(p, ch))) \
            if name == "plain" else (lambda: cond_vols(p, n, 10, ch))
        try:
            wall = timed({"eval": side}, reps)["eval"]
        finally:
            if resident is not None:
                resident.free()
        rows[name] = dict(n_path=n, objective_mean=float(np.mean(vals)), objective_spread=float(np.std(vals, ddof=1)),
                          evaluation_ms=spread(wall))
        print(f"noise {name} at {n} paths: objective {rows[name]['objective_mean']:.3e} +- {rows[name]['objective_spread']:.3e} over "
              f"{n_seeds} seeds, {statistics.median(wall):.3f} ms per evaluation", flush=True)
    return dict(case="objective_noise", n_seeds=n_seeds, objective="unweighted sum of squared vol differences to the mean conditional "
                "vols of the seeds at the large path count, 52 quotes", rows=rows), market


def run_calibration(market, n_plain=100000, n_cond=6250):
    ch = chain()
    vols = [market[13 * i:13 * (i + 1)] for i in range(4)]
    oc = sv.OptionChain(ids=np.array(["a", "b", "c", "d"]), bid_ivs=vols, ask_ivs=vols, **ch)
    p = sv.LOGSV_BTC_PARAMS
    start = sv.LogSvParams(sigma0=1.15 * p.sigma0, theta=1.15 * p.theta, kappa1=1.15 * p.kappa1, kappa2=None, beta=1.15 * p.beta,
                           volvol=1.15 * p.volvol)
    rows = {}
    MC = sv.CalibrationEngine.MC
    for name, kw in (("plain_frozen", dict(nb_path=n_plain, device_randoms=True)), ("conditional", dict(nb_path=n_cond, estimator="conditional"))):
        pricer = sv.LogSVPricer()
        pricer.calibrate_model_params_to_chain(oc, start, calibration_engine=MC, nb_steps=SPY, seed=10, disp=False, **kw)      # warm
        t0 = time.perf_counter()
        fit = pricer.calibrate_model_params_to_chain(oc, start, calibration_engine=MC, nb_steps=SPY, seed=10, disp=False, **kw)
        wall = (time.perf_counter() - t0) * 1e3
        rows[name] = dict(n_path=kw["nb_path"], wall_ms=wall, n_eval=pricer.last_calibration["n_eval"],
                          n_gradient_batches=pricer.last_calibration["n_gradient_batches"], objective=pricer.last_calibration["objective"],
                          fit={k: float(getattr(fit, k)) for k in ("sigma0", "theta", "kappa1", "kappa2", "beta", "volvol")})
        print(f"calibration {name} at {kw['nb_path']} paths: {wall:.1f} ms, n_eval {rows[name]['n_eval']}, objective "
              f"{rows[name]['objective']:.3e}, fit {rows[name]['fit']}", flush=True)
    return dict(case="params5_calibration", start="LOGSV_BTC_PARAMS with the five fitted parameters moved by 15 %", rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmc_calibration_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if a.trace:
        ch, plist = chain(), bumped_sets(6)
        for _ in range(50):
            sv.logsv_mc_chain_pricer_conditional_sets(plist, nb_path=100000, nb_steps_per_year=SPY, seed=10, return_ivols=True, **ch)
        return
    rows = [run_evaluation(n, n_sets, a.reps) for n in (8192, 1 << 14, 100000) for n_sets in (1, 6)]
    noise, market = run_noise(a.reps)
    rows.append(noise)
    rows.append(run_calibration(market))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(dict(tool="tools/bench_cmc_calibration.py", timing="host clock around synchronised calls, medians of the warm rounds, "
                           "the sides alternating in one process", rows=rows), fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
