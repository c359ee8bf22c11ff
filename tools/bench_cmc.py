"""
Conditional against plain Monte Carlo chain pricing (logsv_mc_chain_pricer_conditional / heston_mc_chain_pricer_conditional vs
logsv_mc_chain_pricer / heston_mc_chain_pricer, same parameters, same path counts):

    c2            LogSV, LOGSV_BTC_PARAMS, 2^20 paths x 1024 steps x 21 strikes (bench.py's C2)
    chain_1e5     LogSV, LOGSV_BTC_PARAMS, the 4 x 13 chain of tools/bench_mc_many.py at 360 steps per year (364 steps), 10^5 paths
    chain_4e5     the same at 4 x 10^5 paths
    c3_euler      Heston base set, 2^22 paths x 4 x 128 steps, 4 x 21 strikes, Euler (bench.py's C3)

Per case: warm-up calls of both sides, then REPS rounds that alternate conditional and plain in the same process, each call timed
by the host clock (a call returns synchronised).  Recorded: the medians (and min / max) of the whole call and of the stepping
launch (the session's events around it; for the plain side its spot-sum reduce rides inside), the rest of the call (payoff
launches, finish, download, host), per quote (se_plain / se_cond)^2, and the product "paths for equal error x time per path"
against the plain pricer: cost = (t_cond / t_plain) / variance ratio (below 1: the conditional estimator is cheaper at equal error).
Kernel times proper come from a run of this tool under `rocprofv3 --kernel-trace --stats -- python tools/bench_cmc.py --only c2
--reps 3 --out ""` (a run of its own; profiles/cmc_bench.json keeps its rows under "rocprofv3").

    python tools/bench_cmc.py [--out profiles/cmc_bench.json] [--reps 10] [--only NAME]
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
from stochvolmodels_amd.engine import get_engine                       # noqa: E402


def cases():
    lp = sv.LOGSV_BTC_PARAMS
    logsv = dict(v0=lp.sigma0, theta=lp.theta, kappa1=lp.kappa1, kappa2=lp.kappa2, beta=lp.beta, volvol=lp.volvol)
    kk = np.linspace(0.5, 1.5, 21)
    c2 = dict(ttms=np.array([1.0]), forwards=np.ones(1), discfactors=np.ones(1), strikes_ttms=[kk],
              optiontypes_ttms=[np.where(kk >= 1.0, "C", "P")])
    t4, k13 = np.array([1 / 12, 0.25, 0.5, 1.0]), np.linspace(0.7, 1.3, 13)
    c4 = dict(ttms=t4, forwards=np.ones(4), discfactors=np.ones(4), strikes_ttms=[k13.copy() for _ in t4],
              optiontypes_ttms=[np.where(k13 < 1.0, "P", "C") for _ in t4])
    t3 = np.array([0.25, 0.5, 0.75, 1.0])
    c3 = dict(ttms=t3, forwards=np.ones(4), discfactors=np.ones(4), strikes_ttms=[kk] * 4, optiontypes_ttms=[np.where(kk >= 1.0, "C", "P")] * 4)
    heston = dict(v0=0.04, theta=0.04, kappa=4.0, rho=-0.5, volvol=0.4)
    lfn = (sv.logsv_mc_chain_pricer_conditional, sv.logsv_mc_chain_pricer)
    hfn = (sv.heston_mc_chain_pricer_conditional, sv.heston_mc_chain_pricer)
    return {
        "c2": dict(fns=lfn, chain=c2, kw=dict(logsv, vol_backbone_etas=np.ones(1), nb_steps_per_year=1023), n=1 << 20, steps=1024,
                   kernels=("logsv_chain_cmc_kernel", "logsv_rng_kernel")),
        "chain_1e5": dict(fns=lfn, chain=c4, kw=dict(logsv, vol_backbone_etas=np.ones(4), nb_steps_per_year=360), n=100000, steps=364,
                          kernels=("logsv_chain_cmc_kernel", "logsv_chain_rng_kernel")),
        "chain_4e5": dict(fns=lfn, chain=c4, kw=dict(logsv, vol_backbone_etas=np.ones(4), nb_steps_per_year=360), n=400000, steps=364,
                          kernels=("logsv_chain_cmc_kernel", "logsv_chain_rng_kernel")),
        "c3_euler": dict(fns=hfn, chain=c3, kw=dict(heston, nb_steps_per_year=508), n=1 << 22, steps=512,
                         kernels=("heston_chain_cmc_kernel", "heston_chain_rng_kernel")),
    }


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def run_case(name, c, reps):
    eng = get_engine(c["n"])
    call = [lambda seed, f=f: f(nb_path=c["n"], seed=seed, **c["chain"], **c["kw"]) for f in c["fns"]]
    for f in call:                                           # warm: buffers, the session, the chain's marshalled arrays
        f(1)
        f(2)
    wall, step = ([], []), ([], [])
    last = [None, None]
    for r in range(reps):
        for side in ((0, 1) if r % 2 == 0 else (1, 0)):
            eng.start_kernel_timing()
            t0 = time.perf_counter()
            last[side] = call[side](100 + r)
            wall[side].append((time.perf_counter() - t0) * 1e3)
            prof = eng.stop_kernel_timing()
            step[side].append(sum(sum(v) for v in prof.values()))
    ratios = [((pe / ce) ** 2).tolist() for ce, pe in zip(last[0][1], last[1][1])]
    flat = np.concatenate([np.asarray(r) for r in ratios])
    t_c, t_p = statistics.median(wall[0]), statistics.median(wall[1])
    med = float(np.median(flat))
    out = dict(case=name, n_path=c["n"], steps=c["steps"], reps=reps, kernels=dict(conditional=c["kernels"][0], plain=c["kernels"][1]),
               conditional=dict(call_ms=spread(wall[0]), stepping_ms=spread(step[0]),
                                rest_ms=statistics.median([w - s for w, s in zip(wall[0], step[0])])),
               plain=dict(call_ms=spread(wall[1]), stepping_ms=spread(step[1]),
                          rest_ms=statistics.median([w - s for w, s in zip(wall[1], step[1])])),
               variance_ratio=dict(min=float(flat.min()), median=med, max=float(flat.max()), per_quote=ratios),
               cost_at_equal_error=dict(at_median_ratio=(t_c / t_p) / med, at_min_ratio=(t_c / t_p) / float(flat.min())))
    print(f"{name}: call {t_c:.3f} vs {t_p:.3f} ms, stepping {out['conditional']['stepping_ms']['median']:.3f} vs "
          f"{out['plain']['stepping_ms']['median']:.3f} ms (plain min-max {out['plain']['stepping_ms']['min']:.3f}-"
          f"{out['plain']['stepping_ms']['max']:.3f}), variance ratio {flat.min():.1f} / {med:.1f} / {flat.max():.1f}, cost at equal "
          f"error {out['cost_at_equal_error']['at_median_ratio']:.4f}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmc_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    all_cases = cases()
    rows = [run_case(k, c, a.reps) for k, c in all_cases.items() if a.only in (None, k)]
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(dict(tool="tools/bench_cmc.py", timing="host clock around a synchronised call, medians of the warm rounds, "
                           "conditional and plain alternating in one process", rows=rows), fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
