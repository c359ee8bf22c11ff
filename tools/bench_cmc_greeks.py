"""
Conditional Monte Carlo Greeks (logsv_mc_chain_greeks_conditional) against what a user did before them: (a) one
logsv_mc_chain_pricer_conditional call, which the new call contains, and (b) three such calls at F - h, F, F + h, the cost of a
finite-difference delta and gamma (which has no error and a second difference that drowns in rounding).  LogSV, LOGSV_BTC_PARAMS,
the 4 x 13 chain of tools/bench_mc_many.py at 360 steps per year (364 steps), n_path 10^5 and 2^20.

Per case: warm-up calls of every side, then REPS rounds that alternate the sides in one process, each call timed by the host clock
(a call returns synchronised).  Recorded: the medians (and min / max) of each side's whole call, the stepping launch of the new call
and of the single conditional call (the session's events around it), and the TAIL of each -- the call less its stepping launch: the
table's upload, the launches, the download and the host's shaping of the result rows.

    python tools/bench_cmc_greeks.py [--out profiles/cmc_greeks_bench.json] [--reps 10] [--only NAME]
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

H = 1e-4


def chain():
    t4, k13 = np.array([1 / 12, 0.25, 0.5, 1.0]), np.linspace(0.7, 1.3, 13)
    return dict(ttms=t4, forwards=np.ones(4), discfactors=np.ones(4), strikes_ttms=[k13.copy() for _ in t4],
                optiontypes_ttms=[np.where(k13 < 1.0, "P", "C") for _ in t4])


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def run_case(n, reps):
    p, ch = sv.LOGSV_BTC_PARAMS, chain()
    kw = dict(v0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2, beta=p.beta, volvol=p.volvol, vol_backbone_etas=np.ones(4))
    bumped = [dict(ch, forwards=ch["forwards"] * f) for f in (1.0 - H, 1.0, 1.0 + H)]
    eng = get_engine(n)

    def three(seed):
        return [sv.logsv_mc_chain_pricer_conditional(nb_path=n, seed=seed, **c, **kw) for c in bumped]

    sides = {
        "greeks": lambda seed: sv.logsv_mc_chain_greeks_conditional(nb_path=n, seed=seed, **ch, **kw),
        "conditional": lambda seed: sv.logsv_mc_chain_pricer_conditional(nb_path=n, seed=seed, **ch, **kw),
        "three_conditional": three,
    }
    for f in sides.values():                                  # warm: buffers, the session, the chains' marshalled arrays
        f(1)
        f(2)
    wall, step = {k: [] for k in sides}, {k: [] for k in sides}
    order = list(sides)
    for r in range(reps):
        for k in (order if r % 2 == 0 else order[::-1]):
            eng.start_kernel_timing()
            t0 = time.perf_counter()
            sides[k](100 + r)
            wall[k].append((time.perf_counter() - t0) * 1e3)
            step[k].append(sum(sum(v) for v in eng.stop_kernel_timing().values()))
    tail = {k: statistics.median([w - s for w, s in zip(wall[k], step[k])]) for k in sides}
    med = {k: statistics.median(wall[k]) for k in sides}
    out = dict(case=f"n{n}", n_path=n, steps=364, quotes=52, reps=reps,
               greeks=dict(call_ms=spread(wall["greeks"]), stepping_ms=spread(step["greeks"]), tail_ms=tail["greeks"]),
               conditional=dict(call_ms=spread(wall["conditional"]), stepping_ms=spread(step["conditional"]), tail_ms=tail["conditional"]),
               three_conditional=dict(call_ms=spread(wall["three_conditional"]), stepping_ms=spread(step["three_conditional"]),
                                      tail_ms=tail["three_conditional"]),
               greeks_over_conditional=med["greeks"] / med["conditional"], greeks_over_three_conditional=med["greeks"] / med["three_conditional"],
               greeks_tail_less_conditional_tail_ms=tail["greeks"] - tail["conditional"])
    print(f"{out['case']}: greeks {med['greeks']:.3f} ms (stepping {out['greeks']['stepping_ms']['median']:.3f}, tail {tail['greeks']:.3f}), "
          f"conditional {med['conditional']:.3f} ms (stepping {out['conditional']['stepping_ms']['median']:.3f}, tail "
          f"{tail['conditional']:.3f}), three conditional calls {med['three_conditional']:.3f} ms; greeks / conditional "
          f"{out['greeks_over_conditional']:.3f}, greeks / three {out['greeks_over_three_conditional']:.3f}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmc_greeks_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    rows = [run_case(n, a.reps) for n in (100000, 1 << 20) if a.only in (None, f"n{n}")]
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(dict(tool="tools/bench_cmc_greeks.py", timing="host clock around a synchronised call, medians of the warm rounds, "
                           "the three sides alternating in one process; stepping: the session's events around the stepping launch; "
                           "tail: the call less its stepping launch", rows=rows), fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
