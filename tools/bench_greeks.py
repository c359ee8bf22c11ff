"""
Monte Carlo chain Greeks (logsv_mc_chain_greeks) against the route the library had before it: the same 1 + 2P
bumped jobs through logsv_mc_chain_pricer_many at one seed and a difference on the host, which yields the sensitivities and no
errors.  LogSV, LOGSV_BTC_PARAMS, the 4 x 13 chain of tools/bench_mc_many.py at 360 steps per year (364 steps):

    n_path 10^5 and 2^20, P = 1 (sigma0) and P = 6 (all parameters)

Per case: warm-up calls of every side, then REPS rounds that alternate the sides in one process, each call timed by the host
clock (a call returns synchronised).  Recorded: the medians (and min / max) of the whole Greeks call, of the many-job call on the
same jobs and of the single plain call; the stepping launch of the Greeks call and of the plain call (the session's events around
it); and the TAIL of each, the call less its stepping launch -- for the Greeks call the plain tail on job 0, the four launches of
the Greeks tail, the landing and the host's shaping of 3 + 3P result rows, for the plain call its tail, landing and shaping.

    python tools/bench_greeks.py [--out profiles/greeks_bench.json] [--reps 10] [--only NAME]
"""
from __future__ import annotations

import argparse
import dataclasses
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
from stochvolmodels_amd.mc_greeks import LOGSV_GREEK_PARAMS, greeks_bumps      # noqa: E402


def chain():
    t4, k13 = np.array([1 / 12, 0.25, 0.5, 1.0]), np.linspace(0.7, 1.3, 13)
    return dict(ttms=t4, forwards=np.ones(4), discfactors=np.ones(4), strikes_ttms=[k13.copy() for _ in t4],
                optiontypes_ttms=[np.where(k13 < 1.0, "P", "C") for _ in t4])


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def run_case(n, wrt, reps):
    p, ch = sv.LOGSV_BTC_PARAMS, chain()
    names, hs = greeks_bumps("logsv", {k: getattr(p, k) for k in LOGSV_GREEK_PARAMS}, wrt)
    bumped = [p] + [dataclasses.replace(p, **{nm: getattr(p, nm) + sgn * h}) for nm, h in zip(names, hs) for sgn in (1.0, -1.0)]
    kw = dict(v0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2, beta=p.beta, volvol=p.volvol, vol_backbone_etas=np.ones(4))
    eng = get_engine(n)
    sides = {
        "greeks": lambda seed: sv.logsv_mc_chain_greeks(p, wrt=names, nb_path=n, seed=seed, **ch),
        "many": lambda seed: sv.logsv_mc_chain_pricer_many(bumped, nb_path=n, seeds=[seed] * len(bumped), **ch),
        "plain": lambda seed: sv.logsv_mc_chain_pricer(nb_path=n, seed=seed, **ch, **kw),
    }
    for f in sides.values():                                  # warm: buffers, the session, the chain's marshalled arrays
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
    tail = {k: statistics.median([w - s for w, s in zip(wall[k], step[k])]) for k in ("greeks", "plain")}
    out = dict(case=f"n{n}_P{len(names)}", n_path=n, steps=364, n_params=len(names), n_jobs=len(bumped), wrt=list(names), reps=reps,
               greeks=dict(call_ms=spread(wall["greeks"]), stepping_ms=spread(step["greeks"]), tail_ms=tail["greeks"]),
               many=dict(call_ms=spread(wall["many"])),
               plain=dict(call_ms=spread(wall["plain"]), stepping_ms=spread(step["plain"]), tail_ms=tail["plain"]),
               greeks_over_many=statistics.median(wall["greeks"]) / statistics.median(wall["many"]),
               greeks_tail_less_plain_tail_ms=tail["greeks"] - tail["plain"])
    print(f"{out['case']}: greeks {out['greeks']['call_ms']['median']:.3f} ms (stepping {out['greeks']['stepping_ms']['median']:.3f}, "
          f"tail {tail['greeks']:.3f}), many {out['many']['call_ms']['median']:.3f} ms, plain {out['plain']['call_ms']['median']:.3f} ms "
          f"(stepping {out['plain']['stepping_ms']['median']:.3f}, tail {tail['plain']:.3f}); greeks / many "
          f"{out['greeks_over_many']:.3f}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "greeks_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    rows = []
    for n in (100000, 1 << 20):
        for wrt in (("sigma0",), None):
            name = f"n{n}_P{1 if wrt else 6}"
            if a.only in (None, name):
                rows.append(run_case(n, wrt, a.reps))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(dict(tool="tools/bench_greeks.py", timing="host clock around a synchronised call, medians of the warm rounds, the "
                           "three sides alternating in one process; stepping: the session's events around the stepping launch",
                           rows=rows), fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
