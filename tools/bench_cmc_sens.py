"""
Parameter sensitivities of the conditional Monte Carlo estimator (logsv_mc_chain_greeks_conditional(wrt=...))
against what a user did before them -- the 1 + 2P single logsv_mc_chain_pricer_conditional calls at one seed, differenced on the
host with no error for the difference --, against row f12's call (logsv_mc_chain_greeks, the plain estimator) at the same P, and
the many-job conditional pricer at J = 5 against five single calls.  LogSV, LOGSV_BTC_PARAMS, the 4 x 13 chain of
tools/bench_mc_many.py at 360 steps per year (364 steps), n_path 10^5 and 2^20, P = 1 (sigma0) and P = 6 (every parameter).

Per case: warm-up calls of every side, then REPS rounds that alternate the sides in one process, each side timed by the host
clock (every call returns synchronised).  Recorded: the medians (and min / max) per side, the ratios the README quotes, and per
quote sens_stderr_plain^2 / sens_stderr_conditional^2 at equal path counts (one seed).

    python tools/bench_cmc_sens.py [--out profiles/cmc_sens_bench.json] [--reps 10] [--only NAME]
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
from stochvolmodels_amd.mc_greeks import LOGSV_GREEK_PARAMS, greeks_bumps, greeks_job_table   # noqa: E402

KW_OF = dict(sigma0="v0", theta="theta", kappa1="kappa1", kappa2="kappa2", beta="beta", volvol="volvol")


def chain():
    t4, k13 = np.array([1 / 12, 0.25, 0.5, 1.0]), np.linspace(0.7, 1.3, 13)
    return dict(ttms=t4, forwards=np.ones(4), discfactors=np.ones(4), strikes_ttms=[k13.copy() for _ in t4],
                optiontypes_ttms=[np.where(k13 < 1.0, "P", "C") for _ in t4])


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def run_case(n, wrt, reps):
    p, ch = sv.LOGSV_BTC_PARAMS, chain()
    etas = np.asarray(p.get_vol_backbone_etas(ttms=ch["ttms"]), dtype=np.float64)
    kw = dict(v0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2, beta=p.beta, volvol=p.volvol, vol_backbone_etas=etas)
    values = {k: getattr(p, k) for k in LOGSV_GREEK_PARAMS}
    names, h = greeks_bumps("logsv", values, wrt)
    rows = greeks_job_table("logsv", [values[k] for k in LOGSV_GREEK_PARAMS], names, h)
    singles = [dict(kw, **{KW_OF[k]: row[j] for j, k in enumerate(LOGSV_GREEK_PARAMS)}) for row in rows]

    def loop(seed):                                           # the parent commit's route: 1 + 2P single calls on one seed
        return [sv.logsv_mc_chain_pricer_conditional(nb_path=n, seed=seed, **ch, **s) for s in singles]

    sides = {
        "sens": lambda seed: sv.logsv_mc_chain_greeks_conditional(nb_path=n, seed=seed, wrt=names, **ch, **kw),
        "single_calls": loop,
        "plain_greeks": lambda seed: sv.logsv_mc_chain_greeks(p, nb_path=n, seed=seed, wrt=names, **ch),
    }
    for f in sides.values():                                  # warm: buffers, the session, the chains' marshalled arrays
        f(1)
        f(2)
    wall = {k: [] for k in sides}
    order = list(sides)
    for r in range(reps):
        for k in (order if r % 2 == 0 else order[::-1]):
            t0 = time.perf_counter()
            sides[k](100 + r)
            wall[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(wall[k]) for k in sides}
    cond, plain = sides["sens"](7), sides["plain_greeks"](7)
    ratios = {name: [((np.asarray(plain["sens_stderr"][name][i]) / np.asarray(cond["sens_stderr"][name][i])) ** 2).tolist()
                     for i in range(4)] for name in names}
    flat = np.concatenate([np.ravel(v) for rs in ratios.values() for v in rs])
    out = dict(case=f"n{n}_P{len(names)}", n_path=n, n_params=len(names), wrt=list(names), steps=364, quotes=52, reps=reps,
               sens_call_ms=spread(wall["sens"]), single_calls_ms=spread(wall["single_calls"]), n_single_calls=len(singles),
               plain_greeks_ms=spread(wall["plain_greeks"]), sens_over_single_calls=med["sens"] / med["single_calls"],
               sens_over_plain_greeks=med["sens"] / med["plain_greeks"],
               plain_over_conditional_sens_variance=dict(per_quote=ratios, min=float(flat.min()), median=float(np.median(flat)),
                                                         max=float(flat.max()), seed=7))
    print(f"{out['case']}: sens call {med['sens']:.3f} ms, the {len(singles)} single conditional calls {med['single_calls']:.3f} ms "
          f"(ratio {out['sens_over_single_calls']:.3f}), row f12's call {med['plain_greeks']:.3f} ms (ratio "
          f"{out['sens_over_plain_greeks']:.3f}); plain / conditional sens error squared {flat.min():.2f} .. {np.median(flat):.2f} .. "
          f"{flat.max():.1f}", flush=True)
    return out


def run_many(n, reps, J=5):
    p, ch = sv.LOGSV_BTC_PARAMS, chain()
    plist = [sv.LogSvParams(sigma0=p.sigma0 * (1 + 0.02 * j), theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2, beta=p.beta,
                            volvol=p.volvol * (1 - 0.03 * j)) for j in range(J)]
    seeds = list(range(11, 11 + J))

    def loop(_):
        return [sv.logsv_mc_chain_pricer_conditional(
            v0=q.sigma0, theta=q.theta, kappa1=q.kappa1, kappa2=q.kappa2, beta=q.beta, volvol=q.volvol,
            vol_backbone_etas=q.get_vol_backbone_etas(ttms=ch["ttms"]), nb_path=n, seed=s, **ch) for q, s in zip(plist, seeds)]

    sides = {"many": lambda _: sv.logsv_mc_chain_pricer_conditional_many(plist, nb_path=n, seeds=seeds, **ch), "single_calls": loop}
    for f in sides.values():
        f(0)
        f(0)
    wall = {k: [] for k in sides}
    order = list(sides)
    for r in range(reps):
        for k in (order if r % 2 == 0 else order[::-1]):
            t0 = time.perf_counter()
            sides[k](r)
            wall[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(wall[k]) for k in sides}
    out = dict(case=f"n{n}_many_J{J}", n_path=n, n_jobs=J, steps=364, quotes=52, reps=reps, many_call_ms=spread(wall["many"]),
               single_calls_ms=spread(wall["single_calls"]), many_over_single_calls=med["many"] / med["single_calls"])
    print(f"{out['case']}: many-job call {med['many']:.3f} ms, {J} single calls {med['single_calls']:.3f} ms (ratio "
          f"{out['many_over_single_calls']:.3f})", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmc_sens_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    rows = []
    for n in (100000, 1 << 20):
        for wrt in (("sigma0",), None):
            name = f"n{n}_P{1 if wrt else 6}"
            if a.only in (None, name):
                rows.append(run_case(n, wrt, a.reps))
        if a.only in (None, f"n{n}_many_J5"):
            rows.append(run_many(n, a.reps))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(dict(tool="tools/bench_cmc_sens.py", timing="host clock around synchronised calls, medians of the warm rounds, the "
                           "sides alternating in one process", rows=rows), fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
