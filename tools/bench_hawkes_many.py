#!/usr/bin/env python
"""
Many independent Hawkes jump-diffusion jobs of one chain in one call against a loop of the same single calls
(hawkesjd_mc_chain_pricer_many vs hawkesjd_mc_chain_pricer, same parameters, same seeds): the BTC test chain of
tools/bench_hawkes.py (4 expiries, 49 options, 780 steps at the reference's 1800 per year; tests/golden/hawkes_analytic.npz),
J in {1, 2, 5, 16, 64} at 10^5 paths and J in {1, 2, 5} at 2^20.  The single call is the library's one-job code path, timed in
the same process.  Also: five jobs x three gammas through hawkesjd_mc_chain_pricer_with_risk_premia_gammas_many against five
single hawkesjd_mc_chain_pricer_with_risk_premia_gammas calls at 10^5 paths.

Per case: warm-up calls of both sides, then REPS timed calls of each side, the sides alternating call by call; each timed call
is the host clock around the whole call (every call ends in the library's stream synchronise).  Reported: the medians, the loop's
time over the batch's, the aggregate path-steps/s of each side, the batch's stepping time (session events around its stepping
launch and spot-sum reduce) and whether every job's results are bit-equal to its single call.

    python tools/bench_hawkes_many.py [--out profiles/hawkes_many_bench.json] [--reps 10] [--quick]
"""
from __future__ import annotations

import argparse
import ctypes as C
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
from stochvolmodels_amd import _lib                                    # noqa: E402
from stochvolmodels_amd.engine import get_engine                       # noqa: E402
from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp          # noqa: E402
from stochvolmodels_amd.utils.funcs import time_grid_steps            # noqa: E402

SPY = 1800
GAMMAS = [-1.0, 0.0, 1.0]


def btc_chain():
    f = np.load(os.path.join(ROOT, "tests", "golden", "hawkes_analytic.npz"))
    m = f["ttms"].size
    return dict(ttms=f["ttms"], forwards=f["forwards"], discfactors=f["discfactors"],
                strikes_ttms=[f[f"strikes_{i}"] for i in range(m)], optiontypes_ttms=[f[f"types_{i}"] for i in range(m)])


def total_steps(ttms) -> int:
    t0, n = 0.0, 0
    for t in ttms:
        n += time_grid_steps(ttm=t - t0, nb_steps_per_year=SPY)[0]
        t0 = t
    return n


def jobs(n_jobs: int):
    """a parameter sweep around the defaults: sigma and both start intensities move with the job"""
    d = hp.HawkesJDParams()
    return [dataclasses.replace(d, sigma=d.sigma * (1 + 0.01 * (j % 16)), lambda_p=d.lambda_p * (1 + 0.02 * (j % 7)),
                                lambda_m=d.lambda_m * (1 + 0.03 * (j % 5))) for j in range(n_jobs)]


def model_kw(p):
    kw = p.to_dict()
    kw.pop("risk_premia_gamma")
    return kw


def timed(fn) -> float:
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def flat(result) -> np.ndarray:
    """every number of a pricer's return value (nested lists / tuples of arrays), in order"""
    if isinstance(result, np.ndarray):
        return result.ravel()
    return np.concatenate([flat(r) for r in result]) if len(result) else np.zeros(0)


def same_bits(a, b) -> bool:
    return len(a) == len(b) and all(np.array_equal(flat(x), flat(y), equal_nan=True) for x, y in zip(a, b))


def stepping_ms(batch, nb_path, ch, L, reps):
    eng = get_engine(nb_path)
    sess = eng.fused_chain_session(len(ch["ttms"]), sum(np.size(k) for k in ch["strikes_ttms"]))
    _lib.check(L.svmc_session_time_stepping(sess, 1))
    out = []
    try:
        for _ in range(reps):
            batch()
            ms = C.c_float()
            _lib.check(L.svmc_session_last_stepping_ms(sess, C.byref(ms)))
            out.append(float(ms.value))
    finally:
        _lib.check(L.svmc_session_time_stepping(sess, 0))
    return statistics.median(out)


def case(kind, n_jobs, nb_path, reps, ch, L):
    ps = jobs(n_jobs)
    seeds = [1000 + j for j in range(n_jobs)]
    if kind == "plain":
        def batch():
            return sv.hawkesjd_mc_chain_pricer_many(ps, nb_path=nb_path, nb_steps_per_year=SPY, seeds=seeds, **ch)

        def loop():
            return [hp.hawkesjd_mc_chain_pricer(nb_path=nb_path, nb_steps_per_year=SPY, seed=s, **ch, **model_kw(p))
                    for p, s in zip(ps, seeds)]
    else:
        def batch():
            return sv.hawkesjd_mc_chain_pricer_with_risk_premia_gammas_many(
                ps, nb_path=nb_path, nb_steps_per_year=SPY, seeds=seeds, risk_premia_gammas=GAMMAS, return_forwards=True, **ch)

        def loop():
            return [hp.hawkesjd_mc_chain_pricer_with_risk_premia_gammas(
                nb_path=nb_path, nb_steps_per_year=SPY, seed=s, risk_premia_gammas=GAMMAS, return_forwards=True, **ch, **model_kw(p))
                for p, s in zip(ps, seeds)]
    ok = same_bits(batch(), loop())
    for _ in range(2):
        batch()
        loop()
    tb, tl = [], []
    for q in range(reps):
        for fn in ((batch, loop) if q % 2 == 0 else (loop, batch)):
            (tb if fn is batch else tl).append(timed(fn))
    ms = stepping_ms(batch, nb_path, ch, L, min(reps, 5))
    work = n_jobs * nb_path * total_steps(ch["ttms"])
    mb, ml = statistics.median(tb), statistics.median(tl)
    return {"kind": kind, "n_jobs": n_jobs, "nb_path": nb_path, "n_gammas": len(GAMMAS) if kind == "tilted" else 0,
            "batch_ms": round(mb, 4), "loop_ms": round(ml, 4), "loop_over_batch": round(ml / mb, 3),
            "batch_path_steps_per_s": float(f"{work / (mb * 1e-3):.4g}"), "loop_path_steps_per_s": float(f"{work / (ml * 1e-3):.4g}"),
            "batch_stepping_ms": round(ms, 4), "stepping_path_steps_per_s": float(f"{work / (ms * 1e-3):.4g}"),
            "same_bits": bool(ok), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hawkes_many_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="J in {1, 5} at 10^5 paths and the tilted case only")
    a = ap.parse_args()
    L = _lib.load()
    ch = btc_chain()
    cases = [("plain", j, 100_000) for j in ((1, 5) if a.quick else (1, 2, 5, 16, 64))]
    if not a.quick:
        cases += [("plain", j, 1 << 20) for j in (1, 2, 5)]
    cases.append(("tilted", 5, 100_000))
    from stochvolmodels_amd import build as svbuild
    meta = json.load(open(svbuild.ISA_JSON)).get("metadata", {})
    regs = {("many" if "many" in k else "single"): v for k, v in meta.items() if "hawkesjd_chain_rng" in k}
    rows = []
    for kind, n_jobs, nb_path in cases:
        r = case(kind, n_jobs, nb_path, a.reps, ch, L)
        rows.append(r)
        print(json.dumps(r), flush=True)
        get_engine(nb_path).synchronize()
    info = C.create_string_buffer(256)
    name = info.value.decode(errors="replace") if L.svmc_device_info(0, info, 256, None, None, None) == 0 else ""
    out = {"what": "many Hawkes jobs of one chain per call vs a loop of single calls (tools/bench_hawkes_many.py)", "device": name,
           "chain": "BTC test chain, 4 expiries, 49 options, 1800 steps/yr", "total_steps": total_steps(ch["ttms"]),
           "timing": "median of `reps` warm calls per side, host clock around each whole call (ends in a stream synchronise), "
                     "sides alternating",
           "stepping_kernel_registers": regs, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
