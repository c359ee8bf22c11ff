"""
Many independent jobs of one chain in one call against a loop of the same single calls (logsv_mc_chain_pricer_many /
heston_mc_chain_pricer_many vs logsv_mc_chain_pricer / heston_mc_chain_pricer, same parameters, same seeds): the 4 x 13 chain
of tools/bench_calibration_mc.py (ttms 1/12, 1/4, 1/2, 1; 13 strikes 0.7-1.3) at 360 steps per year, J in {1, 2, 4, 5, 8, 16},
nb_path in {10^5, 4 x 10^5}, for LogSV, Heston Euler and Heston QE.

Per case: warm-up calls of both sides, then PASSES passes that alternate which side goes first, REPS timed calls of each side
per pass; the medians of the warm wall times, the aggregate path-steps/s of each side, the batch's stepping time (session
events around its stepping launch and spot-sum reduce: the rest of a call is payoff + finish + host), the shader clock of the
batch's stepping launch (svmc_clock_probe_read; LogSV only, the Heston generators carry no probe) and whether every job's
prices and standard errors are bit-equal to its single call.

    python tools/bench_mc_many.py [--out profiles/mc_many_bench.json] [--passes 5] [--reps 5] [--quick]
"""
from __future__ import annotations

import argparse
import ctypes as C
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
from stochvolmodels_amd.engine import get_engine, option_type_codes    # noqa: E402
from stochvolmodels_amd.utils.funcs import time_grid_steps            # noqa: E402

SPY = 360


def chain_4x13():
    ttms = np.array([1 / 12, 0.25, 0.5, 1.0])
    k = np.linspace(0.7, 1.3, 13)
    return dict(ttms=ttms, forwards=np.ones(4), discfactors=np.ones(4), strikes_ttms=[k.copy() for _ in ttms],
                optiontypes_ttms=[np.where(k < 1.0, "P", "C") for _ in ttms])


def total_steps(ttms) -> int:
    t0, n = 0.0, 0
    for t in ttms:
        n += time_grid_steps(ttm=t - t0, nb_steps_per_year=SPY)[0]
        t0 = t
    return n


def jobs(model: str, n_jobs: int):
    lp = sv.LOGSV_BTC_PARAMS
    if model == "logsv":
        return [sv.LogSvParams(sigma0=lp.sigma0 * (1 + 0.03 * j), theta=lp.theta, kappa1=lp.kappa1, kappa2=lp.kappa2,
                               beta=lp.beta - 0.02 * j, volvol=lp.volvol * (1 - 0.01 * j)) for j in range(n_jobs)]
    return [sv.HestonParams(v0=0.04 * (1 + 0.05 * j), theta=0.04, kappa=4.0, rho=-0.5, volvol=0.4 * (1 + 0.02 * j))
            for j in range(n_jobs)]


def runners(model: str, ps, seeds, nb_path, ch):
    if model == "logsv":
        def one(p, s):
            return sv.logsv_mc_chain_pricer(v0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2, beta=p.beta,
                                            volvol=p.volvol, vol_backbone_etas=p.get_vol_backbone_etas(ttms=ch["ttms"]),
                                            nb_path=nb_path, nb_steps_per_year=SPY, seed=s, **ch)

        def batch():
            return sv.logsv_mc_chain_pricer_many(ps, nb_path=nb_path, nb_steps_per_year=SPY, seeds=seeds, **ch)
    else:
        scheme = "qe" if model == "heston_qe" else "euler"

        def one(p, s):
            return sv.heston_mc_chain_pricer(v0=p.v0, theta=p.theta, kappa=p.kappa, rho=p.rho, volvol=p.volvol, nb_path=nb_path,
                                             nb_steps_per_year=SPY, scheme=scheme, seed=s, **ch)

        def batch():
            return sv.heston_mc_chain_pricer_many(ps, nb_path=nb_path, nb_steps_per_year=SPY, scheme=scheme, seeds=seeds, **ch)

    def loop():
        return [one(p, s) for p, s in zip(ps, seeds)]
    return batch, loop


def timed(fn) -> float:
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def same_bits(a, b) -> bool:
    return len(a) == len(b) and all(np.array_equal(x, y) for (pa, ea), (pb, eb) in zip(a, b) for x, y in zip(pa + ea, pb + eb))


def case(model, n_jobs, nb_path, passes, reps, ch, L):
    ps = jobs(model, n_jobs)
    seeds = [1000 + j for j in range(n_jobs)]
    batch, loop = runners(model, ps, seeds, nb_path, ch)
    ok = same_bits(batch(), loop())
    for _ in range(3):
        batch()
        loop()
    tb, tl = [], []
    for q in range(passes):
        order = (batch, loop) if q % 2 == 0 else (loop, batch)
        for fn in order:
            (tb if fn is batch else tl).extend(timed(fn) for _ in range(reps))
    # the batch's stepping time (session events) and its stepping launch's shader clock (in-kernel probe)
    eng = get_engine(nb_path)
    sess = eng.fused_chain_session(len(ch["ttms"]), sum(np.size(k) for k in ch["strikes_ttms"]))
    _lib.check(L.svmc_session_time_stepping(sess, 1))
    steps_ms = []
    for _ in range(reps):
        batch()
        ms = C.c_float()
        _lib.check(L.svmc_session_last_stepping_ms(sess, C.byref(ms)))
        steps_ms.append(float(ms.value))
    _lib.check(L.svmc_session_time_stepping(sess, 0))
    clock_mhz = None
    if model == "logsv":
        _lib.check(L.svmc_clock_probe_arm(1))
        try:
            batch()
            st = (C.c_uint64 * 8)()
            _lib.check(L.svmc_clock_probe_read(st, eng.stream))
            dt, dr = st[2] - st[0], st[3] - st[1]
            clock_mhz = round(dt / dr * 100.0, 1) if dr > 0 else None
        finally:
            _lib.check(L.svmc_clock_probe_arm(0))
    work = n_jobs * nb_path * total_steps(ch["ttms"])
    mb, ml, ms = statistics.median(tb), statistics.median(tl), statistics.median(steps_ms)
    return {"model": model, "n_jobs": n_jobs, "nb_path": nb_path, "batch_ms": round(mb, 4), "loop_ms": round(ml, 4),
            "speedup": round(ml / mb, 3), "batch_path_steps_per_s": float(f"{work / (mb * 1e-3):.4g}"),
            "loop_path_steps_per_s": float(f"{work / (ml * 1e-3):.4g}"), "batch_stepping_ms": round(ms, 4),
            "batch_rest_ms": round(mb - ms, 4), "stepping_path_steps_per_s": float(f"{work / (ms * 1e-3):.4g}"),
            "kernel_clock_mhz": clock_mhz, "same_bits": bool(ok), "samples": len(tb)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_many_bench.json"))
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="J in {1, 5}, 10^5 paths, LogSV only")
    ap.add_argument("--models", default="logsv,heston_euler,heston_qe")
    a = ap.parse_args()
    L = _lib.load()
    ch = chain_4x13()
    ch["optiontypes_ttms"] = [np.asarray(t) for t in ch["optiontypes_ttms"]]
    assert all(option_type_codes(t).size == 13 for t in ch["optiontypes_ttms"])
    models = ["logsv"] if a.quick else a.models.split(",")
    js = (1, 5) if a.quick else (1, 2, 4, 5, 8, 16)
    paths = (100_000,) if a.quick else (100_000, 400_000)
    rows = []
    for model in models:
        for nb_path in paths:
            for n_jobs in js:
                r = case(model, n_jobs, nb_path, a.passes, a.reps, ch, L)
                rows.append(r)
                print(json.dumps(r), flush=True)
    name = ""
    info = C.create_string_buffer(256)
    if L.svmc_device_info(0, info, 256, None, None, None) == 0:
        name = info.value.decode(errors="replace")
    out = {"what": "many jobs of one chain per call vs a loop of single calls (tools/bench_mc_many.py)", "device": name,
           "chain": "4 x 13 (ttms 1/12, 1/4, 1/2, 1; strikes 0.7-1.3), 360 steps/yr", "total_steps": total_steps(ch["ttms"]),
           "passes": a.passes, "reps": a.reps, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
