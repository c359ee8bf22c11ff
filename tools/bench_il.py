"""
Times of the impermanent-loss row on the GPU -> profiles/il_bench.json:

  * logsv_il_pricer_vector per call for a profile of 1, 101 and 1 001 forwards (the script's parameter set, ttm 10/365), split
    into the ODE launch and the slice launch with its download, against the reference's seconds per call from the fixture (its
    np.vectorize form pays them once per forward);
  * mgf_il_slice_kernel alone at 256 cases x 1 001 points by device events around back-to-back launches, beside
    mgf_digital_slice_kernel at 256 strikes: what the five passes cost against one;
  * model_mc_il_payoff's reduction (svmc_il_payoff on the resident state) at 400 000 paths for 1, 101 and 1 001 forwards.

Medians of --repeats runs (default 10) after a warm-up, host clock around work that ends in a synchronise.

    python tools/bench_il.py [--repeats 10] [--out profiles/il_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import stochvolmodels_amd as sv  # noqa: E402
from stochvolmodels_amd import _lib  # noqa: E402
from stochvolmodels_amd.analytic import AnalyticGrid  # noqa: E402
from stochvolmodels_amd.engine import DeviceBuffer, get_engine  # noqa: E402
from stochvolmodels_amd.pricers import il_pricer as ilp  # noqa: E402
from stochvolmodels_amd.utils import mgf_pricer as mgfp  # noqa: E402

PARAMS = sv.LogSvParams(sigma0=0.4861785891939535, theta=0.6176006871606874, kappa1=1.955809653686808, kappa2=1.978367101612294,
                        beta=-0.26916969112829325, volvol=3.265815229306317)
TTM, P0, PA, PB = 10.0 / 365.0, 2200.0, 2000.0, 2400.0


def median_ms(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def split_call(forwards, repeats):
    """(ODE ms, slice launch + download ms) of one profile on a pooled grid, as the pricer runs it"""
    L = _lib.load()
    cases, _ = ilp.il_cases(forwards, P0, PA, PB)
    vs = PARAMS.sigma0 * np.sqrt(np.minimum(TTM, 0.5 / 12.0))
    phi, psi, _ = mgfp.get_transform_var_grid(vol_scaler=vs, real_phi=ilp.IL_REAL_PHI, max_phi=ilp.IL_MAX_PHI)
    rows = [[PARAMS.sigma0, PARAMS.theta, PARAMS.kappa1, PARAMS.kappa2, PARAMS.beta, PARAMS.volvol, 1.0, 0.0]]
    ode, inv = [], []
    for i in range(repeats + 1):
        grid = AnalyticGrid.acquire([phi], [psi], 5)
        try:
            _lib.check(L.svmc_stream_synchronize(None))
            t0 = time.perf_counter()
            grid.logsv_advance(TTM, rows, True, 2)
            _lib.check(L.svmc_stream_synchronize(None))
            t1 = time.perf_counter()
            n_out = cases.shape[0] * ilp.IL_SLICE_SUMS
            grid.reserve_results(n_out)
            ilp._slice_launch(L, grid.phi.ptr, grid.log_mgf.ptr, grid.n, 1, cases, True, grid._capped.ptr)
            grid.download_results(n_out)
            t2 = time.perf_counter()
        finally:
            grid.release()
        if i:
            ode.append((t1 - t0) * 1e3)
            inv.append((t2 - t1) * 1e3)
    return statistics.median(ode), statistics.median(inv)


def kernel_times(n_cases=256, repeats=100):
    """us per call of the IL slice entry (8 launches of 32 cases, five passes each) and of the digital entry at as many strikes"""
    L = _lib.load()
    vs = PARAMS.sigma0 * np.sqrt(TTM)
    phi, _, _ = mgfp.get_transform_var_grid(vol_scaler=vs, real_phi=ilp.IL_REAL_PHI, max_phi=ilp.IL_MAX_PHI)
    lm = 0.5 * (PARAMS.sigma0 ** 2 * TTM) * (phi + phi * phi)
    forwards = np.linspace(1800.0, 2600.0, n_cases)
    cases, _ = ilp.il_cases(forwards, P0, PA, PB)
    bufs = [DeviceBuffer(2 * phi.size), DeviceBuffer(2 * phi.size), DeviceBuffer(5 * n_cases)]
    for b, z in zip(bufs[:2], (phi, lm)):
        _lib.check(L.svmc_memcpy_h2d(b.ptr, np.ascontiguousarray(z).ctypes.data, z.nbytes, None))
    _lib.check(L.svmc_stream_synchronize(None))
    pf = C.POINTER(C.c_double)

    def il():
        ilp._slice_launch(L, bufs[0].ptr, bufs[1].ptr, phi.size, 1, cases, True, bufs[2].ptr)

    def digital():
        _lib.check(L.svmc_mgf_digital_slice_batch(bufs[0].ptr, bufs[1].ptr, phi.size, 1, P0, forwards.ctypes.data_as(pf), n_cases, 1, 1,
                                                  bufs[2].ptr, None))

    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _lib.check(L.svmc_event_create(C.byref(e)))
    out = {}
    for _ in range(3):
        for name, fn in (("svmc_mgf_il_slice_batch", il), ("svmc_mgf_digital_slice_batch", digital)):
            fn()
            _lib.check(L.svmc_event_record(ev[0], None))
            for _ in range(repeats):
                fn()
            _lib.check(L.svmc_event_record(ev[1], None))
            _lib.check(L.svmc_event_synchronize(ev[1]))
            ms = C.c_float()
            _lib.check(L.svmc_event_elapsed_ms(ev[0], ev[1], C.byref(ms)))
            out.setdefault(name, []).append(ms.value / repeats)
    for e in ev:
        _lib.check(L.svmc_event_destroy(e))
    for b in bufs:
        b.free()
    return {k: {"us_per_call_back_to_back": statistics.median(v) * 1e3, "cases_or_strikes": n_cases, "grid_points": int(phi.size),
                "launches_per_call": (n_cases + 31) // 32} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "il_bench.json"))
    args = ap.parse_args()
    res = {"params": "the parameter set of the reference's IL script, ttm 10/365, p0 2200, range [2000, 2400], second order",
           "repeats": args.repeats, "logsv_il_pricer_vector_ms": {}, "svmc_il_payoff_ms": {}}
    for n in (1, 101, 1001):
        forwards = np.linspace(1800.0, 2600.0, n) if n > 1 else np.array([2200.0])
        call = median_ms(lambda: sv.logsv_il_pricer_vector(PARAMS, TTM, forwards, P0, PA, PB), args.repeats)
        ode, inv = split_call(forwards, args.repeats)
        res["logsv_il_pricer_vector_ms"][str(n)] = {"call": call, "ode_launch": ode, "slice_launches_and_download": inv}
        print(n, res["logsv_il_pricer_vector_ms"][str(n)], flush=True)
    res["slice_entry_points"] = kernel_times()
    print(res["slice_entry_points"], flush=True)
    n_path = 400_000
    sv.LogSVPricer().model_mc_il_payoff(PARAMS, TTM, 2200.0, P0, PA, PB, nb_path=n_path, seed=1)
    eng = get_engine(n_path)
    for n in (1, 101, 1001):
        forwards = np.linspace(1800.0, 2600.0, n) if n > 1 else np.array([2200.0])
        res["svmc_il_payoff_ms"][str(n)] = median_ms(lambda: eng.il_payoffs(forwards, P0, PA, PB), args.repeats)
    res["svmc_il_payoff_ms"]["paths"] = n_path
    print(res["svmc_il_payoff_ms"], flush=True)
    fx_path = os.path.join(ROOT, "tests", "golden", "il_payoff.npz")
    if os.path.exists(fx_path):
        fx = np.load(fx_path)
        s = float(fx["ref_seconds"])
        res["reference_cpu_s"] = {"per_call": s, "profile_of_101_forwards": 101 * s, "profile_of_1001_forwards": 1001 * s,
                                  "machine": str(fx["ref_cpu"]),
                                  "how": "one call of the unmodified reference's logsv_il_pricer at its default solver settings, one "
                                         "process, NumPy-mode stand-in for numba, timed by tests/golden/make_golden_il_payoff.py; its "
                                         "logsv_il_pricer_vector is np.vectorize and pays this once per forward"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
