"""
Times of the density row on the GPU -> profiles/densities_bench.json:

  * logsv_pdfs per call for the three variables at 200 and 2 001 space points, split into the ODE launch (queue + wait) and the
    inversion (upload of the space grid, launch, download of the masses and the log-MGF);
  * the six calls of one density figure (three variables x two expansion orders) as single calls and through logsv_pdfs_batch;
  * terminal_value_histograms' counting against downloading the three state vectors, at 400 000 and 2^22 paths;
  * exp evaluations per second of mgf_pdf_slice_kernel against mgf_vanilla_slice_kernel (and mgf_digital_slice_kernel,
    mgf_qvar_slice_kernel) on the same 1000-point grid and the same number of blocks (32), by device events around 200 queued
    launches of each.

Host clocks around work that ends in a synchronise; medians of --repeats runs after a warm-up.  The reference's CPU seconds
come from the fixture (timed when it was generated; the reference never runs on the GPU machine).

    python tools/bench_densities.py [--repeats 20] [--out profiles/densities_bench.json]
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
from stochvolmodels_amd.pricers import logsv_pricer as lp  # noqa: E402

TEST = sv.LogSvParams(sigma0=0.2, theta=0.22, kappa1=3.0, kappa2=12.0, beta=-0.3, volvol=0.4)
TTM = 0.25
VARS = {"LOG_RETURN": sv.VariableType.LOG_RETURN, "Q_VAR": sv.VariableType.Q_VAR, "SIGMA": sv.VariableType.SIGMA}


def median_ms(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def split_call(vt, space, repeats):
    """(ODE ms, inversion ms) of one second-order logsv_pdfs case, on a pooled grid as the pricer uses it"""
    L = _lib.load()
    phi, psi, a_t0, var, resident, shift, scale = lp._pdf_setup(TEST, TTM, True, 2, vt, None)
    ode, inv = [], []
    for i in range(repeats + 1):
        grid = AnalyticGrid.acquire(phi, psi, 5)
        try:
            if np.any(a_t0):
                grid.set_a(a_t0[None])
            _lib.check(L.svmc_stream_synchronize(None))
            t0 = time.perf_counter()
            grid.logsv_advance(TTM, [[TEST.sigma0, TEST.theta, TEST.kappa1, TEST.kappa2, TEST.beta, TEST.volvol, 1.0, 0.0]], True, 2)
            _lib.check(L.svmc_stream_synchronize(None))
            t1 = time.perf_counter()
            grid.pdf_sums([var], [space], [shift], [scale], resident=resident)
            t2 = time.perf_counter()
        finally:
            grid.release()
        if i:
            ode.append((t1 - t0) * 1e3)
            inv.append((t2 - t1) * 1e3)
    return statistics.median(ode), statistics.median(inv)


def kernel_rates(repeats=200):
    L = _lib.load()
    from stochvolmodels_amd.utils.mgf_pricer import get_phi_grid
    phi = get_phi_grid(vol_scaler=0.04)
    lm = 0.5 * 0.0225 * (phi + phi * phi)
    space = np.linspace(-0.5, 0.4, 32)
    strikes = np.exp(-space)
    bufs = [DeviceBuffer(2 * phi.size), DeviceBuffer(2 * phi.size), DeviceBuffer(32), DeviceBuffer(32)]
    for b, z in zip(bufs[:3], (phi, lm, space)):
        _lib.check(L.svmc_memcpy_h2d(b.ptr, np.ascontiguousarray(z).ctypes.data, z.nbytes, None))
    _lib.check(L.svmc_stream_synchronize(None))
    pf = C.POINTER(C.c_double)
    one, zero = np.array([1.0]), np.array([0.0])

    def pdf():
        _lib.check(L.svmc_mgf_pdf_slice_batch(bufs[0].ptr, bufs[1].ptr, phi.size, 1, bufs[2].ptr, 32, zero.ctypes.data_as(pf),
                                              one.ctypes.data_as(pf), 1, bufs[3].ptr, None))

    def vanilla():
        _lib.check(L.svmc_mgf_vanilla_slice(bufs[0].ptr, bufs[1].ptr, phi.size, 1.0, strikes.ctypes.data_as(pf), 32, bufs[3].ptr, None))

    def digital():
        _lib.check(L.svmc_mgf_digital_slice_batch(bufs[0].ptr, bufs[1].ptr, phi.size, 1, 1.0, strikes.ctypes.data_as(pf), 32, 1, 1,
                                                  bufs[3].ptr, None))

    def qvar():                                              # the phi grid standing in for psi: the same 32 x 1000 terms
        _lib.check(L.svmc_mgf_qvar_slice(bufs[0].ptr, bufs[1].ptr, phi.size, 1.0, strikes.ctypes.data_as(pf), 32, bufs[3].ptr, None))

    out = {}
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _lib.check(L.svmc_event_create(C.byref(e)))
    for _ in range(3):                                       # alternate the kernels: other work shares the machine
        for name, fn in (("mgf_pdf_slice_kernel", pdf), ("mgf_vanilla_slice_kernel", vanilla),
                         ("mgf_digital_slice_kernel", digital), ("mgf_qvar_slice_kernel", qvar)):
            fn()
            _lib.check(L.svmc_event_record(ev[0], None))
            for _ in range(repeats):
                fn()
            _lib.check(L.svmc_event_record(ev[1], None))
            ms = C.c_float()
            _lib.check(L.svmc_event_elapsed_ms(ev[0], ev[1], C.byref(ms)))
            out.setdefault(name, []).append(ms.value / repeats)
    for e in ev:
        _lib.check(L.svmc_event_destroy(e))
    for b in bufs:
        b.free()
    terms = 32 * phi.size
    return {k: {"us_per_launch_back_to_back": statistics.median(v) * 1e3, "blocks": 32, "grid_points": int(phi.size),
                "exp_evaluations_per_s": terms / (statistics.median(v) * 1e-3)} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densities_bench.json"))
    args = ap.parse_args()
    res = {"params": "TEST set (sigma0 .2, theta .22, kappa1 3, kappa2 12, beta -.3, volvol .4), ttm 0.25, second order",
           "repeats": args.repeats, "logsv_pdfs_ms": {}, "figure_six_calls_ms": {}, "histograms": {}}
    for vname, vt in VARS.items():
        for n in (200, 2001):
            space = TEST.get_variable_space_grid(variable_type=vt, ttm=TTM, n=n, n_stdevs=4.5)
            total = median_ms(lambda: sv.logsv_pdfs(params=TEST, ttm=TTM, space_grid=space, variable_type=vt), args.repeats)
            ode, inv = split_call(vt, space, args.repeats)
            res["logsv_pdfs_ms"][f"{vname}_{n}"] = {"call": total, "ode_launch": ode, "inversion": inv}
            print(vname, n, res["logsv_pdfs_ms"][f"{vname}_{n}"], flush=True)
        space = TEST.get_variable_space_grid(variable_type=vt, ttm=TTM, n=200, n_stdevs=4.5)
        orders = [sv.ExpansionOrder.FIRST, sv.ExpansionOrder.SECOND]
        res["figure_six_calls_ms"][vname] = {
            "two_single_calls": median_ms(lambda: [sv.logsv_pdfs(params=TEST, ttm=TTM, space_grid=space, variable_type=vt,
                                                                 expansion_order=o) for o in orders], args.repeats),
            "logsv_pdfs_batch": median_ms(lambda: sv.logsv_pdfs_batch([TEST, TEST], TTM, [space, space], expansion_orders=orders,
                                                                      variable_type=vt), args.repeats)}
        print(vname, res["figure_six_calls_ms"][vname], flush=True)
    for k in ("two_single_calls", "logsv_pdfs_batch"):
        res["figure_six_calls_ms"]["all_three_variables_" + k] = sum(res["figure_six_calls_ms"][v][k] for v in VARS)
    pricer = sv.LogSVPricer()
    for n in (400_000, 1 << 22):
        grids = {vt: TEST.get_variable_space_grid(variable_type=vt, ttm=TTM, n=200, n_stdevs=4.5) for vt in VARS.values()}
        pricer.terminal_value_histograms(params=TEST, ttm=TTM, nb_path=n, seed=1, space_grids=grids)
        eng = get_engine(n)
        res["histograms"][str(n)] = {
            "three_device_histograms_ms": median_ms(lambda: lp.engine_state_histograms(eng, grids, TTM), args.repeats),
            "download_three_state_vectors_ms": median_ms(eng.get_state, max(3, args.repeats // 4)),
            "bytes_downloaded": {"histograms": 3 * 8 * 199, "state": 3 * 8 * n}}
        print(n, res["histograms"][str(n)], flush=True)
    res["inversion_kernel_rate"] = kernel_rates()
    print(res["inversion_kernel_rate"], flush=True)
    fx_path = os.path.join(ROOT, "tests", "golden", "densities.npz")
    if os.path.exists(fx_path):
        fx = np.load(fx_path)
        res["reference_cpu_s"] = {"LOG_RETURN_200": float(fx["ref_seconds_x"]), "SIGMA_200": float(fx["ref_seconds_sigma"]),
                                  "Q_VAR_200": float(fx["ref_seconds_qvar"]), "machine": str(fx["ref_cpu"]),
                                  "how": "the unmodified reference's logsv_pdfs at its default solver settings, one process, "
                                         "NumPy-mode stand-in for numba, timed by tests/golden/make_golden_densities.py"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
