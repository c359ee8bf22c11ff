"""
Times of the kernel density estimates on the GPU -> profiles/kde_bench.json:

  * LogSVPricer.terminal_value_kdes of the three variables at 10^5, 4 x 10^5 and 2^22 paths on 200 and 2 001 points: the whole call
    (simulation included), engine_state_kdes alone (upload of the grids, 3 x 6 launches, one download) and the 18 launches alone
    (queued on resident grids and results, then one synchronise), with the exponentials per second of the launches;
  * on the same box and the same sample: the download of the three state vectors, and scipy.stats.gaussian_kde of x on one host
    core at 10^5 x 200 and 4 x 10^5 x 200 (--scipy-repeats runs; seconds each).

Host clocks around work that ends in a synchronise; medians of --repeats runs after a warm-up.

    python tools/bench_kde.py [--repeats 10] [--scipy-repeats 3] [--out profiles/kde_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import stochvolmodels_amd as sv  # noqa: E402
from stochvolmodels_amd import _lib, analytic  # noqa: E402
from stochvolmodels_amd.engine import DeviceBuffer, get_engine  # noqa: E402
from stochvolmodels_amd.pricers import logsv_pricer as lp  # noqa: E402

TEST = sv.LogSvParams(sigma0=0.2, theta=0.22, kappa1=3.0, kappa2=12.0, beta=-0.3, volvol=0.4)
TTM = 0.25
VTS = (sv.VariableType.LOG_RETURN, sv.VariableType.Q_VAR, sv.VariableType.SIGMA)
PDF_SLICE_EXP_PER_S = 2.0e11          # mgf_pdf_slice_kernel, profiles/densities_bench.json


def median_ms(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def launches_only(eng, grids, ttm):
    """a closure queueing the 3 x 6 launches on resident grids, results and workspace and waiting for them: no copies, no allocation"""
    L = _lib.load()
    src = [(eng.x.ptr, 1.0), (eng.qvar.ptr, float(ttm)), (eng.vol.ptr, 1.0)]
    hosts = [np.ascontiguousarray(grids[vt], dtype=np.float64) for vt in VTS]
    ws_bytes = analytic.kde_workspace(eng.n_path)[0]
    bufs = [DeviceBuffer(g.size) for g in hosts] + [DeviceBuffer(g.size + analytic.KDE_STATS_DOUBLES) for g in hosts] + [DeviceBuffer(ws_bytes // 8)]
    for b, g in zip(bufs[:3], hosts):
        _lib.check(L.svmc_memcpy_h2d(b.ptr, g.ctypes.data, g.nbytes, eng.stream))
    _lib.check(L.svmc_stream_synchronize(eng.stream))

    def run():
        for (ptr, div), gb, rb, g in zip(src, bufs[:3], bufs[3:6], hosts):
            _lib.check(L.svmc_kde_gaussian(ptr, eng.n_path, div, 1e16, gb.ptr, g.size, 0.0, rb.ptr, rb.offset(g.size), bufs[6].ptr,
                                           ws_bytes, eng.stream))
        _lib.check(L.svmc_stream_synchronize(eng.stream))

    return run, bufs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--scipy-repeats", type=int, default=3)
    ap.add_argument("--paths", type=int, nargs="*", default=[100_000, 400_000, 1 << 22])
    ap.add_argument("--points", type=int, nargs="*", default=[200, 2001])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kde_bench.json"))
    args = ap.parse_args()
    pricer = sv.LogSVPricer()
    out = {"repeats": args.repeats, "scipy_repeats": args.scipy_repeats, "ttm": TTM,
           "pdf_slice_kernel_exp_per_s": PDF_SLICE_EXP_PER_S, "device_runs": [], "same_box": []}
    for n in args.paths:
        for m in args.points:
            grids = {vt: TEST.get_variable_space_grid(variable_type=vt, ttm=TTM, n=m, n_stdevs=4.5) for vt in VTS}
            whole = median_ms(lambda: pricer.terminal_value_kdes(params=TEST, ttm=TTM, nb_path=n, seed=1, space_grids=grids), args.repeats)
            eng = get_engine(n)
            state = median_ms(lambda: lp.engine_state_kdes(eng, grids, TTM), args.repeats)
            run, bufs = launches_only(eng, grids, TTM)
            try:
                launches = median_ms(run, args.repeats)
            finally:
                for b in bufs:
                    b.free()
            n_exp = 3 * n * m
            row = {"n_path": n, "n_points": m, "chunk_length": analytic.kde_workspace(n)[1], "terminal_value_kdes_ms": whole,
                   "engine_state_kdes_ms": state, "kde_launches_ms": launches, "exp_evaluations": n_exp,
                   "exp_per_s_of_the_launches": n_exp / (launches * 1e-3)}
            print(json.dumps(row), flush=True)
            out["device_runs"].append(row)
    from scipy.stats import gaussian_kde
    for n in args.paths:
        pricer.terminal_value_kdes(params=TEST, ttm=TTM, nb_path=n, seed=1)
        eng = get_engine(n)
        row = {"n_path": n, "download_three_state_vectors_ms": median_ms(eng.get_state, args.repeats)}
        if n <= 400_000 and args.scipy_repeats > 0:
            x = eng.get_state()[0]
            grid = TEST.get_variable_space_grid(variable_type=sv.VariableType.LOG_RETURN, ttm=TTM, n=200, n_stdevs=4.5)
            ts = []
            for _ in range(args.scipy_repeats):
                t0 = time.perf_counter()
                gaussian_kde(x)(grid)
                ts.append(time.perf_counter() - t0)
            row["scipy_gaussian_kde_one_variable_200_points_s"] = statistics.median(ts)
        print(json.dumps(row), flush=True)
        out["same_box"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
