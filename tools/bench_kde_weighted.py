"""
Times of the weighted kernel density estimates on the GPU -> profiles/kde_weighted_bench.json, by the method
of tools/bench_kde.py: the six launches of ONE vector (the simulated log-return x of the TEST set) on 200 resident points at 10^5,
4 x 10^5 and 2^22 paths, queued on resident buffers and ended by one synchronise --

  * unweighted          svmc_kde_gaussian, the launches of row f7 in the same build;
  * weighted, no vector svmc_kde_gaussian_weighted with weights = tilt = NULL (the same bits as the unweighted);
  * weights             a resident vector of uniform weights;
  * tilt                exp(gamma x) of the resident x at gamma = 1;

each with its ratio to the unweighted launches, and on the same box and sample scipy.stats.gaussian_kde(x, weights=exp(x)) on one
host core at the first two sizes (--scipy-repeats runs; seconds each).  Host clocks around work that ends in a synchronise;
medians of --repeats runs after a warm-up.

    python tools/bench_kde_weighted.py [--repeats 10] [--scipy-repeats 3] [--out profiles/kde_weighted_bench.json]
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

from bench_kde import TEST, TTM, median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--scipy-repeats", type=int, default=3)
    ap.add_argument("--paths", type=int, nargs="*", default=[100_000, 400_000, 1 << 22])
    ap.add_argument("--points", type=int, default=200)
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kde_weighted_bench.json"))
    args = ap.parse_args()
    L = _lib.load()
    pricer = sv.LogSVPricer()
    grid = np.ascontiguousarray(TEST.get_variable_space_grid(variable_type=sv.VariableType.LOG_RETURN, ttm=TTM, n=args.points, n_stdevs=4.5))
    m = grid.size
    out = {"repeats": args.repeats, "scipy_repeats": args.scipy_repeats, "ttm": TTM, "n_points": m, "gamma": args.gamma,
           "device_runs": [], "same_box": []}
    for n in args.paths:
        pricer.terminal_value_kdes(params=TEST, ttm=TTM, nb_path=n, seed=1)              # leaves the terminal state on the engine
        eng = get_engine(n)
        weights = np.random.default_rng(1).random(n)
        ws_plain, ws_weighted = analytic.kde_workspace(n)[0], analytic.kde_weighted_workspace(n)[0]
        bufs = [DeviceBuffer(m), DeviceBuffer(m + analytic.KDE_WEIGHTED_STATS_DOUBLES), DeviceBuffer(ws_weighted // 8), DeviceBuffer(n)]
        gb, rb, wsb, wb = bufs
        try:
            _lib.check(L.svmc_memcpy_h2d(gb.ptr, grid.ctypes.data, grid.nbytes, eng.stream))
            _lib.check(L.svmc_memcpy_h2d(wb.ptr, weights.ctypes.data, weights.nbytes, eng.stream))
            _lib.check(L.svmc_stream_synchronize(eng.stream))

            def plain():
                _lib.check(L.svmc_kde_gaussian(eng.x.ptr, n, 1.0, 1e16, gb.ptr, m, 0.0, rb.ptr, rb.offset(m), wsb.ptr, ws_plain, eng.stream))
                _lib.check(L.svmc_stream_synchronize(eng.stream))

            def weighted(w_ptr, t_ptr):
                def run():
                    _lib.check(L.svmc_kde_gaussian_weighted(eng.x.ptr, w_ptr, t_ptr, args.gamma, n, 1.0, 1e16, gb.ptr, m, 0.0, rb.ptr,
                                                            rb.offset(m), wsb.ptr, ws_weighted, eng.stream))
                    _lib.check(L.svmc_stream_synchronize(eng.stream))
                return run

            ms = {"unweighted": median_ms(plain, args.repeats), "weighted_no_vector": median_ms(weighted(None, None), args.repeats),
                  "weights": median_ms(weighted(wb.ptr, None), args.repeats), "tilt": median_ms(weighted(None, eng.x.ptr), args.repeats)}
        finally:
            for b in bufs:
                b.free()
        row = {"n_path": n, "n_points": m, "chunk_length": analytic.kde_weighted_workspace(n)[1], "exp_evaluations_of_the_density": n * m}
        for k, v in ms.items():
            row[k + "_launches_ms"] = v
            row[k + "_ratio_to_unweighted"] = v / ms["unweighted"]
        print(json.dumps(row), flush=True)
        out["device_runs"].append(row)
        if n <= 400_000 and args.scipy_repeats > 0:
            from scipy.stats import gaussian_kde
            x = eng.get_state()[0]
            ts = []
            for _ in range(args.scipy_repeats):
                t0 = time.perf_counter()
                gaussian_kde(x, weights=np.exp(args.gamma * x))(grid)
                ts.append(time.perf_counter() - t0)
            row = {"n_path": n, "scipy_weighted_gaussian_kde_one_variable_s": statistics.median(ts)}
            print(json.dumps(row), flush=True)
            out["same_box"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
