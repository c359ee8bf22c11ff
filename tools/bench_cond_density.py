#!/usr/bin/env python
"""
Measurement of the mixture density of the simulated log-return (libsvmc_est.so's cond_density_*_kernel) in the
settings of row f18's density table: the Hawkes jump-diffusion at default HawkesJDParams, one month, 200 points on [-0.6, 0.6], at
10^5 and 2^20 paths, for 1 gamma (-1), 5 gammas (-3, -1, 0, 0.5, 3) and 16 gammas (-3 .. 3).  Medians of --reps (10) calls after 3
warm-up calls, the host clock around a call that returns synchronised.  Row f18's routes and the weighted KDE are the parent commit's
code, untouched: their times are measured here, in the same process.  Writes ONE JSON object to --out (default
profiles/cond_density_bench.json) and prints it:

  mc[n][G].mixture_tail_ms       engine.conditional_densities alone on resident rows (svmc_cond_density_chain: three launches)
  mc[n][G].greeks_tail_ms        engine.tilted_conditional_greeks alone on the same rows at K = exp(x): the tail of row f18's density
  mc[n][G].mixture_call_ms       HawkesJDPricer.get_log_return_mc_pdf_mixture: the stepping call and the tail
  mc[n][G].greeks_route_call_ms  HawkesJDPricer.get_log_return_mc_pdf_conditional_under_risk_kernel: the stepping call and two tails
  mc[n][G].weighted_kde_call_ms  HawkesJDPricer.get_log_return_mc_pdf_device(risk_premia_gamma=): its own stepping call and the KDE
  mc[n][G].exp_per_s             n x 200 x ceil(G / GT) exponentials of the main kernel over the WHOLE tail's time (the weight pass, the
                                 finish, the upload and the download included: a lower bound of the kernel's own rate)
  mc[n][G].tail_vs_greeks_tail, call_vs_greeks_route, call_vs_weighted_kde   the ratios
  kde_exp_per_s                  profiles/kde_bench.json's exp_per_s_of_the_launches at (100 000 paths, 200 points), to set beside it
  main_kernels                   the two instances of the main kernel (the tile of calls of up to GT gammas, the tile of larger calls) with
                                 VGPRs and waves per SIMD; mc[n][G].GT: the tile that call ran
  variants[XT,GT,weights][n][G]  the tail with SVMC_CD_XT points per thread and ONE tile of SVMC_CD_GT gammas, each build loaded by a process
                                 of its own through SVMC_EST_LIB, with the main kernel's metadata (VGPRs; waves per SIMD = 512 // VGPRs,
                                 at most 8).  --variant-lib XT,GT,LABEL=FILE takes a prebuilt library (LABEL "pass": the weights from the
                                 pre-pass's rows, as built; any other label names a build this source no longer produces); without any,
                                 the (XT, GT) pairs of VARIANTS are compiled into a temporary directory.

    python tools/bench_cond_density.py [--reps 10] [--variant-lib 4,4,pass=FILE ...] [--no-variants] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (100000, 1 << 20)
GAMMA_SETS = ([-1.0], [-3.0, -1.0, 0.0, 0.5, 3.0], [float(g) for g in np.linspace(-3.0, 3.0, 16)])
VARIANTS = ((2, 4), (4, 2), (4, 4), (8, 4), (4, 8), (8, 8), (2, 16), (4, 16))
TTM, X = 1.0 / 12.0, np.linspace(-0.6, 0.6, 200)


def median_ms(call, reps):
    for _ in range(3):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(wall))


def main_kernels(lib_isa_json=None):
    """[(XT, GT, metadata with waves per SIMD)] of a build's main kernels, narrow tile first, read off their mangled names:
    cond_density_kernelILi<XT>ELi<GT>EE.  A call of up to the narrow GT gammas runs the first, any other the last."""
    import re
    from stochvolmodels_amd import build as svbuild
    meta = json.load(open(lib_isa_json or svbuild.EST_ISA_JSON))["metadata"]
    out = []
    for name, m in meta.items():
        hit = re.search(r"cond_density_kernelILi(\d+)ELi(\d+)E", name)
        if hit:
            out.append((int(hit.group(1)), int(hit.group(2)), dict(m, waves_per_simd=min(512 // m["vgpr"], 8))))
    return sorted(out, key=lambda k: k[1])


def tile_of(kernels, n_gammas):
    return kernels[0][1] if n_gammas <= kernels[0][1] else kernels[-1][1]


def step_rows(n):
    """the rows one mixture call leaves on the engine: mu in snapshot row 0, cv in row 1"""
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.engine import get_engine
    sv.HawkesJDPricer().get_log_return_mc_pdf_mixture(sv.HawkesJDParams(), TTM, X[:4], nb_path=n, seed=1)
    return get_engine(n)


def tail_times(reps):
    """{n: {G: ms}} of the mixture tail alone with the library _lib.load_est() finds"""
    out = {}
    for n in SIZES:
        eng = step_rows(n)
        out[str(n)] = {str(len(g)): median_ms(lambda: eng.conditional_densities([X], g, mu_rows=[0], cv_rows=[1]), reps) for g in GAMMA_SETS}
    return out


def variant_comparison(libs, reps):
    from stochvolmodels_amd import build as svbuild
    out = {}
    with tempfile.TemporaryDirectory(prefix="svmc_cd_variants_") as tmp:
        if not libs:
            for xt, gt in VARIANTS:
                lib = os.path.join(tmp, f"libsvmc_est_x{xt}_g{gt}.so")
                svbuild.build_side(lib, lib + ".isa.json", svbuild.EST_SRC, False,
                                   extra=(f"-DSVMC_CD_XT={xt}", f"-DSVMC_CD_GT={gt}", f"-DSVMC_CD_GT_WIDE={gt}"))      # one tile for every count
                libs.append((f"{xt},{gt},pass", lib))
        for label, lib in libs:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--tail-only", "--reps", str(reps)],
                                 env=dict(os.environ, SVMC_EST_LIB=os.path.abspath(lib)), capture_output=True, text=True, timeout=300)
            if res.returncode != 0:
                raise RuntimeError(f"{label}: {res.stdout}{res.stderr}")
            out[label] = json.loads(res.stdout.strip().splitlines()[-1])
            if os.path.exists(lib + ".isa.json"):
                out[label]["kernel"] = main_kernels(lib + ".isa.json")[0][2]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--variant-lib", action="append", default=[], help="XT,GT,LABEL=FILE: a prebuilt libsvmc_est.so")
    ap.add_argument("--no-variants", action="store_true")
    ap.add_argument("--tail-only", action="store_true", help="print the mixture tail's times of the loaded library and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cond_density_bench.json"))
    a = ap.parse_args()
    if a.tail_only:
        print(json.dumps(tail_times(a.reps)))
        return
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import build as svbuild
    kernels = main_kernels()
    pricer, params = sv.HawkesJDPricer(), sv.HawkesJDParams()
    kde = json.load(open(os.path.join(ROOT, "profiles", "kde_bench.json")))
    out = {"model": "Hawkes jump-diffusion, default HawkesJDParams", "ttm": TTM, "points": int(X.size), "reps": a.reps,
           "main_kernels": [{"XT": xt, "GT": gt, **m} for xt, gt, m in kernels],
           "kernel_metadata": {k: v for k, v in json.load(open(svbuild.EST_ISA_JSON))["metadata"].items() if "cond_density" in k},
           "kde_exp_per_s": next(r["exp_per_s_of_the_launches"] for r in kde["device_runs"] if r["n_path"] == 100000 and r["n_points"] == 200),
           "mc": {}}
    zeros = np.zeros(X.size, dtype=np.int8)
    for n in SIZES:
        eng = step_rows(n)
        out["mc"][str(n)] = {}
        for g in GAMMA_SETS:
            row = {"mixture_tail_ms": median_ms(lambda: eng.conditional_densities([X], g, mu_rows=[0], cv_rows=[1]), a.reps),
                   "greeks_tail_ms": median_ms(lambda: eng.tilted_conditional_greeks([1.0], [np.exp(X)], [zeros], g, False, mu_rows=[0],
                                                                                     cv_rows=[1]), a.reps),
                   "mixture_call_ms": median_ms(lambda: pricer.get_log_return_mc_pdf_mixture(params, TTM, X, risk_premia_gammas=g, nb_path=n),
                                                a.reps),
                   "greeks_route_call_ms": median_ms(lambda: pricer.get_log_return_mc_pdf_conditional_under_risk_kernel(params, TTM, X, g,
                                                                                                                         nb_path=n), a.reps),
                   "weighted_kde_call_ms": median_ms(lambda: pricer.get_log_return_mc_pdf_device(TTM, params, X, nb_path=n,
                                                                                                 risk_premia_gamma=g), a.reps)}
            step_rows(n)                                     # (the other routes left their own rows)
            row["GT"] = tile_of(kernels, len(g))
            row["exp_per_s"] = n * X.size * -(-len(g) // row["GT"]) / (1e-3 * row["mixture_tail_ms"])
            row["tail_vs_greeks_tail"] = row["mixture_tail_ms"] / row["greeks_tail_ms"]
            row["call_vs_greeks_route"] = row["mixture_call_ms"] / row["greeks_route_call_ms"]
            row["call_vs_weighted_kde"] = row["mixture_call_ms"] / row["weighted_kde_call_ms"]
            out["mc"][str(n)][str(len(g))] = row
    if not a.no_variants:
        out["variants"] = variant_comparison([tuple(s.split("=", 1)) for s in a.variant_lib], a.reps)
    text = json.dumps(out)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
