#!/usr/bin/env python
"""
Measurement of the Hawkes jump-diffusion (csrc/svmc_hawkes.hip) on the reference's BTC test chain (4 expiries, 49 options,
780 steps at the reference's 1800 per year; tests/golden/hawkes_analytic.npz), default HawkesJDParams.  Prints ONE JSON line:

  mc[n]         n = 10^5 (the reference's default) and 2^20 paths: whole-call ms of hawkesjd_mc_chain_pricer (median), the
                stepping launch's ms (svmc_session_time_stepping), path-steps/s of the stepping, and the time loop's instruction
                counts from libsvmc.isa.json
  analytic_ms   hawkesjd_chain_pricer (DOP853, rtol 1e-10), median
  z_default     (MC - analytic) / stderr of every option at 1800 steps per year, 2^20 paths: the reference's
                time-discretisation bias (expected to lean negative); not asserted anywhere
  cpu_twin      the reference algorithm in NumPy (tests/hawkes_twin.py) at 4096 paths, scaled linearly to 10^5 paths --
                labelled as such: a CPU figure of the reference's own algorithm, not of this library

    python tools/bench_hawkes.py [--reps 10]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
    from stochvolmodels_amd import build as svbuild
    from stochvolmodels_amd.engine import get_engine
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    import hawkes_twin as twin

    f = np.load(os.path.join(ROOT, "tests", "golden", "hawkes_analytic.npz"))
    m = f["ttms"].size
    ttms, fw, df = f["ttms"], f["forwards"], f["discfactors"]
    ks, ts = [f[f"strikes_{i}"] for i in range(m)], [f[f"types_{i}"] for i in range(m)]
    p = hp.HawkesJDParams()
    kw = {k: getattr(p, k) for k in hp.PARAM_NAMES}
    steps = sum(twin.time_grid(t - t0, 1800)[0] for t, t0 in zip(ttms, np.concatenate([[0.0], ttms[:-1]])))
    isa = json.load(open(svbuild.ISA_JSON))["kernels"].get("hawkesjd_chain_rng_kernel", {})
    out = {"chain": "BTC test chain, 4 expiries, 49 options", "steps": int(steps), "steps_per_year": 1800,
           "isa_loop": {k: isa.get(k) for k in ("instructions", "valu", "lds", "salu", "classes")}, "mc": {}}

    def call(n, seed=None, spy=1800):
        return hp.hawkesjd_mc_chain_pricer(ttms=ttms, forwards=fw, discfactors=df, strikes_ttms=ks, optiontypes_ttms=ts,
                                           nb_path=n, seed=seed, nb_steps_per_year=spy, **kw)

    for n in (100000, 1 << 20):
        for _ in range(3):
            call(n)
        eng = get_engine(n)
        wall, step = [], []
        for _ in range(reps):
            eng.start_kernel_timing()
            t0 = time.perf_counter()
            call(n)
            wall.append(1e3 * (time.perf_counter() - t0))
            step += eng.stop_kernel_timing().get("hawkesjd_chain_rng_kernel", [])
        st = float(np.median(step))
        out["mc"][str(n)] = {"call_ms": float(np.median(wall)), "stepping_ms": st,
                             "path_steps_per_s": n * steps / (st * 1e-3), "reps": reps}

    for _ in range(2):
        hp.hawkesjd_chain_pricer(model_params=p, ttms=ttms, forwards=fw, discfactors=df, strikes_ttms=ks, optiontypes_ttms=ts)
    ta = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ref = hp.hawkesjd_chain_pricer(model_params=p, ttms=ttms, forwards=fw, discfactors=df, strikes_ttms=ks, optiontypes_ttms=ts)
        ta.append(1e3 * (time.perf_counter() - t0))
    out["analytic_ms"] = float(np.median(ta))

    pr, sd = call(1 << 20, seed=2025)
    z = (np.concatenate(pr) - np.concatenate(ref)) / np.concatenate(sd)
    out["z_default"] = {"n_path": 1 << 20, "seed": 2025, "mean": float(np.mean(z)), "min": float(np.min(z)),
                        "max": float(np.max(z)), "beyond_3": int(np.sum(np.abs(z) > 3)), "z": [round(float(v), 3) for v in z]}

    t0 = time.perf_counter()
    twin.mc_chain(ttms, fw, df, ks, ts, kw, 4096, 1)
    tc = time.perf_counter() - t0
    out["cpu_twin"] = {"label": "reference algorithm in NumPy (tests/hawkes_twin.py, draws included), 4096 paths, scaled to 10^5",
                       "s_4096": tc, "s_scaled_1e5": tc * 100000 / 4096}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
