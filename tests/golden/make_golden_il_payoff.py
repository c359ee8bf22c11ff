"""
Generate tests/golden/il_payoff.npz, what tests/test_il_host.py, tests/test_gpu_il_transform.py and tests/test_gpu_il_mc.py hold
the impermanent-loss pricers to.  Runs on the CPU against the UNMODIFIED reference, imported under the
stand-ins of tests/golden/_shims; the reference's IL script is imported by path and no line of it is restated here:

    STOCHVOLMODELS_REFERENCE=<checkout of the reference> python tests/golden/make_golden_il_payoff.py [--jobs 4]

  sets      "cand" LogSvParams(sigma0=0.5, theta=0.5, kappa1=3, kappa2=3, beta=-0.3, volvol=1.0) and "paper", the parameter set of
            the script itself; ttms 10/365 and 0.25; p0 = 2200 and the three cases (pa, pb, p1) of CASES.
  f_*       per (set, ttm) the reference's logsv_il_pricer with scipy.solve_ivp tightened to rtol 1e-11 / atol 1e-13 (as
            make_golden_densities.py does): the phi grid and the log-MGF it solved (16 KB each; the solve is memoised per
            (set, ttm), since it does not depend on the case), and per case the five nansums the reference formed inside its
            vanilla, digital and square-root pricers (recorded by a numpy stand-in whose nansum notes what it returns), the six
            pieces (its pricers called again on the stored log-MGF) and the IL value.
  ref_seconds   wall-clock of one call of the reference as shipped (default solver) for the script's own case; ref_cpu.
  mc_*      the CPU twin's terminal states (oracle.logsv_terminal_rng, the cand set, MC_PATHS paths, seed MC_SEED, the daily
            grid) reduced by tests/il_twin.py's long-double estimator: value, stderr and pieces per (ttm, case), and the z-score
            of the reference's Fourier value against them.  The file is NOT written unless every |z| <= 4.  No path vector is
            stored.
"""
import argparse
import importlib.util
import os
import sys
import time
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("STOCHVOLMODELS_REFERENCE")
if not REFERENCE:
    raise SystemExit("set STOCHVOLMODELS_REFERENCE to a checkout of the reference")
sys.path.insert(0, os.path.join(HERE, "_shims"))
sys.path.insert(0, os.path.join(REFERENCE, "src"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import stochvolmodels.pricers.logsv.affine_expansion as afe  # noqa: E402
import stochvolmodels.utils.mgf_pricer as mgfp  # noqa: E402

_spec = importlib.util.spec_from_file_location("reference_il_script",
                                               os.path.join(REFERENCE, "papers", "il_hedging", "run_logsv_for_il_payoff.py"))
il = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(il)

SETS = {"cand": dict(sigma0=0.5, theta=0.5, kappa1=3.0, kappa2=3.0, beta=-0.3, volvol=1.0),
        "paper": dict(sigma0=0.4861785891939535, theta=0.6176006871606874, kappa1=1.955809653686808, kappa2=1.978367101612294,
                      beta=-0.26916969112829325, volvol=3.265815229306317)}
TTMS = (10.0 / 365.0, 0.25)
P0 = 2200.0
CASES = ((2000.0, 2400.0, 2200.0), (2000.0, 2400.0, 2050.0), (1800.0, 2600.0, 2500.0))         # (pa, pb, p1)
NOTIONAL = 1000000.0
MC_SEED, MC_PATHS = 20261, 400_000
_ORIG_SOLVE_IVP = afe.solve_ivp
_ORIG_MGF_GRID = il.compute_logsv_a_mgf_grid


def _tight(*a, **k):
    k.setdefault("rtol", 1e-11)
    k.setdefault("atol", 1e-13)
    return _ORIG_SOLVE_IVP(*a, **k)


class RecordingNumpy:
    """numpy, except that nansum notes every value it returns: the sums the reference's slice pricers form and do not return"""

    def __init__(self, seen):
        self._seen = seen

    def __getattr__(self, name):
        return getattr(np, name)

    def nansum(self, *a, **k):
        v = np.nansum(*a, **k)
        self._seen.append(float(v))
        return v


def solve_case_set(job):
    """one (set, ttm) in a worker: the unmodified logsv_il_pricer for the three cases, the ODE solve memoised and tightened"""
    tag, ttm = job
    afe.solve_ivp = _tight
    memo = {}

    def memoised(**kw):
        if "out" not in memo:
            memo["phi"] = np.array(kw["phi_grid"])
            memo["out"] = _ORIG_MGF_GRID(**kw)
        assert np.array_equal(memo["phi"], kw["phi_grid"])
        return memo["out"]

    seen = []
    il.compute_logsv_a_mgf_grid = memoised
    il.np = mgfp.np = RecordingNumpy(seen)
    try:
        params = il.LogSvParams(**SETS[tag])
        values, sums, pieces = [], [], []
        for pa, pb, p1 in CASES:
            del seen[:]
            values.append(float(il.logsv_il_pricer(params=params, ttm=ttm, p1=p1, p0=P0, pa=pa, pb=pb, notional=NOTIONAL)))
            # the order of the calls inside logsv_il_pricer: vanilla (pa, pb), digital (pa, pb), square root
            assert len(seen) == 5, seen
            sums.append([seen[4], seen[0], seen[1], seen[2], seen[3]])
            phi, lm = memo["phi"], memo["out"][1]
            van = mgfp.vanilla_slice_pricer_with_mgf_grid(log_mgf_grid=lm, phi_grid=phi, forward=p1, strikes=np.array([pa, pb]),
                                                          optiontypes=np.array(["P", "C"]), discfactor=1.0)
            dig = mgfp.digital_slice_pricer_with_mgf_grid(log_mgf_grid=lm, phi_grid=phi, forward=p1, strikes=np.array([pa, pb]),
                                                          optiontypes=np.array(["P", "C"]), discfactor=1.0)
            root = il.square_root_payoff_pricer_with_mgf_grid(log_mgf_grid=lm, phi_grid=phi, forward=p1, pa=pa, pb=pb, discfactor=1.0)
            pieces.append([float(root), float(np.sqrt(P0) * (p1 / P0 + 1.0)), float(van[0]), float(van[1]), float(dig[0]), float(dig[1])])
    finally:
        il.compute_logsv_a_mgf_grid = _ORIG_MGF_GRID
        il.np = mgfp.np = np
        afe.solve_ivp = _ORIG_SOLVE_IVP
    return job, memo["phi"], np.asarray(memo["out"][1]), np.array(values), np.array(sums), np.array(pieces)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or platform.machine()


def key(tag, ttm):
    return f"{tag}_{TTMS.index(ttm)}"


def g_mc(out):
    import il_twin
    from oracle import oracle
    p = SETS["cand"]
    z_all = []
    for i, ttm in enumerate(TTMS):
        nb_steps, dt = oracle.set_time_grid(ttm, 360)
        x, _, _ = oracle.logsv_terminal_rng(np.zeros(MC_PATHS), np.full(MC_PATHS, p["sigma0"]), np.zeros(MC_PATHS), nb_steps, dt,
                                            p["theta"], p["kappa1"], p["kappa2"], p["beta"], p["volvol"], MC_SEED)
        rows, zs = [], []
        for c, (pa, pb, p1) in enumerate(CASES):
            res, n_kept, n_dropped = il_twin.brute(x, p1, P0, pa, pb, NOTIONAL)
            assert n_dropped == 0
            assert il_twin.nearest_boundary(x, p1, pa, pb) > 1e-9, "a twin spot sits on a range boundary: choose another seed"
            rows.append([float(res[k]) for k in il_twin.FIELDS])
            zs.append((out[f"f_cand_{i}_values"][c] - rows[-1][0]) / rows[-1][1])
            print(f"mc ttm {ttm:.4f} case {c}: fourier {out[f'f_cand_{i}_values'][c]:.4f} mc {rows[-1][0]:.4f} +- {rows[-1][1]:.4f} "
                  f"z {zs[-1]:+.2f}", flush=True)
        out[f"mc_{i}_twin"] = np.array(rows)
        out[f"mc_{i}_z"] = np.array(zs)
        z_all += zs
    out.update(mc_seed=MC_SEED, mc_paths=MC_PATHS, mc_fields=np.array(il_twin.FIELDS))
    if np.max(np.abs(z_all)) > 4.0:
        raise SystemExit(f"the reference's Fourier value and the twin's Monte Carlo value are {np.max(np.abs(z_all)):.2f} standard "
                         "errors apart: the fixture is not written")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4)
    args = ap.parse_args()
    out = dict(ttms=np.array(TTMS), p0=P0, notional=NOTIONAL, cases=np.array(CASES), set_names=np.array(list(SETS)),
               pieces=np.array(["square_root", "linear", "put", "call", "digital_put", "digital_call"]),
               sums=np.array(["square_root", "capped_pa", "capped_pb", "digital_pa", "digital_pb"]))
    for tag, p in SETS.items():
        out[f"{tag}_params"] = np.array([p[k] for k in ("sigma0", "theta", "kappa1", "kappa2", "beta", "volvol")])
    with Pool(args.jobs) as pool:
        results = pool.imap_unordered(solve_case_set, [(tag, ttm) for tag in SETS for ttm in TTMS], chunksize=1)
        # meanwhile, in this process: the reference as shipped, the script's own case
        t0 = time.perf_counter()
        shipped = il.logsv_il_pricer(params=il.LogSvParams(**SETS["paper"]), ttm=TTMS[0], p1=2200.0, p0=P0, pa=2000.0, pb=2400.0)
        out.update(ref_seconds=time.perf_counter() - t0, ref_value_default_solver=float(shipped), ref_cpu=np.array(cpu_model()))
        print(f"reference as shipped: {shipped:.6f} in {out['ref_seconds']:.2f} s", flush=True)
        for (tag, ttm), phi, lm, values, sums, pieces in results:
            k = key(tag, ttm)
            out[f"f_{k}_phi"], out[f"f_{k}_log_mgf"] = phi, lm
            out[f"f_{k}_values"], out[f"f_{k}_sums"], out[f"f_{k}_pieces"] = values, sums, pieces
            print(f"{tag} ttm {ttm:.4f}: values {values}", flush=True)
    g_mc(out)
    path = os.path.join(HERE, "il_payoff.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"il_payoff.npz {size / 1024:.1f} KiB")
    assert size < 1024 * 1024, "over the size limit for a committed file"


if __name__ == "__main__":
    main()
