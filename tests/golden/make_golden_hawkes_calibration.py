"""
Generate tests/golden/hawkes_calibration.npz from the UNMODIFIED Python reference (pricers/hawkes_jd_pricer.py,
HawkesJDPricer.calibrate_model_params_to_chain).  Runs only in the build container, like make_golden_hawkes.py (same _shims
for numba):

    python tests/golden/make_golden_hawkes_calibration.py

The Black vega and implied-vol routines the reference calls live in the third-party `vanilla_option_pricers`, absent here: as
in make_golden.py's g_calibration they are bound to the host helpers of stochvolmodels_amd.data.option_chain (textbook
Black-76), so the fixture pins the calibration LOOP (codec, weights, objective, constraint, SLSQP), not that inversion.

The chain is the reference's get_btc_test_chain_data() with its bid / ask vols (4 expiries, 49 quotes), passed through
OptionChain.to_forward_normalised_strikes as papers/jump_risk_premia_clustered_jumps/calibrate_chain.py does, and params0 is
HawkesJDParams(), as there.  Stored:
  chain           ttms, forwards (ones), discfactors, forwards0, strikes_i, types_i, bid_i, ask_i
  params0         the 16 fields of HawkesJDParams() in twin.PARAM_NAMES order
  weights         the objective's vega weights, read from the objective closure the reference hands to minimize
  market_vols     the same closure's flattened mid vols
  x0, bounds      the start vector and bounds the reference passes to minimize
  samples         three optimizer vectors (x0 and two others); sample_params: their unpacked 16-field sets (the closure's
                  unpack_pars); sample_conds: the constraint function at each; sample_objective_tight: the reference's
                  objective at each with solve_ivp tightened to rtol 1e-10 / atol 1e-12 (the `tight` idiom of
                  make_golden_hawkes.py's g_analytic); sample_objective_default: the same at SciPy's default tolerance
  default_* / tight_*  full reference calibrations at SciPy's default solve_ivp tolerance and tightened: the optimizer's
                  vector (x), the unpacked fit (params), the final objective (fun), objective evaluations (nfev), SLSQP
                  iterations (nit), the SLSQP status and the wall time in seconds on one CPU core of the build container
  default_fit_objective_tight  the reference's tightened objective at the default-tolerance fit
The objective is captured by wrapping the module's `minimize`, not restated.
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "_shims"))
sys.path.insert(0, "/root/reference/src")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import stochvolmodels as svm  # noqa: E402
import stochvolmodels.data.option_chain as roc  # noqa: E402
import stochvolmodels.pricers.hawkes_jd_pricer as hp  # noqa: E402

from stochvolmodels_amd.data import option_chain as host  # noqa: E402  pure-host helpers, no GPU needed

import hawkes_twin as twin  # noqa: E402

# two optimizer vectors beside x0: (sigma, mean_p, mean_m, theta_p, theta_m, kappa, beta_p, beta_m)
OTHER_SAMPLES = np.array([[0.55, 0.05, -0.05, 10.0, 12.0, 30.0, 60.0, 30.0],
                          [0.35, 0.02, -0.08, 4.0, 6.0, 15.0, 40.0, 10.0]])


def bind_black_helpers():
    def vegas_ttms(ttms, forwards, strikes_ttms, optiontypes_ttms, vols_ttms):
        return [host.black_vega(float(f), np.asarray(k, float), float(t), np.asarray(v, float))
                for t, f, k, v in zip(ttms, forwards, strikes_ttms, vols_ttms)]

    def ivols_ttms(ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms, model_prices_ttms):
        return [host.infer_black_ivols(np.asarray(p, float), float(t), float(f), np.asarray(k, float), ty, float(d))
                for t, f, d, k, ty, p in zip(ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms, model_prices_ttms)]
    roc.bsm.compute_bsm_vegas_ttms = vegas_ttms
    roc.bsm.infer_bsm_ivols_from_model_chain_prices = ivols_ttms


def params_vec(p):
    return np.array([getattr(p, k) for k in twin.PARAM_NAMES], dtype=np.float64)


class Captured(Exception):
    pass


class MinimizeProbe:
    """stands in for the module's `minimize`: records what the reference hands it, then either stops (capture) or runs the
    real SLSQP counting objective calls"""

    def __init__(self, run: bool):
        self.run, self.orig, self.n_calls = run, hp.minimize, 0

    def __call__(self, fun, x0, **kw):
        self.fun, self.x0, self.kw = fun, np.array(x0, dtype=float), kw
        if not self.run:
            raise Captured()

        def counted(*a, **k):
            self.n_calls += 1
            return fun(*a, **k)
        self.res = self.orig(counted, x0, **kw)
        return self.res

    def closure(self, name):
        return self.fun.__closure__[self.fun.__code__.co_freevars.index(name)].cell_contents


def with_solver(tight: bool):
    orig = hp.solve_ivp

    def tight_ivp(*a, **k):
        k.setdefault("rtol", 1e-10)
        k.setdefault("atol", 1e-12)
        return orig(*a, **k)
    return orig, (tight_ivp if tight else orig)


def calibrate(pricer, chain, params0, tight: bool, out: dict, tag: str):
    probe = MinimizeProbe(run=True)
    orig_ivp, ivp = with_solver(tight)
    hp.minimize, hp.solve_ivp = probe, ivp
    try:
        t0 = time.perf_counter()
        fit = pricer.calibrate_model_params_to_chain(option_chain=chain, params0=params0, is_vega_weighted=True)
        wall = time.perf_counter() - t0
    finally:
        hp.minimize, hp.solve_ivp = probe.orig, orig_ivp
    res = probe.res
    out.update({f"{tag}_x": np.asarray(res.x, dtype=float), f"{tag}_params": params_vec(fit), f"{tag}_fun": float(res.fun),
                f"{tag}_nfev": int(res.nfev), f"{tag}_objective_calls": probe.n_calls, f"{tag}_nit": int(res.nit),
                f"{tag}_status": int(res.status), f"{tag}_wall_s": wall})
    print(tag, "fun", res.fun, "nfev", res.nfev, "nit", res.nit, "status", res.status, res.message, f"{wall:.1f} s")
    print(tag, "x", np.asarray(res.x).tolist())
    return probe


def main():
    bind_black_helpers()
    chain = roc.OptionChain.to_forward_normalised_strikes(obj=svm.get_btc_test_chain_data())
    params0 = hp.HawkesJDParams()
    pricer = hp.HawkesJDPricer()
    out = dict(ttms=np.asarray(chain.ttms, dtype=np.float64), forwards=np.asarray(chain.forwards, dtype=np.float64),
               discfactors=np.asarray(chain.discfactors, dtype=np.float64),
               forwards0=np.asarray(chain.forwards0, dtype=np.float64), params0=params_vec(params0))
    for i, (k, t, b, a) in enumerate(zip(chain.strikes_ttms, chain.optiontypes_ttms, chain.bid_ivs, chain.ask_ivs)):
        out[f"strikes_{i}"], out[f"types_{i}"] = np.asarray(k, dtype=np.float64), np.asarray(t)
        out[f"bid_{i}"], out[f"ask_{i}"] = np.asarray(b, dtype=np.float64), np.asarray(a, dtype=np.float64)

    # the objective closure, its codec and its constraint, without running SLSQP
    probe = MinimizeProbe(run=False)
    hp.minimize = probe
    try:
        pricer.calibrate_model_params_to_chain(option_chain=chain, params0=params0, is_vega_weighted=True)
    except Captured:
        pass
    finally:
        hp.minimize = probe.orig
    unpack = probe.closure("unpack_pars")
    cons = probe.kw["constraints"]
    samples = np.vstack([probe.x0, OTHER_SAMPLES])
    out.update(weights=np.asarray(probe.closure("weights"), dtype=float),
               market_vols=np.asarray(probe.closure("market_vols"), dtype=float), x0=probe.x0,
               bounds=np.asarray(probe.kw["bounds"], dtype=float), ftol=float(probe.kw["options"]["ftol"]),
               samples=samples, sample_params=np.stack([params_vec(unpack(pars=s)) for s in samples]),
               sample_conds=np.array([cons["fun"](s) for s in samples]))
    out["sample_objective_default"] = np.array([probe.fun(s, None) for s in samples])
    orig_ivp, tight_ivp = with_solver(True)
    hp.solve_ivp = tight_ivp
    try:
        t0 = time.perf_counter()
        out["sample_objective_tight"] = np.array([probe.fun(s, None) for s in samples])
        out["tight_eval_s"] = (time.perf_counter() - t0) / len(samples)
    finally:
        hp.solve_ivp = orig_ivp
    print("samples", out["sample_objective_default"], out["sample_objective_tight"])

    calibrate(pricer, chain, params0, False, out, "default")
    calibrate(pricer, chain, params0, True, out, "tight")
    hp.solve_ivp = tight_ivp
    try:
        out["default_fit_objective_tight"] = float(probe.fun(out["default_x"], None))
    finally:
        hp.solve_ivp = orig_ivp

    path = os.path.join(HERE, "hawkes_calibration.npz")
    np.savez_compressed(path, **out)
    print(f"hawkes_calibration.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
