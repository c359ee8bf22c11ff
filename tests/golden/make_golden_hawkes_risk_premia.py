"""
Generate tests/golden/hawkes_risk_premia.npz from the UNMODIFIED Python reference: the risk-premia (Esscher-type) side of
pricers/hawkes_jd_pricer.py (hawkesjd_forwards_under_risk_kernel :487-515, hawkesjd_chain_pricer_with_risk_premia :420-484,
HawkesJDPricer.calibrate_risk_premia_gamma_to_chain :304-357) and utils/mgf_pricer.py's slice_pricer_with_mgf_grid_with_gamma
(:273-321).  Runs only in the build container, like make_golden_hawkes_calibration.py (same _shims for numba, same Black
helpers bound to stochvolmodels_amd.data.option_chain's):

    python tests/golden/make_golden_hawkes_risk_premia.py                     # everything, one process
    python tests/golden/make_golden_hawkes_risk_premia.py --parts A,B --save P.npz   # some parts into a partial file
    python tests/golden/make_golden_hawkes_risk_premia.py --merge P1.npz P2.npz ...  # partial files -> the fixture

The full 100-iteration calibration takes about 20 minutes on one core; --parts lets the slow parts run side by side.

The chain is the reference's get_btc_test_chain_data() passed through OptionChain.to_forward_normalised_strikes, as
papers/jump_risk_premia_clustered_jumps/calibrate_chain.py does.  `tight`: SciPy's solve_ivp tightened to rtol 1e-10 /
atol 1e-12 (the idiom of make_golden_hawkes.py); `default`: SciPy's own tolerance.  Stored:
  chain           ttms, forwards (ones), discfactors, forwards0, strikes_i, types_i, bid_i, ask_i
  gammas          the risk-premia gammas of the forward and chain-price parts
  param_sets      [2][16] HawkesJDParams() and the same with lambda_p = 50, lambda_m = 5 (twin.PARAM_NAMES order)
  fwd_{tol}_{s}_{case}_{norm|gfwd}  [n_gammas][n] hawkesjd_forwards_under_risk_kernel, case chain (the chain's ttms with
                  forwards0), grid (linspace(0.01, 0.5, 12) with linspace forwards) and paper (the same ttms with the paper's
                  forwards=np.array([1.0]): only the first entry is computed); _failed: where either of the entry's two
                  solve_ivp calls failed (status != 0: the solution blows up before ttm) and the reference kept the last
                  state it reached
  grid_ttms, grid_forwards
  prices_{tol}_{s}_{g}_{i}   hawkesjd_chain_pricer_with_risk_premia, param set s, gamma index g, expiry i
  slice_*         one slice's log_mgf on the risk grid (tight, set 1, gamma 1, first expiry) and the slice pricer's output
  obj_*           the calibration objective (vega-weighted and not) at a few (sigma, gamma / 8) vectors, tight and default,
                  with the weights and market vols read from the objective's closure and the options handed to minimize
  cal_{tag}_*     full calibrate_risk_premia_gamma_to_chain runs: x, fun, nfev, nit, status, wall time, maxiter, and the
                  objective calls counted by a probe around minimize.  default_chain: the 4-expiry chain,
                  is_vega_weighted=False, maxiter=100; default_slice: the first expiry alone, is_vega_weighted=True, maxiter=100;
                  tight_slice: the one-slice run at the tight tolerance, capped at maxiter=5.  The 4-expiry tight run is not
                  recorded: SLSQP's first line search reaches (sigma, gamma) = (1.45, 7.87), where the coefficient ODEs blow up
                  within the chain's ttms and SciPy's tightened solver ran for over 40 minutes on that one pricing without
                  finishing (`--parts cal_tight_chain` still runs it)
"""
import argparse
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
import stochvolmodels.utils.mgf_pricer as rmgf  # noqa: E402

from make_golden_hawkes_calibration import bind_black_helpers, params_vec  # noqa: E402

GAMMAS = np.array([-2.0, -0.5, 0.0, 1e-4, 1.0, 4.8])
OBJ_SAMPLES = np.array([[0.45, 0.0], [0.5248, 2.504 / 8.0], [0.35, -0.2], [0.7, 0.6]])
GRID_TTMS = np.linspace(0.01, 0.5, 12)
GRID_FORWARDS = np.linspace(1.0, 1.1, 12)


def param_sets():
    p0 = hp.HawkesJDParams()
    p1 = hp.HawkesJDParams()
    p1.lambda_p, p1.lambda_m = 50.0, 5.0
    return [p0, p1]


def calib_params0():
    p = hp.HawkesJDParams()
    p.lambda_p, p.lambda_m, p.risk_premia_gamma = 50.0, 5.0, 0.0
    return p


def chains():
    chain = roc.OptionChain.to_forward_normalised_strikes(obj=svm.get_btc_test_chain_data())
    first = roc.OptionChain.get_slices_as_chain(chain, ids=[chain.ids[0]])
    return chain, first


class Tol:
    """solve_ivp at SciPy's default tolerance or tightened, patched into the reference module for a `with` block"""

    def __init__(self, tight: bool):
        self.tight, self.orig = tight, hp.solve_ivp

    def __enter__(self):
        orig = self.orig

        def tight_ivp(*a, **k):
            k.setdefault("rtol", 1e-10)
            k.setdefault("atol", 1e-12)
            return orig(*a, **k)
        if self.tight:
            hp.solve_ivp = tight_ivp

    def __exit__(self, *exc):
        hp.solve_ivp = self.orig


class Captured(Exception):
    pass


class MinimizeProbe:
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


def part_chain():
    chain, _ = chains()
    out = dict(ttms=np.asarray(chain.ttms, dtype=np.float64), forwards=np.asarray(chain.forwards, dtype=np.float64),
               discfactors=np.asarray(chain.discfactors, dtype=np.float64),
               forwards0=np.asarray(chain.forwards0, dtype=np.float64), gammas=GAMMAS,
               param_sets=np.stack([params_vec(p) for p in param_sets()]), grid_ttms=GRID_TTMS, grid_forwards=GRID_FORWARDS,
               calib_params0=params_vec(calib_params0()), obj_samples=OBJ_SAMPLES)
    for i, (k, t, b, a) in enumerate(zip(chain.strikes_ttms, chain.optiontypes_ttms, chain.bid_ivs, chain.ask_ivs)):
        out[f"strikes_{i}"], out[f"types_{i}"] = np.asarray(k, dtype=np.float64), np.asarray(t)
        out[f"bid_{i}"], out[f"ask_{i}"] = np.asarray(b, dtype=np.float64), np.asarray(a, dtype=np.float64)
    return out


def part_forwards():
    chain, _ = chains()
    out = {}
    cases = dict(chain=(np.asarray(chain.ttms, dtype=float), np.asarray(chain.forwards0, dtype=float)),
                 grid=(GRID_TTMS, GRID_FORWARDS), paper=(GRID_TTMS, np.array([1.0])))
    for tol in ("tight", "default"):
        with Tol(tol == "tight"):
            inner, statuses = hp.solve_ivp, []

            def recording_ivp(*a, **k):                       # one solve per point: phi = -gamma, then -gamma - 1
                sol = inner(*a, **k)
                statuses.append(sol.status)
                return sol
            hp.solve_ivp = recording_ivp
            try:
                for s, params in enumerate(param_sets()):
                    for case, (ttms, fwds) in cases.items():
                        res, failed = [], []
                        for g in GAMMAS:
                            statuses.clear()
                            res.append(hp.hawkesjd_forwards_under_risk_kernel(model_params=params, risk_premia_gamma=float(g),
                                                                              ttms=ttms, forwards=fwds))
                            st = np.array(statuses).reshape(-1, 2)
                            failed.append(np.concatenate([np.any(st != 0, axis=1), np.zeros(ttms.size - len(st), bool)]))
                        out[f"fwd_{tol}_{s}_{case}_norm"] = np.stack([r[0] for r in res])
                        out[f"fwd_{tol}_{s}_{case}_gfwd"] = np.stack([r[1] for r in res])
                        out[f"fwd_{tol}_{s}_{case}_failed"] = np.stack(failed)
            finally:
                hp.solve_ivp = inner
    print("forwards done")
    return out


def part_prices(tol: str, s: int):
    chain, _ = chains()
    params = param_sets()[s]
    out = {}
    t0 = time.perf_counter()
    with Tol(tol == "tight"):
        for g, gamma in enumerate(GAMMAS):
            params.risk_premia_gamma = float(gamma)
            prices = hp.hawkesjd_chain_pricer_with_risk_premia(model_params=params, ttms=chain.ttms, forwards=chain.forwards,
                                                               discfactors=chain.discfactors, strikes_ttms=chain.strikes_ttms,
                                                               optiontypes_ttms=chain.optiontypes_ttms)
            for i, p in enumerate(prices):
                out[f"prices_{tol}_{s}_{g}_{i}"] = np.asarray(p, dtype=np.float64)
    out[f"prices_{tol}_{s}_wall_s"] = (time.perf_counter() - t0) / len(GAMMAS)
    print("prices", tol, s, f"{out[f'prices_{tol}_{s}_wall_s']:.2f} s per pricing")
    return out


def part_slice():
    chain, _ = chains()
    params = param_sets()[1]
    gamma = 1.0
    vol_scaler = hp.set_vol_scaler(sigma0=params.sigma, ttm=np.min(chain.ttms))
    phi, psi, theta = rmgf.get_transform_var_grid(max_phi=hp.MAX_PHI, vol_scaler=vol_scaler, real_phi=-0.5 - gamma)
    ttm, fwd = float(chain.ttms[0]), float(chain.forwards[0])
    with Tol(True):
        _, log_mgf = hp.compute_hawkes_a_mgf_grid(ttm=ttm, phi_grid=phi, psi_grid=psi, model_params=params)
        norm, gfwd = hp.hawkesjd_forwards_under_risk_kernel(model_params=params, risk_premia_gamma=gamma,
                                                            ttms=np.array([ttm]), forwards=np.array([fwd]))
    strikes, types = np.asarray(chain.strikes_ttms[0], dtype=float), np.asarray(chain.optiontypes_ttms[0])
    prices = rmgf.slice_pricer_with_mgf_grid_with_gamma(log_mgf_grid=log_mgf, phi_grid=phi, risk_premia_gamma=gamma, ttm=ttm,
                                                        forward=fwd, normalizer=float(norm[0]), gamma_forward=float(gfwd[0]),
                                                        strikes=strikes, optiontypes=types)
    # the real shortcut at gamma = -0.5 on the same log_mgf: the branch is picked from the grid alone
    phi_s = 1j * phi.imag
    prices_short = rmgf.slice_pricer_with_mgf_grid_with_gamma(log_mgf_grid=log_mgf, phi_grid=phi_s, risk_premia_gamma=-0.5,
                                                              ttm=ttm, forward=fwd, normalizer=float(norm[0]),
                                                              gamma_forward=float(gfwd[0]), strikes=strikes, optiontypes=types)
    return dict(slice_phi=phi, slice_log_mgf=log_mgf, slice_gamma=gamma, slice_ttm=ttm, slice_forward=fwd,
                slice_normalizer=float(norm[0]), slice_gamma_forward=float(gfwd[0]), slice_strikes=strikes,
                slice_types=types, slice_prices=prices, slice_prices_shortcut=prices_short)


def capture(pricer, chain, is_vega_weighted):
    probe = MinimizeProbe(run=False)
    hp.minimize = probe
    try:
        pricer.calibrate_risk_premia_gamma_to_chain(option_chain=chain, params0=calib_params0(),
                                                    is_vega_weighted=is_vega_weighted, print_iter=False)
    except Captured:
        pass
    finally:
        hp.minimize = probe.orig
    return probe


def part_objective():
    chain, _ = chains()
    pricer = hp.HawkesJDPricer()
    out = {}
    for vw in (False, True):
        probe = capture(pricer, chain, vw)
        tag = "vega" if vw else "flat"
        out[f"obj_{tag}_weights"] = np.asarray(probe.closure("weights"), dtype=float)
        out[f"obj_{tag}_market_vols"] = np.asarray(probe.closure("market_vols"), dtype=float)
        if not vw:
            out["obj_x0"], out["obj_bounds"] = probe.x0, np.asarray(probe.kw["bounds"], dtype=float)
            opts = probe.kw["options"]
            out.update(obj_ftol=float(opts["ftol"]), obj_maxiter=int(opts["maxiter"]), obj_eps=float(opts["eps"]),
                       obj_tol=float(probe.kw["tol"]), obj_disp=bool(opts["disp"]))
        for tol in ("tight", "default"):
            with Tol(tol == "tight"):
                out[f"obj_{tag}_{tol}"] = np.array([probe.fun(s, None) for s in OBJ_SAMPLES])
        print("objective", tag, out[f"obj_{tag}_tight"], out[f"obj_{tag}_default"])
    return out


def part_calibration(tag: str):
    chain, first = chains()
    tol, which = tag.split("_")
    ch, vw = (chain, False) if which == "chain" else (first, True)
    maxiter = 100 if tol == "default" else 5
    pricer = hp.HawkesJDPricer()
    probe = MinimizeProbe(run=True)
    hp.minimize = probe
    try:
        with Tol(tol == "tight"):
            t0 = time.perf_counter()
            fit = pricer.calibrate_risk_premia_gamma_to_chain(option_chain=ch, params0=calib_params0(), is_vega_weighted=vw,
                                                              maxiter=maxiter, print_iter=False)
            wall = time.perf_counter() - t0
    finally:
        hp.minimize = probe.orig
    res = probe.res
    print("cal", tag, "x", np.asarray(res.x).tolist(), "fun", res.fun, "nfev", res.nfev, "nit", res.nit, "status", res.status,
          res.message, f"{wall:.1f} s")
    return {f"cal_{tag}_x": np.asarray(res.x, dtype=float), f"cal_{tag}_params": params_vec(fit),
            f"cal_{tag}_gamma": float(fit.risk_premia_gamma), f"cal_{tag}_fun": float(res.fun),
            f"cal_{tag}_nfev": int(res.nfev), f"cal_{tag}_objective_calls": probe.n_calls, f"cal_{tag}_nit": int(res.nit),
            f"cal_{tag}_status": int(res.status), f"cal_{tag}_wall_s": wall, f"cal_{tag}_maxiter": maxiter,
            f"cal_{tag}_vega_weighted": vw}


PARTS = {"chain": part_chain, "forwards": part_forwards, "slice": part_slice, "objective": part_objective,
         **{f"prices_{tol}_{s}": (lambda tol=tol, s=s: part_prices(tol, s)) for tol in ("tight", "default") for s in (0, 1)},
         **{f"cal_{t}": (lambda t=t: part_calibration(t)) for t in ("default_chain", "default_slice", "tight_slice")}}
OPTIONAL_PARTS = {"cal_tight_chain": lambda: part_calibration("tight_chain")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--save", default=os.path.join(HERE, "hawkes_risk_premia.npz"))
    ap.add_argument("--merge", nargs="*")
    args = ap.parse_args()
    bind_black_helpers()
    out = {}
    if args.merge:
        for path in args.merge:
            with np.load(path, allow_pickle=False) as f:
                out.update({k: f[k] for k in f.files})
        sentinel = dict(chain="ttms", forwards="fwd_tight_0_chain_norm", slice="slice_prices", objective="obj_flat_tight")
        missing = [k for k in PARTS if not any(key == sentinel.get(k) or key.startswith(k + "_") for key in out)]
        assert not missing, missing
    else:
        for name in args.parts.split(","):
            out.update({**PARTS, **OPTIONAL_PARTS}[name]())
    np.savez_compressed(args.save, **out)
    print(f"{os.path.basename(args.save)}  {os.path.getsize(args.save) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
