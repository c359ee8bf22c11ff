"""Shared by tests/test_gpu_cmc_sets.py and its child process: the conditional calibration objective's call
(logsv_mc_chain_pricer_conditional_sets / heston_mc_chain_pricer_conditional_sets) and, per set, the single
conditional call it must equal bit for bit.

As a program it is the worker of tests/test_gpu_cmc_sets.py::test_bits_full_launch_form: the test starts it with
SVMC_FEW_WAVES_MAX_PATHS=0 (read once per process), so that every stepping launch runs the FULL-LAUNCH kernels, and it writes the
flattened results of the sets call and of the single calls to the .npz named on its command line:
    python tests/cmc_sets_worker.py OUT.npz N_PATH"""
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cmc_many_worker as mw  # noqa: E402

# three expiries: nine strikes (calls and puts mixed, 0.8 F to 1.2 F), a call at 0.3 F -- all intrinsic value: its price sits within
# an ulp of the bracket's lower end, and whichever side rounding puts it on, the kernel must say what the host routine says -- and a
# call at K <= 0, which has no vol (NaN by contract); one strike; none
TTMS = np.array([1.0 / 12.0, 0.25, 0.5])
FORWARDS = np.array([1.0, 1.05, 0.95])
DISCFACTORS = np.array([0.999, 0.995, 0.99])
STRIKES = [np.array([0.8, 0.9, 1.0, 1.1, 1.2, 0.85, 1.0, 1.15, 0.95, 0.3, -0.5]), np.array([1.05]), np.array([])]
TYPES = [np.array(["C", "C", "C", "C", "C", "P", "P", "P", "P", "C", "C"]), np.array(["P"]), np.array([])]
CHAIN = dict(ttms=TTMS, forwards=FORWARDS, discfactors=DISCFACTORS, strikes_ttms=STRIKES, optiontypes_ttms=TYPES)
SPY = 120
STATS_FIELDS = ("forward_mc", "forward_mc_stderr", "corr", "n_kept", "n_dropped")


def logsv_params(row):
    """the LogSvParams of a row of cmc_many_worker.py, its etas on this chain's three expiries"""
    from stochvolmodels_amd import LogSvParams
    p = LogSvParams(sigma0=row[0], theta=row[1], kappa1=row[2], kappa2=row[3], beta=row[4], volvol=row[5])
    etas = np.asarray(row[6:6 + TTMS.size], dtype=float)
    if np.any(etas != 1.0):
        p.set_vol_backbone(pd.Series(etas, index=TTMS))
    return p


def heston_params(row):
    from stochvolmodels_amd import HestonParams
    return HestonParams(v0=row[0], theta=row[1], kappa=row[2], rho=row[3], volvol=row[4])


def model_sets(model):
    """{name: parameters}: two differing sets (LogSV's B with an eta != 1) and the zero-noise set"""
    if model == "logsv":
        return {"A": logsv_params(mw.LOGSV_A), "B": logsv_params(mw.LOGSV_B), "Z": logsv_params(mw.LOGSV_ZERO)}
    return {"A": heston_params(mw.HESTON_A), "B": heston_params(mw.HESTON_B), "Z": heston_params(mw.HESTON_ZERO)}


def sets_list(model, n_sets):
    """n_sets parameter sets, cycling A, B, Z"""
    s = model_sets(model)
    return [s["ABZ"[q % 3]] for q in range(n_sets)]


def flat(result):
    """(prices, stderrs[, ivols], stats) of one set -> [prices | stderrs | stats] flattened and the vols (or None)"""
    prices, stderrs, stats = result[0], result[1], result[-1]
    ivols = np.concatenate([np.ravel(v) for v in result[2]]) if len(result) == 4 else None
    st = np.array([[d[f] for f in STATS_FIELDS] for d in stats], dtype=float)
    return np.concatenate([np.concatenate([np.ravel(p) for p in prices]), np.concatenate([np.ravel(e) for e in stderrs]), st.ravel()]), ivols


def sets_call(model, params_list, n_path, seed, recenter=True, chain=None, spy=SPY):
    import stochvolmodels_amd as sv
    fn = sv.logsv_mc_chain_pricer_conditional_sets if model == "logsv" else sv.heston_mc_chain_pricer_conditional_sets
    out = fn(params_list, nb_path=n_path, nb_steps_per_year=spy, seed=seed, recenter=recenter, return_ivols=True, return_stats=True,
             **(chain or CHAIN))
    return [flat(r) for r in out]


def single_call(model, p, n_path, seed, recenter=True, chain=None, spy=SPY):
    """the single conditional call of one set, and the host routine's vols of its prices"""
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.data.option_chain import black_ivols_native
    chain = chain or CHAIN
    kw = dict(nb_path=n_path, nb_steps_per_year=spy, seed=seed, recenter=recenter, return_stats=True, **chain)
    if model == "logsv":
        out = sv.logsv_mc_chain_pricer_conditional(v0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2, beta=p.beta, volvol=p.volvol,
                                                   vol_backbone_etas=p.get_vol_backbone_etas(ttms=chain["ttms"]), **kw)
    else:
        out = sv.heston_mc_chain_pricer_conditional(v0=p.v0, theta=p.theta, kappa=p.kappa, rho=p.rho, volvol=p.volvol, **kw)
    ivols = [black_ivols_native(np.ravel(pr), float(t), float(f), np.ravel(k), np.ravel(ty), float(d))
             for pr, t, f, k, ty, d in zip(out[0], chain["ttms"], chain["forwards"], chain["strikes_ttms"], chain["optiontypes_ttms"],
                                           chain["discfactors"])]
    return flat(out)[0], np.concatenate(ivols)


def run(n_path):
    """{model_sets / model_sets_iv / model_single / model_single_iv: [8][...]} at eight sets, recentred"""
    out = {}
    for model in ("logsv", "heston"):
        plist = sets_list(model, 8)
        got = sets_call(model, plist, n_path, 21)
        ref = [single_call(model, p, n_path, 21) for p in plist]
        out[model + "_sets"], out[model + "_sets_iv"] = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
        out[model + "_single"], out[model + "_single_iv"] = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    return out


def main():
    assert os.environ.get("SVMC_FEW_WAVES_MAX_PATHS") == "0"
    np.savez(sys.argv[1], **run(int(sys.argv[2])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
