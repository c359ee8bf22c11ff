"""
GPU tests of the many-job conditional stepping kernels and the conditional estimator's parameter sensitivities (include/svmc.h,
DESIGN.md row f14):

  1  many-job stepping, few-waves form: every row of a five-job launch equals the job's single uniform-start call bit for bit,
     LogSV and Heston; permuting the jobs permutes the rows
  2  the same in the full-launch form, in a child process with SVMC_FEW_WAVES_MAX_PATHS=0 (tests/cmc_many_worker.py)
  3  the sensitivity tail on supplied (mu, cv) against the long-double twin (tests/cmc_sens_twin.py) within SENS_EPS eps DF max(F, K)
     / (2 h); n_pairs exact
  4  identities end to end: the base job's rows are the f13 call's bits, 2 h sens is the difference of two single conditional
     prices, identical paths give errors of exactly 0, the many-job pricer's jobs are their single calls, a quote does not depend
     on what shares the call
  5  the reported error against the spread over 64 seeds, per parameter, both recenter values
  6  agreement with the plain estimator's sensitivities (row f12) within 4 combined standard errors

With SVMC_CMC_SENS_TOLERANCES / SVMC_CMC_SENS_Z_JSON set to file names, items 3 and 5 / item 6 append what they measured
(profiles/cmc_sens_observed_tolerances.txt, profiles/cmc_sens_z_scores.json).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cmc_many_worker as cm  # noqa: E402
import cmc_sens_twin as st  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
SENS_EPS = 64.0            # a per-path price is good to a few ulp of max(F, K) (row f13 measured 1.5e-15 on O(1) values), a difference
                           # doubles that and blocked sums keep it: 64 eps leaves about 8 times over that


def note(line):
    print(line)
    path = os.environ.get("SVMC_CMC_SENS_TOLERANCES")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


# ---- 1, 2 -------------------------------------------------------------------------------------------------------------------------
def assert_rows_equal_single_calls(out, where):
    for model, jobs in cm.JOBS.items():
        many, single = out[model + "_many"], out[model + "_single"]
        assert many.shape == (2, len(jobs), cm.M, many.shape[-1]) and np.all(np.isfinite(many))
        for j in range(len(jobs)):
            for a, name in enumerate(("mu", "cv")):
                assert np.array_equal(many[a, j], single[j, a]), (where, model, j, name)
        # two jobs on one (seed, call id) are other paths for other parameters; equal parameters on other seeds too
        assert not np.array_equal(many[0, 0], many[0, 1]) and not np.array_equal(many[0, 2], many[0, 3])
        zero = many[:, len(jobs) - 1]
        assert np.all(zero == zero[..., :1]), (where, model, "the zero-noise job's paths are identical")


def test_many_job_stepping_few_waves_form():
    from stochvolmodels_amd.engine import HipEngine
    n = 300
    assert_rows_equal_single_calls(cm.run(n), "few waves")
    eng = HipEngine(n)
    try:
        for model, jobs in cm.JOBS.items():
            rows = cm.many_rows(eng, model, jobs)
            perm = [3, 0, 4, 2, 1]
            assert np.array_equal(cm.many_rows(eng, model, [jobs[j] for j in perm]), rows[:, perm]), model
            assert np.array_equal(cm.many_rows(eng, model, jobs[1:2])[:, 0], rows[:, 1]), model      # a job alone in its launch
    finally:
        eng.close()


def test_many_job_stepping_full_launch_form(tmp_path):
    """1 100 paths: whole blocks plus a partial one for the 1 024-thread (LogSV) and the 512-thread (Heston) kernels"""
    path = str(tmp_path / "many_full_launch.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "cmc_many_worker.py"), path, "1100"],
                       env=dict(os.environ, SVMC_FEW_WAVES_MAX_PATHS="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    g = np.load(path)
    assert_rows_equal_single_calls({k: g[k] for k in g.files}, "full launch")


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
TAIL_N = 700                                                   # three path blocks, the last partial
TAIL_F = np.array([1.0, 1.05, 0.95])
TAIL_DF = np.array([0.97, 0.99, 0.95])
TAIL_K = [np.array([0.8, 0.9, 1.0, 1.1, 1.2, 0.85, 1.0, 1.15, -0.5]), np.array([1.05]), np.array([])]     # 9, 1 and 0 strikes
TAIL_T = [np.array(["C", "C", "C", "C", "C", "P", "P", "P", "C"]), np.array(["P"]), np.array([])]         # K = -0.5: K' <= 0
TAIL_H = np.array([1e-3, 2.5e-3])


def tail_rows():
    """(mu_up, cv_up, mu_dn, cv_dn), each [P][m][n]: smooth functions of one draw per (parameter, expiry), with planted paths"""
    rng = np.random.default_rng(2024)
    out = [[[None] * 3 for _ in range(2)] for _ in range(4)]
    for p in range(2):
        for i in range(3):
            b = rng.standard_normal(TAIL_N)
            for a, s0 in ((0, 0.4 + TAIL_H[p]), (2, 0.4 - TAIL_H[p])):
                sigma = s0 * np.exp(0.5 * b - 0.125)
                T, rho = 0.25 * (i + 1), -0.6
                cv = (1 - rho * rho) * sigma * sigma * T
                mu = -0.5 * sigma * sigma * T + rho * sigma * np.sqrt(T) * b
                cv[3] = 0.0                                    # cv == 0 in both jobs
                cv[13] = 0.0 if a == 0 else cv[13]             # ... and in the up job only
                if a == 0:
                    mu[5] = np.nan                             # dropped in the up job only
                else:
                    cv[9] = -1e-3                              # cv < 0 in the dn job only
                if p == 1 and i == 1:
                    mu[0] = np.inf if a == 0 else mu[0]        # path 0 is not a kept pair: the shift is 0
                out[a][p][i], out[a + 1][p][i] = mu, cv
    return out


@pytest.mark.parametrize("recenter", [True, False])
def test_sens_tail_against_the_long_double_twin(recenter):
    from stochvolmodels_amd.engine import HipEngine
    rows = tail_rows()
    codes = [np.array([0 if t == "C" else 1 for t in ts], dtype=np.int8) for ts in TAIL_T]
    eng = HipEngine(TAIL_N)
    try:
        sens, slices = eng.conditional_sens(TAIL_F, TAIL_DF, TAIL_K, codes, TAIL_H, recenter, host_rows=rows)
    finally:
        eng.close()
    assert sens.shape == (2, 3, 10)
    worst = {"sens": 0.0, "sens_stderr": 0.0}
    ok = True
    for p in range(2):
        for i in range(2):
            want = st.estimator(rows[0][p][i], rows[1][p][i], rows[2][p][i], rows[3][p][i], TAIL_H[p], TAIL_F[i], TAIL_K[i], TAIL_T[i],
                                TAIL_DF[i], recenter)
            got = sens[p][:, slices[i]]
            bound = SENS_EPS * EPS * TAIL_DF[i] * np.maximum(TAIL_F[i], TAIL_K[i]) / (2 * TAIL_H[p])
            for r, name in enumerate(("sens", "sens_stderr")):
                ratio = np.abs(got[r] - want[r]) / bound
                worst[name] = max(worst[name], float(ratio.max()))
                ok = ok and bool(np.all(ratio <= 1.0)) and bool(np.all(np.isfinite(got[r])))
            assert np.array_equal(got[2], want[2].astype(np.float64)), (p, i, got[2], want[2])
            assert want[2][0] == TAIL_N - (3 if (p, i) == (1, 1) else 2)
    note(f"cmc sens tail recenter={recenter} n={TAIL_N}: largest |device - twin| / (64 eps DF max(F, K) / 2h): sens "
         f"{worst['sens']:.3f} sens_stderr {worst['sens_stderr']:.3f}")
    assert ok, worst


def test_sens_of_no_kept_pair_is_nan_with_a_count_of_zero():
    import stochvolmodels_amd as sv
    n = 70
    s, e, c = sv.compute_mc_vars_sens_conditional(np.full(n, np.nan), np.ones(n), np.zeros(n), np.ones(n), 1e-3, 1.0,
                                                  np.array([0.9, 1.1]), np.array(["C", "P"]))
    assert np.all(np.isnan(s)) and np.all(np.isnan(e)) and np.array_equal(c, [0, 0]) and c.dtype == np.int64
    mu_up, cv_up, mu_dn, cv_dn = (a[:n] for a in st.toy_jobs(5, -0.4))
    got = sv.compute_mc_vars_sens_conditional(mu_up, cv_up, mu_dn, cv_dn, st.TOY_BUMP, 1.0, np.array([[0.9], [1.1]]), np.array([["C"], ["P"]]))
    want = st.estimator(mu_up, cv_up, mu_dn, cv_dn, st.TOY_BUMP, 1.0, [0.9, 1.1], ["C", "P"])
    assert got[0].shape == (2, 1) and np.array_equal(got[2].ravel(), [n, n])
    bound = SENS_EPS * EPS * 1.1 / (2 * st.TOY_BUMP)
    assert np.all(np.abs(got[0].ravel() - want[0]) <= bound) and np.all(np.abs(got[1].ravel() - want[1]) <= bound)


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
ID_STRIKES = np.array([0.8, 0.9, 1.0, 1.1, 1.2])
ID_CHAIN = dict(ttms=np.array([1.0 / 12.0, 0.25]), forwards=np.array([1.0, 1.02]), discfactors=np.array([0.999, 0.995]),
                strikes_ttms=[ID_STRIKES, ID_STRIKES], optiontypes_ttms=[np.array(["P", "P", "C", "C", "C"])] * 2)
LOGSV_KW = dict(v0=0.2, theta=0.22, kappa1=3.0, kappa2=12.0, beta=-0.3, volvol=0.4, vol_backbone_etas=np.array([1.0, 1.05]))
HESTON_KW = dict(v0=0.04, theta=0.05, kappa=4.0, rho=-0.5, volvol=0.4)


def routes(model):
    """(greeks function, single pricer, keywords, wrt, {wrt name: keyword})"""
    import stochvolmodels_amd as sv
    if model == "logsv":
        return (sv.logsv_mc_chain_greeks_conditional, sv.logsv_mc_chain_pricer_conditional, LOGSV_KW, ("sigma0", "volvol"),
                {"sigma0": "v0", "volvol": "volvol"})
    return (sv.heston_mc_chain_greeks_conditional, sv.heston_mc_chain_pricer_conditional, HESTON_KW, ("v0", "rho"), {"v0": "v0", "rho": "rho"})


@pytest.mark.parametrize("recenter", [True, False])
@pytest.mark.parametrize("model", ["logsv", "heston"])
def test_base_rows_are_the_f13_bits_and_sens_is_the_difference_of_two_single_prices(model, recenter):
    from stochvolmodels_amd.engine import CMC_GREEKS_FIELDS
    greeks, pricer, kw, wrt, key = routes(model)
    n, seed, rel = 4096, 77, 1e-3
    out = greeks(nb_path=n, seed=seed, recenter=recenter, return_stats=True, wrt=wrt, rel_bump=rel, **ID_CHAIN, **kw)
    base = greeks(nb_path=n, seed=seed, recenter=recenter, return_stats=True, **ID_CHAIN, **kw)
    assert out["stats"] == base["stats"]
    for f in CMC_GREEKS_FIELDS:
        for i in range(2):
            assert np.array_equal(out[f][i], base[f][i]), (f, i)
    for name in wrt:
        v = kw[key[name]]
        h = rel * abs(v)
        up, _ = pricer(nb_path=n, seed=seed, recenter=recenter, **ID_CHAIN, **dict(kw, **{key[name]: v + h}))
        dn, _ = pricer(nb_path=n, seed=seed, recenter=recenter, **ID_CHAIN, **dict(kw, **{key[name]: v - h}))
        for i in range(2):
            assert np.array_equal(out["n_pairs"][name][i], np.full(5, n))                # all paths kept
            # three blocked sums of terms bounded by max(F, K)
            bound = SENS_EPS * EPS * ID_CHAIN["discfactors"][i] * np.maximum(ID_CHAIN["forwards"][i], ID_STRIKES)
            dev = np.abs(2 * h * out["sens"][name][i] - (up[i] - dn[i]))
            print(f"cmc sens identity {model} recenter={recenter} {name} expiry {i}: largest |2h sens - (up - dn)| / bound {np.max(dev / bound):.3f}")
            assert np.all(dev <= bound), (name, i, dev / bound)
            assert np.all(out["sens_stderr"][name][i] > 0.0)


@pytest.mark.parametrize("model", ["logsv", "heston"])
def test_identical_paths_give_errors_of_exactly_zero(model):
    greeks = routes(model)[0]
    if model == "logsv":
        kw, wrt = dict(LOGSV_KW, beta=0.0, volvol=0.0), ("sigma0", "theta", "kappa1")
    else:
        # volvol = 0 makes the variance path deterministic; the paths are identical once rho = 0 takes the driver out of mu too
        kw, wrt = dict(HESTON_KW, volvol=0.0, rho=0.0), ("v0", "theta", "kappa")
    for recenter in (True, False):
        out = greeks(nb_path=64, seed=3, recenter=recenter, wrt=wrt, **ID_CHAIN, **kw)
        for name in wrt:
            for i in range(2):
                assert np.all(out["sens_stderr"][name][i] == 0.0), (name, i, out["sens_stderr"][name][i])
                assert np.all(np.isfinite(out["sens"][name][i])) and np.all(out["n_pairs"][name][i] == 64)
        assert np.any(out["sens"][wrt[0]][1] != 0.0)


@pytest.mark.parametrize("model", ["logsv", "heston"])
def test_many_job_pricer_jobs_are_their_single_calls(model):
    import stochvolmodels_amd as sv
    n, seeds = 4096, [5, 6, 5]
    if model == "logsv":
        plist = [sv.LogSvParams(sigma0=0.2, theta=0.22, kappa1=3.0, kappa2=12.0, beta=-0.3, volvol=0.4),
                 sv.LogSvParams(sigma0=0.35, theta=0.3, kappa1=2.0, kappa2=5.0, beta=0.2, volvol=0.9), sv.LOGSV_BTC_PARAMS]
        many = sv.logsv_mc_chain_pricer_conditional_many(plist, nb_path=n, seeds=seeds, return_stats=True, **ID_CHAIN)
        singles = [sv.logsv_mc_chain_pricer_conditional(
            v0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2, beta=p.beta, volvol=p.volvol,
            vol_backbone_etas=p.get_vol_backbone_etas(ttms=ID_CHAIN["ttms"]), nb_path=n, seed=s, return_stats=True, **ID_CHAIN)
            for p, s in zip(plist, seeds)]
        oc = sv.OptionChain(ids=np.array(["a", "b"]), **ID_CHAIN)
        routed = sv.LogSVPricer().model_mc_price_chain_conditional_many(oc, plist[:2], nb_path=n, seeds=seeds[:2], nb_steps=360)
    else:
        plist = [sv.HestonParams(v0=0.04, theta=0.05, kappa=4.0, rho=-0.5, volvol=0.4),
                 sv.HestonParams(v0=0.09, theta=0.06, kappa=2.0, rho=0.3, volvol=0.8), sv.BTC_HESTON_PARAMS]
        many = sv.heston_mc_chain_pricer_conditional_many(plist, nb_path=n, seeds=seeds, return_stats=True, **ID_CHAIN)
        singles = [sv.heston_mc_chain_pricer_conditional(v0=p.v0, theta=p.theta, kappa=p.kappa, rho=p.rho, volvol=p.volvol, nb_path=n,
                                                         seed=s, return_stats=True, **ID_CHAIN) for p, s in zip(plist, seeds)]
        oc = sv.OptionChain(ids=np.array(["a", "b"]), **ID_CHAIN)
        routed = sv.HestonPricer().model_mc_price_chain_conditional_many(oc, plist[:2], nb_path=n, seeds=seeds[:2])
    assert len(many) == 3 and len(routed) == 2 and len(routed[0]) == 2
    for j, (got, want) in enumerate(zip(many, singles)):
        for a in range(2):
            for i in range(2):
                assert np.array_equal(got[a][i], want[a][i]), (j, a, i)
        assert got[2] == want[2], j
    for j in range(2):
        for i in range(2):
            assert np.array_equal(routed[j][0][i], many[j][0][i]) and np.array_equal(routed[j][1][i], many[j][1][i])


def test_a_quote_does_not_depend_on_what_shares_the_call():
    greeks, _, kw, wrt, _ = routes("logsv")
    n, seed = 4096, 9
    full = greeks(nb_path=n, seed=seed, wrt=wrt, **ID_CHAIN, **kw)
    few = dict(ID_CHAIN, strikes_ttms=[ID_STRIKES[3:4], ID_STRIKES[1:2]], optiontypes_ttms=[np.array(["C"]), np.array(["P"])])
    alone = greeks(nb_path=n, seed=seed, wrt=wrt[1:], **few, **kw)
    for key in ("sens", "sens_stderr", "n_pairs"):
        assert np.array_equal(alone[key]["volvol"][0], full[key]["volvol"][0][3:4]), key
        assert np.array_equal(alone[key]["volvol"][1], full[key]["volvol"][1][1:2]), key


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
CAL_TTMS = np.array([1.0 / 12.0, 0.25, 0.5])
CAL_STRIKES = np.round(np.arange(0.8, 1.2001, 0.05), 2)
CAL_CHAIN = dict(ttms=CAL_TTMS, forwards=np.array([1.0, 1.0, 1.0]), discfactors=np.array([0.999, 0.995, 0.99]),
                 strikes_ttms=[np.concatenate([CAL_STRIKES, CAL_STRIKES])] * 3,
                 optiontypes_ttms=[np.array(["C"] * CAL_STRIKES.size + ["P"] * CAL_STRIKES.size)] * 3)


@pytest.mark.parametrize("recenter", [True, False])
def test_the_reported_error_is_the_spread_over_64_seeds(recenter):
    """64 seeds at 4 096 paths, LOGSV_BTC_PARAMS on the 3 x 18 chain: per parameter the median over the priced quotes of (spread of
    sens over the seeds / mean reported error) within the band of a 64-sample deviation (1 / sqrt(126) = 0.089, three of those)"""
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.mc_greeks import LOGSV_GREEK_PARAMS
    p = sv.LOGSV_BTC_PARAMS
    kw = dict(v0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2, beta=p.beta, volvol=p.volvol,
              vol_backbone_etas=p.get_vol_backbone_etas(ttms=CAL_TTMS))
    runs = [sv.logsv_mc_chain_greeks_conditional(nb_path=4096, seed=1000 + s, recenter=recenter, wrt=None, **CAL_CHAIN, **kw)
            for s in range(64)]
    priced = np.concatenate([np.mean([r["price"][i] for r in runs], axis=0) > 1e-3 * CAL_CHAIN["discfactors"][i] for i in range(3)])
    ok = True
    for name in LOGSV_GREEK_PARAMS:
        vals = np.array([np.concatenate(r["sens"][name]) for r in runs])
        errs = np.array([np.concatenate(r["sens_stderr"][name]) for r in runs])
        ratio = vals.std(axis=0, ddof=1) / errs.mean(axis=0)
        med = float(np.median(ratio[priced]))
        note(f"cmc sens error ratio recenter={recenter} {name}: median over {int(priced.sum())} priced quotes {med:.3f} min "
             f"{ratio[priced].min():.3f} max {ratio[priced].max():.3f} all " + " ".join(f"{v:.2f}" for v in ratio))
        ok = ok and 0.73 <= med <= 1.27
    assert ok


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["logsv", "heston"])
def test_agreement_with_the_plain_estimators_sensitivities(model):
    """2^16 paths, 2 expiries x 5 strikes x 2 parameters: the two estimators run on independent streams (8 and the plain one's), so
    |sens_cond - sens_plain| <= 4 sqrt(se_cond^2 + se_plain^2) on every quote"""
    import stochvolmodels_amd as sv
    greeks, _, kw, wrt, _ = routes(model)
    n, seed = 1 << 16, 41
    if model == "logsv":                                       # (the plain route takes the etas from the parameters: both use those)
        params = sv.LogSvParams(sigma0=kw["v0"], theta=kw["theta"], kappa1=kw["kappa1"], kappa2=kw["kappa2"], beta=kw["beta"],
                                volvol=kw["volvol"])
        plain = sv.logsv_mc_chain_greeks(params=params, nb_path=n, seed=seed, wrt=wrt, **ID_CHAIN)
        kw = dict(kw, vol_backbone_etas=params.get_vol_backbone_etas(ttms=ID_CHAIN["ttms"]))
    else:
        plain = sv.heston_mc_chain_greeks(params=sv.HestonParams(**kw), nb_path=n, seed=seed, wrt=wrt, **ID_CHAIN)
    cond = greeks(nb_path=n, seed=seed, wrt=wrt, **ID_CHAIN, **kw)
    record = dict(model=model, n_path=n, seed=seed, quotes=[])
    ok = True
    for name in wrt:
        for i in range(2):
            se = np.hypot(cond["sens_stderr"][name][i], plain["sens_stderr"][name][i])
            z = (cond["sens"][name][i] - plain["sens"][name][i]) / se
            ratio = (plain["sens_stderr"][name][i] / cond["sens_stderr"][name][i]) ** 2
            print(f"cmc sens vs plain {model} {name} expiry {i}: z " + " ".join(f"{v:+.2f}" for v in z) + " variance ratio "
                  + " ".join(f"{v:.1f}" for v in ratio))
            record["quotes"].append(dict(param=name, expiry=i, z=z.tolist(), variance_ratio=ratio.tolist(),
                                         sens_cond=cond["sens"][name][i].tolist(), sens_plain=plain["sens"][name][i].tolist()))
            ok = ok and bool(np.all(np.abs(z) <= 4.0))
    if os.environ.get("SVMC_CMC_SENS_Z_JSON"):
        with open(os.environ["SVMC_CMC_SENS_Z_JSON"], "a") as fh:
            fh.write(json.dumps(record) + "\n")
    assert ok, record
