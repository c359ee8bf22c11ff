"""
Many (sigma, gamma) sets on one set of jump rows, on the CPU (include/svmc_est.h svmc_jump_sets_payoff_chain):

  1. the shift identity the whole row rests on: tests/hawkes_cmc_twin.np_chain at sigma and at sigma = 0 differ by -host_cv / 2 to
     rounding, on the six-slice fixture's grids;
  2. the Python v_qi is hawkes_cmc_twin.host_cv bit for bit, on the fused drivers' step grid;
  3. the twin: tests/tilted_cond_twin.estimator on (a - v / 2, v) with the corr of the rows (a, 0);
  4. every refusal of the routes is raised with no engine asked for;
  5. the header declares the two names, the binding has them, tc_keep_cmc is shared and not redefined;
  6. the routes on the twin engine: shapes, the 16-set chunking, one stepping call; and the calibration with
     estimator="conditional" recovers (sigma*, gamma*) -- |x_fit - x*| and the final objective are printed, and recorded in
     profiles/hawkes_jump_sets_observed_tolerances.txt: the GPU test of the same fit is held to ten times that.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
for _p in (ROOT, _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import hawkes_cmc_twin as hc  # noqa: E402
import hawkes_twin as ht  # noqa: E402
import jump_sets_twin as js  # noqa: E402
import mc_steps_worker as mw  # noqa: E402
import tilted_cond_twin as tc  # noqa: E402

EPS = 2.0 ** -52
CHAIN = dict(ttms=np.array([0.25, 0.5]), forwards=np.array([1.0, 1.02]), discfactors=np.array([1.0, 0.99]),
             strikes_ttms=[np.array([[0.9, 1.0, 1.1]]), np.array([1.0])], optiontypes_ttms=[np.array([["C", "P", "C"]]), np.array(["P"])])
# the calibration of item 6: what the GPU test repeats on the device
CAL_TTMS, CAL_SPY, CAL_N, CAL_SEED = np.array([1.0 / 52.0, 1.0 / 12.0]), 480, 4096, 2026
CAL_MONEYNESS = (-1.0, -0.5, 0.0, 0.5, 1.0)
CAL_TRUE, CAL_START = (0.4, -2.0), (0.6, 1.0)              # (sigma, gamma): the market's, the start's


class Two:
    world, rank = 2, 0


def hawkes_params(name="hawkes_mc"):
    g = np.load(os.path.join(os.path.dirname(hc.FIXTURE), name + ".npz"))
    return dict(zip(ht.PARAM_NAMES, (float(v) for v in g["params"])))


def model_kw(p):
    return {k: v for k, v in p.items() if k != "sigma"}


@pytest.fixture
def twin_engine(monkeypatch):
    from stochvolmodels_amd.pricers import hawkes_jd_pricer
    from stochvolmodels_amd.utils import mc_payoffs
    engines = {}

    def get(n, *a, **k):
        get.requests.append(int(n))
        return engines.setdefault(int(n), js.TwinEngine(int(n)))
    get.requests, get.engines = [], engines
    for mod in (hawkes_jd_pricer, mc_payoffs):
        monkeypatch.setattr(mod, "get_engine", get)
    monkeypatch.setattr(hawkes_jd_pricer, "DeviceBuffer", js.HostBuffer)
    return get


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
def test_the_rows_at_sigma_and_at_zero_differ_by_half_the_variance():
    fx = mw.Fixture(hc.FIXTURE)
    m = fx.meta
    runs, worst = {}, 0.0
    for c in fx.cases:
        runs.setdefault((c["set"], c["offset"]), c)
    assert len(runs) == 4
    for (sname, offset), c in runs.items():
        p = dict(c["params"])
        assert p["sigma"] > 0.0
        with_sigma = hc.np_chain(p, c["seed"], c["n"], m["steps"], m["dts"], offset)
        zero = hc.np_chain(dict(p, sigma=0.0), c["seed"], c["n"], m["steps"], m["dts"], offset)
        v = hc.host_cv(p["sigma"], m["steps"], m["dts"])
        total, scale = 0, 1.0
        for i, ((mu, lp, lm), (a, lp0, lm0)) in enumerate(zip(with_sigma, zero)):
            assert np.array_equal(lp, lp0) and np.array_equal(lm, lm0)         # the intensities, hence the jumps, do not see sigma
            total += m["steps"][i]
            scale = max(scale, float(np.max(np.abs(mu))), float(np.max(np.abs(a))))
            dev = float(np.max(np.abs(mu.astype(np.longdouble) - (a.astype(np.longdouble) - np.longdouble(v[i]) / 2))))
            bound = (total + 2) * EPS * scale
            worst = max(worst, dev / bound)
            print(f"{sname} offset {offset} expiry {i}: max |mu_sigma - (a - v/2)| = {dev:.3e}  bound {bound:.3e}")
            assert dev <= bound, (sname, offset, i, dev, bound)
            # a wrong sign or a missing v / 2 is far outside
            assert float(np.max(np.abs(mu - (a + v[i] / 2)))) > 1e3 * bound or v[i] < 1e3 * bound
    print(f"largest deviation / bound: {worst:.3f}")


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def test_the_python_variances_are_host_cv_bit_for_bit():
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    for ttms, spy in ((hc.STAT_TTMS, hc.STAT_SPY), ((1.0 / 365.0, 0.1, 0.25, 1.0, 2.5), 1800), (np.linspace(0.05, 1.7, 17), 28800)):
        nbs, dts = hp.jump_step_grid(ttms, spy)
        t0 = 0.0
        for t, nb, dt in zip(ttms, nbs, dts):                              # engine.step_hawkesjd_chain_cond_rows' grid
            d = float(t) - t0
            assert nb == int(d * float(spy)) + 1 and dt == (d if nb == 1 else d / float(nb))
            t0 = float(t)
        for sigma in (0.0, 0.1, 0.45, 1.0 / 3.0, 1.5):
            got = hp.jump_sets_variances(sigma, nbs, dts)
            assert got.dtype == np.float64 and np.array_equal(got, hc.host_cv(sigma, nbs, dts))
    rows = hp.HawkesJumpRows(js.TwinEngine(8), js.HostBuffer(16), [0.1, 0.3], [49, 97], [0.1 / 49, 0.2 / 97], 1, 0)
    assert np.array_equal(rows.variances(0.45), hc.host_cv(0.45, [49, 97], [0.1 / 49, 0.2 / 97])) and rows.n_expiries == 2
    with pytest.raises(ValueError):
        hp.jump_step_grid([0.1], 0)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_the_twin_is_the_tilted_twin_on_shifted_rows():
    rng = np.random.default_rng(5)
    a = 0.2 * rng.standard_normal(513) - 0.03
    k, t = np.array([0.8, 1.0, 1.3, 1.3]), np.array(["P", "C", "C", "P"])
    for v in (0.0, 1e-4, 0.04):
        for gamma in (-3.0, 0.0, 0.5):
            mu, cv = js.rows_of(a, v)
            want = tc.estimator(mu, cv, 1.3, k, t, gamma, recenter=False)
            got = js.estimator(a, v, 1.3, k, t, gamma, recenter=False)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2]["corr"] == 0
            # recentred: the corr of the rows (a, 0), the same number whatever (v, gamma) are; the tilted twin's own differs by rounding
            rec = js.estimator(a, v, 1.3, k, t, gamma, recenter=True)
            assert rec[2]["corr"] == js.corr_of(a, 1.3, True) == tc.corr_of(a, np.zeros(a.size), 1.3, True)
            own = tc.estimator(mu, cv, 1.3, k, t, gamma, recenter=True)
            assert abs(float(rec[2]["corr"] - own[2]["corr"])) <= 8 * EPS * 1.3
            np.testing.assert_allclose(rec[0].astype(float), own[0].astype(float), rtol=0, atol=1e-14)
    # W = c w with c = exp(g (g - 1) v / 2): the weight the header states
    mu, cv = js.rows_of(a, 0.04)
    w = tc.path_terms(mu, cv, 1.0, 1.0, False, 3.0)[0]
    np.testing.assert_allclose((w / (np.exp(np.longdouble(3.0) * a) * np.exp(np.longdouble(3.0 * 2.0 * 0.04 / 2)))).astype(float), 1.0,
                               rtol=1e-15)
    # a = 120 overflows W^2 at gamma 3 alone
    a2 = a.copy()
    a2[7] = 120.0
    for gamma, dropped in ((-3.0, 0), (0.0, 0), (0.5, 0), (3.0, 1)):
        assert js.estimator(a2, 0.04, 1.0, k, t, gamma)[2]["n_dropped"] == dropped


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def option_chain(sv, chain=CHAIN):
    flat = dict(chain, strikes_ttms=[np.ravel(k) for k in chain["strikes_ttms"]],
                optiontypes_ttms=[np.ravel(t) for t in chain["optiontypes_ttms"]])
    return sv.OptionChain(ids=np.array(["a", "b"]), **flat)


def test_the_routes_refuse_before_any_engine_is_asked_for(twin_engine):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import VariableType
    kw = sv.HawkesJDParams().to_dict()
    kw.pop("risk_premia_gamma")
    kw.pop("sigma")
    ic = dict(CHAIN, optiontypes_ttms=[np.array([["IC", "C", "C"]]), np.array(["P"])])
    ip = dict(CHAIN, optiontypes_ttms=[np.array([["C", "C", "C"]]), np.array(["IP"])])
    fn = sv.hawkesjd_mc_chain_pricer_conditional_sets
    sets = ([0.3, 0.4], [-1.0, 1.0])
    for inverse in (ic, ip):
        with pytest.raises(ValueError, match="not implemented"):
            fn(*sets, nb_path=64, seed=1, **inverse, **kw)
    for vt in (VariableType.Q_VAR, VariableType.SIGMA):
        with pytest.raises(NotImplementedError):
            fn(*sets, nb_path=64, seed=1, variable_type=vt, **CHAIN, **kw)
    with pytest.raises(NotImplementedError):
        fn(*sets, nb_path=64, seed=1, comm=Two(), **CHAIN, **kw)
    with pytest.raises(NotImplementedError):
        fn(*sets, nb_path=64, seed=1, devices=2, **CHAIN, **kw)
    for bad in (([0.3], [1.0, 2.0]), ([], []), ([-0.1], [0.0]), ([np.nan], [0.0]), ([np.inf], [0.0]), ([0.3], [np.nan]), ([0.3], [np.inf])):
        with pytest.raises(ValueError):
            fn(*bad, nb_path=64, seed=1, **CHAIN, **kw)
    for shard in (dict(comm=Two()), dict(devices=[0, 0])):
        with pytest.raises(NotImplementedError):
            sv.hawkesjd_jump_rows(CHAIN["ttms"], nb_path=64, seed=1, **kw, **shard)
    pricer, params = sv.HawkesJDPricer(), sv.HawkesJDParams(risk_premia_gamma=0.5)
    route = pricer.model_mc_price_chain_conditional_sets
    with pytest.raises(ValueError, match="not implemented"):
        route(option_chain(sv, ic), params, *sets, nb_path=64, seed=1)
    with pytest.raises(NotImplementedError):
        route(option_chain(sv), params, *sets, nb_path=64, seed=1, variable_type=VariableType.Q_VAR)
    with pytest.raises(NotImplementedError):
        route(option_chain(sv), params, *sets, nb_path=64, seed=1, comm=Two())
    with pytest.raises(NotImplementedError):
        route(option_chain(sv), params, *sets, nb_path=64, seed=1, devices=[0, 0])
    with pytest.raises(ValueError):
        route(option_chain(sv), params, [0.3], [1.0, 2.0], nb_path=64, seed=1)
    # the calibration keyword: another estimator, and the conditional mode's refusals
    chain = option_chain(sv, dict(CHAIN, bid_ivs=[np.full(3, 0.4), np.full(1, 0.4)], ask_ivs=[np.full(3, 0.5), np.full(1, 0.5)]))
    with pytest.raises(ValueError, match="estimator"):
        pricer.risk_premia_calibration_objective(chain, params, estimator="plain")
    with pytest.raises(ValueError, match="estimator"):
        pricer.calibrate_risk_premia_gamma_to_chain(chain, params, estimator="mc", print_iter=False, disp=False)
    for shard in (dict(comm=Two()), dict(devices=[0, 0])):
        with pytest.raises(NotImplementedError):
            pricer.risk_premia_calibration_objective(chain, params, estimator="conditional", nb_path=64, seed=1, **shard)
    inverse = option_chain(sv, dict(ic, bid_ivs=[np.full(3, 0.4), np.full(1, 0.4)], ask_ivs=[np.full(3, 0.5), np.full(1, 0.5)]))
    with pytest.raises(ValueError, match="not implemented"):
        pricer.risk_premia_calibration_objective(inverse, params, estimator="conditional", nb_path=64, seed=1)
    a = np.zeros(64)
    host = sv.compute_mc_vars_payoff_jump_sets
    with pytest.raises(ValueError, match="not implemented"):
        host(a, [0.04], [0.5], 1.0, np.array([1.0]), np.array(["IC"]))
    for bad in (([0.04], [0.5, 1.0]), ([], []), ([-1.0], [0.0]), ([np.nan], [0.0]), ([0.04], [np.inf])):
        with pytest.raises(ValueError):
            host(a, *bad, 1.0, np.array([1.0]), np.array(["C"]))
    with pytest.raises(ValueError):
        host(np.zeros(0), [0.04], [0.5], 1.0, np.array([1.0]), np.array(["C"]))
    assert twin_engine.requests == []
    # ... and a handle refuses what a call on it cannot serve, before its engine is used
    rows = sv.hawkesjd_jump_rows(CHAIN["ttms"], nb_path=64, seed=1, nb_steps_per_year=40, **kw)
    eng = twin_engine.engines[64]
    assert twin_engine.requests == [64] and eng.stepping_calls == 1
    for bad in (([0.3], [1.0, 2.0]), ([-0.1], [0.0]), ([0.3], [np.nan])):
        with pytest.raises(ValueError):
            rows.price_sets(*bad, CHAIN["forwards"], CHAIN["strikes_ttms"], CHAIN["optiontypes_ttms"])
    with pytest.raises(ValueError, match="not implemented"):
        rows.price_sets([0.3], [1.0], CHAIN["forwards"], CHAIN["strikes_ttms"], ic["optiontypes_ttms"])
    with pytest.raises(ValueError):
        rows.price_sets([0.3], [1.0], CHAIN["forwards"][:1], CHAIN["strikes_ttms"][:1], CHAIN["optiontypes_ttms"][:1])
    assert eng.tail_calls == 0


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_two_names_and_the_binding_has_them():
    from stochvolmodels_amd import _lib, engine
    text = open(os.path.join(ROOT, "include", "svmc_est.h")).read()
    declared = set(re.findall(r"SVMC_EST_API\s+int\s+(svmc_[a-z0-9_]+)\s*\(", text))
    names = {"svmc_jump_sets_workspace_bytes", "svmc_jump_sets_payoff_chain"}
    assert names <= declared
    assert re.search(r"#define SVMC_JUMP_SETS_MAX 16\b", text) and engine.JUMP_SETS_MAX == 16
    assert re.search(r"#define SVMC_EST_VERSION 100\b", text)
    E = _lib.load_est()
    assert names <= set(E._svmc_est_symbols) and set(E._svmc_est_symbols) == declared
    assert E.svmc_jump_sets_payoff_chain.restype is C.c_int and len(E.svmc_jump_sets_payoff_chain.argtypes) == 19
    assert len(E.svmc_jump_sets_workspace_bytes.argtypes) == 5
    # the declaration's own argument count
    decl = re.search(r"SVMC_EST_API\s+int\s+svmc_jump_sets_payoff_chain\s*\(([^;]*)\);", text).group(1)
    assert len(decl.split(",")) == 19
    assert callable(engine.HipEngine.jump_sets_payoffs) and callable(engine.HipEngine.step_hawkesjd_jump_rows)
    import stochvolmodels_amd as sv
    for name in ("hawkesjd_jump_rows", "HawkesJumpRows", "hawkesjd_mc_chain_pricer_conditional_sets", "compute_mc_vars_payoff_jump_sets"):
        assert callable(getattr(sv, name))
    assert callable(sv.HawkesJDPricer.model_mc_price_chain_conditional_sets)
    # the kernels: no existing kernel's name is a prefix of a new one's, and the source shares row f11's rule, not a copy of it
    src = open(os.path.join(ROOT, "stochvolmodels_amd", "csrc", "svmc_est.hip")).read()
    kernels = re.findall(r"__global__[^\n]*void (\w+)\(", src)
    new = [k for k in kernels if k.startswith("jump_sets_")]
    assert sorted(new) == ["jump_sets_finish_kernel", "jump_sets_forward_finish_kernel", "jump_sets_forward_kernel", "jump_sets_payoff_kernel"]
    for k in new:
        assert not any(k.startswith(old) for old in kernels if old not in new), k
    assert "tc_keep_cmc(a, 0.0" in src and "bool tc_keep_cmc" not in src and "tc_forward_finish_body(" in src and "tc_black(" in src


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def test_the_routes_on_the_twin_engine(twin_engine):
    import stochvolmodels_amd as sv
    p = hawkes_params()
    kw = model_kw(p)
    n, spy, seed = 257, 40, 11
    sigmas, gammas = np.linspace(0.1, 0.9, 17), np.linspace(-3.0, 3.0, 17)
    prices, errs, fw = sv.hawkesjd_mc_chain_pricer_conditional_sets(sigmas, gammas, nb_path=n, nb_steps_per_year=spy, seed=seed,
                                                                    recenter_forward=True, return_forwards=True, **CHAIN, **kw)
    eng = twin_engine.engines[n]
    assert eng.stepping_calls == 1 and eng.sets_per_call == [16, 1]
    assert len(prices) == len(errs) == len(fw) == 17
    nbs, dts = [11, 11], [0.25 / 11, 0.25 / 11]
    a = [st[0] for st in hc.np_chain(dict(p, sigma=0.0), seed, n, nbs, dts)]
    for q in (0, 5, 16):
        v = hc.host_cv(sigmas[q], nbs, dts)
        for i in range(2):
            want = js.estimator(a[i], v[i], CHAIN["forwards"][i], CHAIN["strikes_ttms"][i], CHAIN["optiontypes_ttms"][i], gammas[q], True)
            assert prices[q][i].shape == CHAIN["strikes_ttms"][i].shape
            assert np.array_equal(prices[q][i].ravel(), want[0].astype(float)) and np.array_equal(errs[q][i].ravel(), want[1].astype(float))
            norm, gf, st = fw[q]
            assert st.shape == (2, 8) and norm[i] == float(want[2]["normalizer"]) and gf[i] == float(want[2]["gamma_forward"])
    # the rows at sigma = 0 price the chain the existing estimator prices at sigma, to the identity of item 1
    q = 5
    mu = [st[0] for st in hc.np_chain(dict(p, sigma=float(sigmas[q])), seed, n, nbs, dts)]
    v = hc.host_cv(sigmas[q], nbs, dts)
    for i in range(2):
        ref = tc.estimator(mu[i], np.full(n, v[i]), CHAIN["forwards"][i], CHAIN["strikes_ttms"][i], CHAIN["optiontypes_ttms"][i], gammas[q])
        got = js.estimator(a[i], v[i], CHAIN["forwards"][i], CHAIN["strikes_ttms"][i], CHAIN["optiontypes_ttms"][i], gammas[q])
        dev = float(np.max(np.abs(got[0] - ref[0])))
        print(f"expiry {i}: shifted rows against the rows at sigma: {dev:.3e}")
        assert dev <= 1e-10 * CHAIN["forwards"][i]
    # the pricer's method and the host-array route
    chain = option_chain(sv)
    got = sv.HawkesJDPricer().model_mc_price_chain_conditional_sets(chain, sv.HawkesJDParams(**p), sigmas[:2], gammas[:2], nb_path=n,
                                                                    nb_steps_per_year=spy, seed=seed, recenter_forward=True)
    for q in range(2):
        for i in range(2):
            assert np.array_equal(got[0][q][i], prices[q][i].ravel())
    rng = np.random.default_rng(3)
    row = 0.2 * rng.standard_normal(64)
    k, t = np.array([[0.9, 1.1]]), np.array([["P", "C"]])
    hp_, he_, hs_ = sv.compute_mc_vars_payoff_jump_sets(row, [0.0, 0.04], [0.5, -1.0], 1.1, k, t, recenter=True, return_stats=True)
    for q, (v, g) in enumerate(((0.0, 0.5), (0.04, -1.0))):
        want = js.estimator(row, v, 1.1, k, t, g, True)
        assert hp_[q].shape == k.shape and np.array_equal(hp_[q].ravel(), want[0].astype(float))
        assert np.array_equal(he_[q].ravel(), want[1].astype(float))
        assert hs_[q]["n_kept"] == 64 and hs_[q]["corr"] == float(want[2]["corr"])


def cal_chain(sv, vols=None):
    p = hawkes_params()
    sds = [hc.total_std(p, t) for t in CAL_TTMS]
    strikes = [np.exp(np.array(CAL_MONEYNESS) * sd) for sd in sds]
    types = [np.where(k <= 1.0, "P", "C") for k in strikes]
    vols = [np.full(5, 0.5)] * 2 if vols is None else vols
    return sv.OptionChain(ttms=CAL_TTMS, forwards=np.ones(2), discfactors=np.ones(2), strikes_ttms=strikes, optiontypes_ttms=types,
                          bid_ivs=[v.copy() for v in vols], ask_ivs=[v.copy() for v in vols], ids=np.array(["w", "m"]))


def market_vols(sv, pricer, params, **mc):
    """the vols of the route's own prices at CAL_TRUE, inverted against its gamma forwards: the calibration's market"""
    chain = cal_chain(sv)
    prices, _, fw = pricer.model_mc_price_chain_conditional_sets(chain, params, [CAL_TRUE[0]], [CAL_TRUE[1]], return_forwards=True, **mc)
    return chain.compute_model_ivols_from_chain_data(model_prices=prices[0], forwards=fw[0][1])


def test_calibration_on_the_twin_recovers_sigma_and_gamma(twin_engine):
    import stochvolmodels_amd as sv
    pricer = sv.HawkesJDPricer()
    p = hawkes_params()
    mc = dict(nb_path=CAL_N, nb_steps_per_year=CAL_SPY, seed=CAL_SEED)
    vols = market_vols(sv, pricer, sv.HawkesJDParams(**p), **mc)
    assert all(np.all(np.isfinite(v)) for v in vols)
    chain = cal_chain(sv, vols)
    params0 = sv.HawkesJDParams(**dict(p, sigma=CAL_START[0]), risk_premia_gamma=CAL_START[1])
    eng = twin_engine.engines[CAL_N]
    before = eng.stepping_calls
    fit = pricer.calibrate_risk_premia_gamma_to_chain(chain, params0, estimator="conditional", print_iter=False, disp=False, **mc)
    last = pricer.last_calibration
    assert fit is params0 and last["estimator"] == "conditional" and last["n_stepping_calls"] == 1
    assert eng.stepping_calls == before + 1                    # ONE stepping call for the whole fit
    assert last["n_gradient_batches"] > 0 and set(eng.sets_per_call[-2 * last["n_gradient_batches"]:]) <= {1, 2, 3}
    err = np.abs(np.array([fit.sigma, fit.risk_premia_gamma]) - np.array(CAL_TRUE))
    print(f"twin calibration: x_fit = ({fit.sigma!r}, {fit.risk_premia_gamma!r})  |x_fit - x*| = ({err[0]:.3e}, {err[1]:.3e})  "
          f"objective {last['objective']:.3e}  nit {last['nit']}  n_eval {last['n_eval']}  status {last['status']}")
    # The figures are RECORDED, not bounded here (profiles/hawkes_jump_sets_observed_tolerances.txt; the device's fit is held to ten
    # times them): with the objective's own options -- the reference's forward-difference step 0.025 -- SLSQP ends at its iteration
    # limit some way off x*, in either mode.  What must hold exactly: the market is the route's own, so the objective at x* is 0;
    # the fit is inside the bounds and no worse than the start.
    from stochvolmodels_amd.pricers.hawkes_jd_pricer import RISK_PREMIA_BOUNDS, RISK_PREMIA_GAMMA_SCALER
    objective = pricer.risk_premia_calibration_objective(chain, params0, estimator="conditional", print_iter=False, **mc)
    x_true = np.array([CAL_TRUE[0], CAL_TRUE[1] / RISK_PREMIA_GAMMA_SCALER])
    assert objective(x_true) == 0.0
    at_start = objective(np.array([CAL_START[0], CAL_START[1] / RISK_PREMIA_GAMMA_SCALER]))
    assert np.isfinite(last["objective"]) and last["objective"] < at_start
    for x, (lo, hi) in zip(last["x"], RISK_PREMIA_BOUNDS):
        assert lo <= x <= hi
    # the Fourier mode's keys plus the two of this mode
    assert set(last) == {"n_eval", "n_gradient_batches", "objective", "success", "status", "message", "nit", "nfev", "x", "estimator",
                         "n_stepping_calls"}
