"""
The Python routes of the conditional Monte Carlo Greeks under the exponential risk-premia kernel on FakeEngine.
No GPU: the refusals before any engine is asked for, what is handed to the engine, the shapes, one gamma = the list form.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from fake_engine import FakeEngine  # noqa: E402

CHAIN = dict(ttms=np.array([0.25, 0.5]), forwards=np.array([1.0, 1.02]), discfactors=np.array([1.0, 0.99]),
             strikes_ttms=[np.array([[0.9, 1.0, 1.1]]), np.array([1.0])], optiontypes_ttms=[np.array([["C", "P", "C"]]), np.array(["P"])])
TEN = ("price", "stderr", "delta", "delta_stderr", "dual_delta", "dual_delta_stderr", "gamma", "gamma_stderr", "dual_gamma",
       "dual_gamma_stderr")


class Two:
    world, rank = 2, 0


class Recorder(FakeEngine):
    """the fake engine with the calls of row f18 recorded; field r of gamma g at strike k is 1000 g + 100 r + k"""

    class _Buf:
        def __init__(self, n):
            self.a = np.zeros(n)
            self.ptr = self.a.ctypes.data

    def __init__(self, n_path):
        super().__init__(n_path)
        self.x, self.cv = self._Buf(n_path), self._Buf(n_path)

    def upload(self, ptr, host):
        import ctypes as C
        host = np.ascontiguousarray(host, dtype=np.float64)
        C.memmove(ptr, host.ctypes.data, host.nbytes)

    @staticmethod
    def _fields(ch, first, names):
        G, K, offs = ch["gammas"].size, ch["total"], ch["offs"]
        return [{name: [(1000.0 * g + 100.0 * (first + r) + np.arange(K))[int(offs[i]):int(offs[i + 1])].reshape(ch["shapes"][i])
                        for i in range(ch["m"])] for r, name in enumerate(names)} for g in range(G)]

    def price_hawkesjd_chain_tilted_cond_greeks(self, ch, params, nb_steps_per_year, seed, call_id, gammas, recenter):
        self.calls.append(("greeks", ch, np.array(params), nb_steps_per_year, seed, call_id, np.array(gammas), recenter))
        G, m = len(gammas), ch["m"]
        return self._fields(dict(ch, gammas=np.asarray(gammas)), 0, TEN), np.arange(G * m * 9, dtype=np.float64).reshape(G, m, 9)

    def tilted_conditional_payoffs(self, forwards, strikes, codes, gammas, recenter=False, mu_rows=None, cv_rows=None, shifts=None):
        from stochvolmodels_amd.engine import tilted_chain_arrays
        ch = tilted_chain_arrays(forwards, strikes, codes, gammas)
        self.calls.append(("payoff_tail", ch, recenter, mu_rows, cv_rows, self.x.a.copy(), self.cv.a.copy()))
        f = self._fields(ch, 0, TEN[:2])
        return [d["price"] for d in f], [d["stderr"] for d in f], np.arange(ch["gammas"].size * 8, dtype=np.float64).reshape(-1, 1, 8)

    def tilted_conditional_greeks(self, forwards, strikes, codes, gammas, recenter=False, mu_rows=None, cv_rows=None):
        from stochvolmodels_amd.engine import tilted_chain_arrays
        ch = tilted_chain_arrays(forwards, strikes, codes, gammas)
        self.calls.append(("greeks_tail", ch, recenter, mu_rows, cv_rows, self.x.a.copy(), self.cv.a.copy()))
        return self._fields(ch, 2, TEN[2:]), -np.arange(ch["gammas"].size * 4, dtype=np.float64).reshape(-1, 1, 4)


@pytest.fixture
def fake(monkeypatch):
    from stochvolmodels_amd.pricers import hawkes_jd_pricer
    from stochvolmodels_amd.utils import mc_payoffs
    eng = Recorder(64)
    eng.requests = []
    for mod in (hawkes_jd_pricer, mc_payoffs):
        monkeypatch.setattr(mod, "get_engine", lambda n, *a, **k: eng.requests.append(n) or eng)
    return eng


def option_chain(sv, chain=CHAIN):
    """(an OptionChain's slices are one-dimensional)"""
    flat = dict(chain, strikes_ttms=[np.ravel(k) for k in chain["strikes_ttms"]],
                optiontypes_ttms=[np.ravel(t) for t in chain["optiontypes_ttms"]])
    return sv.OptionChain(ids=np.array(["a", "b"]), **flat)


def test_the_names_are_exported():
    import stochvolmodels_amd as sv
    for name in ("hawkesjd_mc_chain_greeks_conditional_with_risk_premia", "hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas",
                 "compute_mc_vars_greeks_conditional_with_gamma"):
        assert callable(getattr(sv, name))
    assert callable(sv.HawkesJDPricer.model_mc_chain_greeks_conditional_with_risk_premia)
    assert callable(sv.HawkesJDPricer.get_log_return_mc_pdf_conditional_under_risk_kernel)
    from stochvolmodels_amd import engine
    assert tuple(TEN) == engine.CMC_GREEKS_FIELDS == ("price", "stderr") + engine.TCG_FIELDS
    assert engine.TILTED_COND_GREEKS_STATS_FIELDS == engine.TILTED_COND_STATS_FIELDS + ("n_zero_cv",)
    assert callable(engine.HipEngine.tilted_conditional_greeks)


def test_the_routes_refuse_before_any_engine_is_asked_for(fake):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import VariableType
    kw = sv.HawkesJDParams().to_dict()
    kw.pop("risk_premia_gamma")
    ic = dict(CHAIN, optiontypes_ttms=[np.array([["IC", "C", "C"]]), np.array(["P"])])
    ip = dict(CHAIN, optiontypes_ttms=[np.array([["C", "C", "C"]]), np.array(["IP"])])
    many = sv.hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas
    one = sv.hawkesjd_mc_chain_greeks_conditional_with_risk_premia
    for fn, g in ((many, dict(risk_premia_gammas=[-1.0, 1.0])), (one, dict(risk_premia_gamma=-1.0))):
        for inverse in (ic, ip):
            with pytest.raises(ValueError, match="not implemented"):
                fn(nb_path=64, seed=1, **inverse, **kw, **g)
        for vt in (VariableType.Q_VAR, VariableType.SIGMA):
            with pytest.raises(NotImplementedError):
                fn(nb_path=64, seed=1, variable_type=vt, **CHAIN, **kw, **g)
        with pytest.raises(NotImplementedError):
            fn(nb_path=64, seed=1, comm=Two(), **CHAIN, **kw, **g)
        with pytest.raises(NotImplementedError):
            fn(nb_path=64, seed=1, devices=2, **CHAIN, **kw, **g)
        for wrt in (None, "all", ["sigma"]):
            with pytest.raises(NotImplementedError, match="wrt"):
                fn(nb_path=64, seed=1, wrt=wrt, **CHAIN, **kw, **g)
    for bad in ([], [0.0] * 17, [np.nan]):
        with pytest.raises(ValueError):
            many(nb_path=64, seed=1, risk_premia_gammas=bad, **CHAIN, **kw)
    with pytest.raises(ValueError, match="risk_premia_gamma must be set"):
        one(nb_path=64, seed=1, **CHAIN, **kw)
    pricer, params = sv.HawkesJDPricer(), sv.HawkesJDParams(risk_premia_gamma=0.5)
    route = pricer.model_mc_chain_greeks_conditional_with_risk_premia
    with pytest.raises(ValueError, match="risk_premia_gamma must be set"):
        route(option_chain(sv), sv.HawkesJDParams(), nb_path=64, seed=1)
    with pytest.raises(ValueError, match="not implemented"):
        route(option_chain(sv, ic), params, nb_path=64, seed=1)
    with pytest.raises(NotImplementedError):
        route(option_chain(sv), params, nb_path=64, seed=1, variable_type=VariableType.Q_VAR)
    with pytest.raises(NotImplementedError):
        route(option_chain(sv), params, nb_path=64, seed=1, comm=Two())
    with pytest.raises(NotImplementedError):
        route(option_chain(sv), params, nb_path=64, seed=1, devices=[0, 0])
    with pytest.raises(NotImplementedError, match="wrt"):
        route(option_chain(sv), params, nb_path=64, seed=1, wrt=["sigma"])
    with pytest.raises(ValueError):
        pricer.get_log_return_mc_pdf_conditional_under_risk_kernel(params, 0.25, np.linspace(-1, 1, 5), [], nb_path=64, seed=1)
    mu, cv = np.zeros(64), np.full(64, 0.04)
    fn = sv.compute_mc_vars_greeks_conditional_with_gamma
    with pytest.raises(ValueError, match="not implemented"):
        fn(mu, cv, 1.0, np.array([1.0]), np.array(["IC"]), 0.5)
    with pytest.raises(NotImplementedError):
        fn(mu, cv, 1.0, np.array([1.0]), np.array(["C"]), 0.5, variable_type=VariableType.Q_VAR)
    with pytest.raises(ValueError):
        fn(mu, cv[:3], 1.0, np.array([1.0]), np.array(["C"]), 0.5)
    with pytest.raises(ValueError):
        fn(mu, cv, 1.0, np.array([1.0]), np.array(["C"]), [0.0] * 17)
    assert fake.requests == [] and fake.calls == []


def test_what_the_routes_hand_the_engine_and_their_shapes(fake):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import engine
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    params = sv.HawkesJDParams(mu=0.01, sigma=0.3, lambda_p=5.0, lambda_m=7.0, risk_premia_gamma=0.25)
    kw = params.to_dict()
    kw.pop("risk_premia_gamma")
    gammas = [-1.0, 0.0, 2.0]
    out = sv.hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas(nb_path=777, seed=11, risk_premia_gammas=gammas,
                                                                          recenter_forward=True, return_stats=True, **CHAIN, **kw)
    assert fake.requests == [777]
    what, ch, block, spy, seed, call_id, g, recenter = fake.calls[-1]
    assert what == "greeks" and (spy, seed, call_id, recenter) == (hp.NB_STEPS_PER_YEAR, 11, 0, True) and spy == 1800
    assert block.tolist() == [float(params.to_dict()[k]) for k in hp.PARAM_NAMES] and g.tolist() == gammas
    assert ch["ttms"].tolist() == [0.25, 0.5] and ch["forwards"].tolist() == [1.0, 1.02] and ch["offs"].tolist() == [0, 3, 4]
    assert ch["strikes"].tolist() == [0.9, 1.0, 1.1, 1.0] and ch["codes"].tolist() == [0, 1, 0, 1]
    # one dict per gamma: the ten keys, chain-shaped, and "stats" per expiry
    assert len(out) == 3 and all(tuple(d) == TEN + ("stats",) for d in out)
    assert [a.shape for a in out[1]["delta"]] == [(1, 3), (1,)] and out[2]["dual_gamma"][1].tolist() == [2803.0]
    assert out[0]["price"][0].tolist() == [[0.0, 1.0, 2.0]] and out[1]["gamma_stderr"][0].tolist() == [[1700.0, 1701.0, 1702.0]]
    st = out[1]["stats"]
    assert len(st) == 2 and tuple(st[0]) == engine.TILTED_COND_GREEKS_STATS_FIELDS
    assert st[1]["normalizer"] == 27.0 and st[1]["n_zero_cv"] == 35 and isinstance(st[1]["n_zero_cv"], int) and isinstance(st[1]["n_kept"], int)
    # without return_stats ten keys; nb_steps_per_year and the default recenter_forward=False are passed on
    out = sv.hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas(nb_path=777, seed=12, risk_premia_gammas=gammas,
                                                                          nb_steps_per_year=360, **CHAIN, **kw)
    assert all(tuple(d) == TEN for d in out) and fake.calls[-1][3:6] == (360, 12, 0) and fake.calls[-1][7] is False
    # one gamma is the list form at that gamma
    one = sv.hawkesjd_mc_chain_greeks_conditional_with_risk_premia(nb_path=777, seed=11, risk_premia_gamma=2.0, return_stats=True,
                                                                   **CHAIN, **kw)
    assert fake.calls[-1][6].tolist() == [2.0] and fake.calls[-1][3:6] == (1800, 11, 0)
    assert tuple(one) == TEN + ("stats",) and [a.shape for a in one["dual_delta"]] == [(1, 3), (1,)]
    assert one["dual_delta"][0].tolist() == [[400.0, 401.0, 402.0]]
    # without a seed: the process seed and the NEXT call id, once per call
    sv.set_seed(2024)
    sv.hawkesjd_mc_chain_greeks_conditional_with_risk_premia(nb_path=777, risk_premia_gamma=2.0, **CHAIN, **kw)
    first = fake.calls[-1]
    sv.hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas(nb_path=777, risk_premia_gammas=gammas, **CHAIN, **kw)
    assert first[4] == fake.calls[-1][4] == 2024 and fake.calls[-1][5] == first[5] + 1
    # the class route: the chain's arrays, the parameter set's fields and ITS gamma
    d = sv.HawkesJDPricer().model_mc_chain_greeks_conditional_with_risk_premia(option_chain(sv), params, nb_path=777, seed=11,
                                                                               recenter_forward=True)
    assert fake.calls[-1][2].tolist() == block.tolist() and fake.calls[-1][6].tolist() == [0.25] and fake.calls[-1][7] is True
    assert tuple(d) == TEN
    # the density: one expiry at forward 1, calls at exp(x), no recentring, every gamma in one call; pdf = K dual_gamma
    x = np.linspace(-0.5, 0.5, 5).reshape(1, 5)
    pdf, err = sv.HawkesJDPricer().get_log_return_mc_pdf_conditional_under_risk_kernel(params, 0.25, x, [-1.0, 1.0], nb_path=777, seed=3,
                                                                                       return_stderr=True, nb_steps_per_year=360)
    what, ch, block2, spy, seed, call_id, g, recenter = fake.calls[-1]
    assert (what, spy, seed, recenter) == ("greeks", 360, 3, False) and g.tolist() == [-1.0, 1.0] and block2.tolist() == block.tolist()
    assert ch["ttms"].tolist() == [0.25] and ch["forwards"].tolist() == [1.0] and np.array_equal(ch["strikes"], np.exp(x.ravel()))
    assert ch["codes"].tolist() == [0] * 5
    assert pdf.shape == err.shape == (2, 1, 5)
    assert np.array_equal(pdf[1], (np.exp(x.ravel()) * (1800.0 + np.arange(5))).reshape(1, 5))
    assert np.array_equal(err[0], (np.exp(x.ravel()) * (900.0 + np.arange(5))).reshape(1, 5))
    assert sv.HawkesJDPricer().get_log_return_mc_pdf_conditional_under_risk_kernel(params, 0.25, x, [0.5], nb_path=777).shape == (1, 1, 5)


def test_the_host_array_route(fake):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import engine
    rng = np.random.default_rng(5)
    mu, cv = 0.1 * rng.standard_normal(64), 0.04 * rng.random(64)
    k, t = np.array([[0.9, 1.0], [1.1, 1.2]]), np.array([["P", "P"], ["C", "C"]])
    d = sv.compute_mc_vars_greeks_conditional_with_gamma(mu, cv, 1.05, k, t, -1.0, recenter=True, return_stats=True)
    assert fake.requests == [64]
    assert [c[0] for c in fake.calls] == ["payoff_tail", "greeks_tail"]
    for what, ch, recenter, mu_rows, cv_rows, x_up, cv_up in fake.calls:
        assert recenter is True and mu_rows is None and cv_rows is None
        assert np.array_equal(x_up, mu) and np.array_equal(cv_up, cv)
        assert ch["forwards"].tolist() == [1.05] and ch["gammas"].tolist() == [-1.0] and ch["codes"].tolist() == [1, 1, 0, 0]
    assert tuple(d) == TEN + ("stats",) and all(d[f].shape == (2, 2) for f in TEN)
    assert d["price"].tolist() == [[0.0, 1.0], [2.0, 3.0]] and d["dual_gamma"].tolist() == [[800.0, 801.0], [802.0, 803.0]]
    assert tuple(d["stats"]) == engine.TILTED_COND_GREEKS_STATS_FIELDS and d["stats"]["sum_weights"] == 7.0 and d["stats"]["n_zero_cv"] == -3
    # several gammas: a list, one dict per gamma
    ds = sv.compute_mc_vars_greeks_conditional_with_gamma(mu, cv, 1.05, k, t, [-1.0, 2.0])
    assert len(ds) == 2 and tuple(ds[1]) == TEN and ds[1]["delta"].tolist() == [[1200.0, 1201.0], [1202.0, 1203.0]]
    assert fake.calls[-1][1]["gammas"].tolist() == [-1.0, 2.0] and fake.calls[-1][2] is False
