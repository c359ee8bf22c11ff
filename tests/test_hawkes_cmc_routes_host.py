"""
Host checks of the device side of conditional Monte Carlo for the Hawkes jump-diffusion (include/svmc.h): the three
C symbols, the new kernel's metadata in the build beside the counts the earlier rows' tests hold, the refusals of the Python routes
before any engine is asked for, and what the routes hand the engine.  No GPU.
"""
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from fake_engine import FakeEngine  # noqa: E402

SYMBOLS = ("svmc_hawkesjd_chain_cond", "svmc_hawkesjd_chain_price_cmc", "svmc_hawkesjd_chain_price_cmc_greeks")
KERNEL = "hawkes_chain_cond_kernel"
COUNTED_WORDS = ("hawkesjd", "rng_kernel", "cmc", "greeks", "cond_deriv", "cond_vols_")
CHAIN = dict(ttms=np.array([0.25, 0.5]), forwards=np.array([1.0, 1.02]), discfactors=np.array([1.0, 0.99]),
             strikes_ttms=[np.array([0.9, 1.0, 1.1]), np.array([1.0])], optiontypes_ttms=[np.array(["C", "P", "C"]), np.array(["P"])])
GREEKS_FIELDS = ("price", "stderr", "delta", "delta_stderr", "dual_delta", "dual_delta_stderr", "gamma", "gamma_stderr", "dual_gamma",
                 "dual_gamma_stderr")


class Two:
    world, rank = 2, 0


class Recorder(FakeEngine):
    """the fake engine with the two fused conditional calls of the Hawkes routes recorded"""

    def price_hawkesjd_chain_cmc_fused(self, ch, params, nb_steps_per_year, recenter, seed, call_id):
        self.calls.append(("price", ch, np.array(params), nb_steps_per_year, recenter, seed, call_id))
        rows = [np.arange(sl.start, sl.stop, dtype=np.float64) for sl in ch["slices"]]
        return rows, [-r for r in rows], [dict(n_kept=self.n_path) for _ in rows]

    def price_hawkesjd_chain_cmc_greeks_fused(self, ch, params, nb_steps_per_year, recenter, seed, call_id):
        self.calls.append(("greeks", ch, np.array(params), nb_steps_per_year, recenter, seed, call_id))
        fields = {f: [np.full(sl.stop - sl.start, float(r)) for sl in ch["slices"]] for r, f in enumerate(GREEKS_FIELDS)}
        return fields, [dict(n_kept=self.n_path, n_zero_cv=0) for _ in ch["slices"]]


@pytest.fixture
def fake(monkeypatch):
    """the recording engine where the Hawkes routes' get_engine() returns the HipEngine; `requests` lists every get_engine call"""
    from stochvolmodels_amd.pricers import hawkes_jd_pricer
    eng = Recorder(64)
    eng.requests = []
    monkeypatch.setattr(hawkes_jd_pricer, "get_engine", lambda n, *a, **k: eng.requests.append(n) or eng)
    return eng


def option_chain(sv, chain=CHAIN):
    return sv.OptionChain(ids=np.array(["a", "b"]), **chain)


# ---- symbols ------------------------------------------------------------------------------------------------------------------------
def test_the_three_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "svmc.h")).read()
    binding = open(os.path.join(ROOT, "stochvolmodels_amd", "_lib.py")).read()
    for name in SYMBOLS:
        assert re.search(r"SVMC_API int " + name + r"\(", header), name
        assert f'"{name}"' in binding, name
    assert len(re.findall(r"^SVMC_API ", header, flags=re.M)) == 143
    from stochvolmodels_amd import _lib, build
    build.build()
    L = _lib.load()
    assert all(hasattr(L, name) for name in SYMBOLS)
    assert len(L._svmc_symbols) == 143 and set(SYMBOLS) <= set(L._svmc_symbols)
    from stochvolmodels_amd.engine import HipEngine
    for method in ("hawkesjd_chain_cond", "price_hawkesjd_chain_cmc_fused", "price_hawkesjd_chain_cmc_greeks_fused"):
        assert callable(getattr(HipEngine, method)), method


# ---- the build's metadata -----------------------------------------------------------------------------------------------------------
def test_the_new_kernel_uses_no_lds_and_no_scratch_and_the_earlier_counts_hold():
    from stochvolmodels_amd import build
    build.build()
    meta = json.load(open(build.ISA_JSON))["metadata"]
    new = [k for k in meta if KERNEL in k]
    assert len(new) == 1, sorted(meta)
    assert meta[new[0]]["scratch_bytes"] == 0 and meta[new[0]]["lds_bytes"] == 0, meta[new[0]]
    assert not any(word in new[0] for word in COUNTED_WORDS), new[0]
    assert all(v["scratch_bytes"] == 0 for v in meta.values())               # no kernel of the build spills
    assert len([k for k in meta if "hawkesjd" in k]) == 3
    assert len([k for k in meta if "cmc" in k]) == 8
    assert len([k for k in meta if "greeks" in k]) == 2
    assert len([k for k in meta if "cond_deriv" in k]) == 2
    want = json.load(open(os.path.join(HERE, "golden", "stepping_kernel_registers.json")))
    assert {k for k in meta if "rng_kernel" in k} == set(want)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_the_function_routes_refuse_before_any_engine_is_asked_for(fake):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import VariableType
    kw = sv.HawkesJDParams().to_dict()
    ic = dict(CHAIN, optiontypes_ttms=[np.array(["IC", "C", "C"]), np.array(["P"])])
    ip = dict(CHAIN, optiontypes_ttms=[np.array(["C", "C", "C"]), np.array(["IP"])])
    for fn in (sv.hawkesjd_mc_chain_pricer_conditional, sv.hawkesjd_mc_chain_greeks_conditional):
        for inverse in (ic, ip):
            with pytest.raises(ValueError, match="not implemented"):
                fn(nb_path=64, seed=1, **inverse, **kw)
        for vt in (VariableType.Q_VAR, VariableType.SIGMA):
            with pytest.raises(NotImplementedError):
                fn(nb_path=64, seed=1, variable_type=vt, **CHAIN, **kw)
        with pytest.raises(NotImplementedError):
            fn(nb_path=64, seed=1, comm=Two(), **CHAIN, **kw)
        with pytest.raises(NotImplementedError):
            fn(nb_path=64, seed=1, devices=2, **CHAIN, **kw)
    for wrt in (["sigma"], None, "all"):
        with pytest.raises(NotImplementedError, match="wrt"):
            sv.hawkesjd_mc_chain_greeks_conditional(nb_path=64, seed=1, wrt=wrt, **CHAIN, **kw)
    assert fake.requests == [] and fake.calls == []


def test_the_class_routes_refuse_before_any_engine_is_asked_for(fake):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import VariableType
    pricer, params = sv.HawkesJDPricer(), sv.HawkesJDParams()
    inverse = option_chain(sv, dict(CHAIN, optiontypes_ttms=[np.array(["IC", "C", "C"]), np.array(["P"])]))
    for route in (pricer.model_mc_price_chain_conditional, pricer.model_mc_chain_greeks_conditional):
        with pytest.raises(ValueError, match="not implemented"):
            route(inverse, params, nb_path=64, seed=1)
        with pytest.raises(NotImplementedError):
            route(option_chain(sv), params, nb_path=64, seed=1, variable_type=VariableType.Q_VAR)
        with pytest.raises(NotImplementedError):
            route(option_chain(sv), params, nb_path=64, seed=1, comm=Two())
        with pytest.raises(NotImplementedError):
            route(option_chain(sv), params, nb_path=64, seed=1, devices=[0, 0])
    with pytest.raises(NotImplementedError, match="wrt"):
        pricer.model_mc_chain_greeks_conditional(option_chain(sv), params, nb_path=64, seed=1, wrt=["sigma"])
    assert fake.requests == [] and fake.calls == []


# ---- marshalling --------------------------------------------------------------------------------------------------------------------
def test_what_the_fused_routes_hand_the_engine(fake):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    params = sv.HawkesJDParams(mu=0.01, sigma=0.3, lambda_p=5.0, lambda_m=7.0, risk_premia_gamma=0.25)
    kw = params.to_dict()                                        # risk_premia_gamma among them: accepted and unused
    prices, stderrs = sv.hawkesjd_mc_chain_pricer_conditional(nb_path=777, seed=11, **CHAIN, **kw)
    assert fake.requests == [777]
    what, ch, block, spy, recenter, seed, call_id = fake.calls[-1]
    assert what == "price" and (spy, recenter, seed, call_id) == (hp.NB_STEPS_PER_YEAR, True, 11, 0) and spy == 1800
    assert block.tolist() == [float(kw[k]) for k in hp.PARAM_NAMES] and block.size == 16
    t, f, d, k_all, c_all, offs = ch["keep"]
    assert t.tolist() == [0.25, 0.5] and f.tolist() == [1.0, 1.02] and d.tolist() == [1.0, 0.99]
    assert k_all.tolist() == [0.9, 1.0, 1.1, 1.0] and c_all.tolist() == [0, 1, 0, 1] and offs.tolist() == [0, 3, 4] and ch["m"] == 2
    assert [p.shape for p in prices] == [(3,), (1,)] and prices[1].tolist() == [3.0] and stderrs[0].tolist() == [-0.0, -1.0, -2.0]
    # recenter, the step count and the statistics are passed on; an explicit seed is call 0
    out = sv.hawkesjd_mc_chain_pricer_conditional(nb_path=777, seed=12, recenter=False, nb_steps_per_year=360, return_stats=True,
                                                  **CHAIN, **kw)
    assert len(out) == 3 and out[2] == [dict(n_kept=64)] * 2 and fake.calls[-1][3:] == (360, False, 12, 0)
    # without a seed: the process seed and the NEXT call id, once per call
    sv.set_seed(2024)
    sv.hawkesjd_mc_chain_pricer_conditional(nb_path=777, **CHAIN, **kw)
    first = fake.calls[-1]
    g = sv.hawkesjd_mc_chain_greeks_conditional(nb_path=777, return_stats=True, **CHAIN, **kw)
    second = fake.calls[-1]
    assert first[5] == second[5] == 2024 and second[6] == first[6] + 1 and second[0] == "greeks"
    assert sorted(g) == sorted(GREEKS_FIELDS + ("stats",)) and g["gamma"][0].tolist() == [6.0] * 3 and g["dual_gamma"][1].shape == (1,)
    assert sorted(sv.hawkesjd_mc_chain_greeks_conditional(nb_path=777, seed=3, **CHAIN, **kw)) == sorted(GREEKS_FIELDS)
    # the class routes are the function routes on the chain's arrays and the parameter set's fields
    pricer = sv.HawkesJDPricer()
    pricer.model_mc_price_chain_conditional(option_chain(sv), params, nb_path=777, seed=11)
    assert fake.calls[-1][0] == "price" and fake.calls[-1][2].tolist() == block.tolist() and fake.calls[-1][3:] == (1800, True, 11, 0)
    assert fake.calls[-1][1] is ch                               # the same marshalled chain
    pricer.model_mc_chain_greeks_conditional(option_chain(sv), params, nb_path=777, seed=11, recenter=False)
    assert fake.calls[-1][0] == "greeks" and fake.calls[-1][3:] == (1800, False, 11, 0)
    # the density route: one expiry at forward 1 and discount factor 1, calls at exp(x), no recentring, pdf = K dual_gamma
    x = np.linspace(-0.5, 0.5, 5)
    pdf, err = pricer.get_log_return_mc_pdf_conditional(params, 0.25, x, nb_path=777, seed=4, return_stderr=True)
    what, ch, block2, spy, recenter, seed, call_id = fake.calls[-1]
    t, f, d, k_all, c_all, offs = ch["keep"]
    assert what == "greeks" and (spy, recenter, seed, call_id) == (1800, False, 4, 0) and block2.tolist() == block.tolist()
    assert t.tolist() == [0.25] and f.tolist() == [1.0] and d.tolist() == [1.0] and np.array_equal(k_all, np.exp(x))
    assert c_all.tolist() == [0] * 5 and np.array_equal(pdf, np.exp(x) * 8.0) and np.array_equal(err, np.exp(x) * 9.0)
