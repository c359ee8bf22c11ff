"""
The host skeleton of the four *_mc_chain_pricer*_many functions (mc_chain.many_job_streams / many_job_chunks / many_jobs_shaped and
each function's own loop of single calls), through each of them and without a device: the loop of single calls (one call per job, its own seed, in list order) and the one-launch route's chunks (a list of
MANY_MAX_JOBS + 1 jobs reaches the engine as 64 jobs and 1, each job with its stream: (seed_j, 0), or consecutive call ids).
"""
import numpy as np
import pytest

import stochvolmodels_amd as sv
from stochvolmodels_amd import _lib
from stochvolmodels_amd.engine import MANY_MAX_JOBS
from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
from stochvolmodels_amd.pricers import heston_pricer, logsv_pricer
from stochvolmodels_amd.utils.funcs import get_rng_state, set_rng_state

CHAIN = dict(ttms=np.array([0.1, 0.2]), forwards=np.array([1.0, 1.01]), discfactors=np.array([0.99, 0.98]),
             strikes_ttms=[np.array([0.9, 1.0, 1.1]), np.array([[1.0, 1.2]])],
             optiontypes_ttms=[np.array(["P", "P", "C"]), np.array([["P", "C"]])])
LONG = dict(ttms=0.05 * np.arange(1, 18), forwards=np.ones(17), discfactors=np.ones(17), strikes_ttms=[np.array([1.0])] * 17,
            optiontypes_ttms=[np.array(["C"])] * 17)                     # 17 expiries: one more than a stepping launch takes
WORLD2 = type("World2", (), dict(world=2, rank=0))()
# (the many function, its module, the single pricer's name, a parameter set, its extra keywords, what makes it a loop of singles)
MODELS = {
    "logsv": (sv.logsv_mc_chain_pricer_many, logsv_pricer, "logsv_mc_chain_pricer", sv.LOGSV_BTC_PARAMS, {}, dict(CHAIN, comm=WORLD2)),
    "heston": (sv.heston_mc_chain_pricer_many, heston_pricer, "heston_mc_chain_pricer", sv.HestonParams(), {},
               dict(CHAIN, devices=[0, 1])),
    "hawkesjd": (sv.hawkesjd_mc_chain_pricer_many, hp, "hawkesjd_mc_chain_pricer", hp.HawkesJDParams(), {}, LONG),
    "tilted": (sv.hawkesjd_mc_chain_pricer_with_risk_premia_gammas_many, hp, "hawkesjd_mc_chain_pricer_with_risk_premia_gammas",
               hp.HawkesJDParams(), dict(risk_premia_gammas=[0.0, 1.0]), LONG),
}


class StubEngine:
    """records the many-job engine calls and answers each job with arrays that say which job it was"""

    def __init__(self):
        self.calls = []

    def price_chain_many_fused(self, ch, model, params, seeds, call_ids, mode, nb_steps_per_year, variable_type):
        self.calls.append((len(params), list(seeds), list(call_ids)))
        return [([np.full(3, float(s)), np.full(2, float(s))], [np.full(3, float(c)), np.full(2, float(c))])
                for s, c in zip(seeds, call_ids)]

    def price_hawkesjd_chain_tilted_many_fused(self, ch, params, nb_steps_per_year, seeds, call_ids, gammas, recenter):
        assert len(gammas) == len(params)
        self.calls.append((len(params), list(seeds), list(call_ids)))
        return [(("prices", s, c), ("stderrs", s, c), None) for s, c in zip(seeds, call_ids)]


@pytest.fixture
def stub(monkeypatch):
    """the library may not be loaded; the pricer modules' get_engine hands out the stub"""
    def boom(*a, **k):
        raise AssertionError("the library was asked for")
    eng = StubEngine()
    monkeypatch.setattr(_lib, "load", boom)
    for module in (logsv_pricer, heston_pricer, hp):
        monkeypatch.setattr(module, "get_engine", lambda *a, **k: eng)
    return eng


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("seeded", [True, False])
def test_loop_of_single_calls_one_per_job_with_its_seed_in_order(monkeypatch, stub, model, seeded):
    many, module, single_name, p, extra, chain = MODELS[model]
    seen = []

    def single(**kw):
        seen.append(kw["seed"])
        return ("single", len(seen))
    monkeypatch.setattr(module, single_name, single)
    seeds = [11, 7, 9] if seeded else None
    before = get_rng_state()
    out = many([p, p, p], seeds=seeds, **chain, **extra)
    assert seen == (seeds if seeded else [None] * 3)               # unseeded: every single call takes its own call id itself
    assert out == [("single", 1), ("single", 2), ("single", 3)]
    assert stub.calls == [] and get_rng_state() == before          # the driver itself took no call id and asked for no engine


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("seeded", [True, False])
def test_a_long_list_reaches_the_engine_in_chunks_with_each_jobs_stream(stub, model, seeded):
    many, _, _, p, extra, _ = MODELS[model]
    n = MANY_MAX_JOBS + 1
    seeds = [1000 + 3 * j for j in range(n)] if seeded else None
    seed0, calls0 = get_rng_state()
    try:
        set_rng_state(seed0, 5)
        out = many([p] * n, seeds=seeds, **CHAIN, **extra)
        assert get_rng_state() == ((seed0, 5) if seeded else (seed0, 5 + n))
    finally:
        set_rng_state(seed0, calls0)
    streams = [(s, 0) for s in seeds] if seeded else [(seed0, 5 + j) for j in range(n)]
    assert [c[0] for c in stub.calls] == [MANY_MAX_JOBS, 1]
    assert [(s, c) for _, ss, cc in stub.calls for s, c in zip(ss, cc)] == streams
    assert len(out) == n
    for (s, c), res in zip(streams, out):                           # job j's result is job j's, in the strikes' shapes
        if model == "tilted":
            assert res == (("prices", s, c), ("stderrs", s, c))
        else:
            prices, stderrs = res
            assert [a.shape for a in prices] == [a.shape for a in stderrs] == [(3,), (1, 2)]
            assert all((a == s).all() for a in prices) and all((a == c).all() for a in stderrs)
