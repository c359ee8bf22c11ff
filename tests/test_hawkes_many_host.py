"""
Host side of the many-job Hawkes Monte Carlo calls, no GPU: the two new C entry points in the library, the
header and the ctypes table; the Python functions and methods and their package exports; the argument checks that are made
before any device work; the new stepping kernel's scratch and LDS in the build's metadata.
"""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import stochvolmodels_amd as sv
from stochvolmodels_amd import _lib, engine
from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("svmc_hawkesjd_chain_price_many", "svmc_hawkesjd_chain_price_tilted_many")
CHAIN = dict(ttms=np.array([0.1, 0.2]), forwards=np.array([1.0, 1.01]), discfactors=np.array([0.99, 0.98]),
             strikes_ttms=[np.array([0.9, 1.0, 1.1]), np.array([1.0, 1.2])],
             optiontypes_ttms=[np.array(["P", "P", "C"]), np.array(["P", "C"])])


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to load the library, or to make an engine, fails the test"""
    def boom(*a, **k):
        raise AssertionError("the device was asked for before the request was answered")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(hp, "get_engine", boom)


def test_symbols_in_library_header_and_ctypes():
    from stochvolmodels_amd import build
    lib = C.CDLL(build.build())
    text = open(os.path.join(ROOT, "include", "svmc.h")).read()
    src = open(os.path.join(ROOT, "stochvolmodels_amd", "_lib.py")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name)
        assert re.search(r"SVMC_API int " + name + r"\(", text) and f'"{name}"' in src
    L = _lib.load()
    plain, tilted = (getattr(L, name) for name in SYMBOLS)
    # one argument fewer than the LogSV call (no is_spot_measure); the single tilted call's plus n_jobs, seeds and ids for seed, id
    assert len(plain.argtypes) == len(L.svmc_logsv_chain_price_many.argtypes) - 1 == 16
    assert len(tilted.argtypes) == len(L.svmc_hawkesjd_chain_price_tilted.argtypes) + 1 == 18
    assert int(re.search(r"#define SVMC_MANY_MAX_JOBS (\d+)", text).group(1)) == engine.MANY_MAX_JOBS


def test_python_names_and_exports():
    for name in ("hawkesjd_mc_chain_pricer_many", "hawkesjd_mc_chain_pricer_with_risk_premia_gammas_many"):
        assert name in sv.__all__ and callable(getattr(sv, name)) and getattr(sv, name) is getattr(hp, name)
    sig = inspect.signature(hp.hawkesjd_mc_chain_pricer_many).parameters
    assert list(sig) == ["params_list", "ttms", "forwards", "discfactors", "strikes_ttms", "optiontypes_ttms", "nb_path",
                         "variable_type", "nb_steps_per_year", "seeds", "comm", "devices"]
    assert sig["nb_path"].default == 100000 and sig["nb_steps_per_year"].default == hp.NB_STEPS_PER_YEAR and sig["seeds"].default is None
    sig = inspect.signature(hp.hawkesjd_mc_chain_pricer_with_risk_premia_gammas_many).parameters
    for name, default in (("recenter_forward", False), ("return_forwards", False), ("seeds", None)):
        assert sig[name].default is default
    assert "risk_premia_gammas" in sig
    assert callable(sv.HawkesJDPricer.model_mc_price_chain_many) and callable(sv.HawkesJDPricer.model_mc_price_chain_with_risk_premia_many)
    assert callable(engine.HipEngine.price_hawkesjd_chain_tilted_many_fused)
    assert '"hawkesjd"' in inspect.getsource(engine.HipEngine.price_chain_many_fused)


def test_argument_checks_need_no_device(no_device):
    p = hp.HawkesJDParams()
    many, tilted = sv.hawkesjd_mc_chain_pricer_many, sv.hawkesjd_mc_chain_pricer_with_risk_premia_gammas_many
    assert many([], **CHAIN) == [] and tilted([], risk_premia_gammas=[1.0], **CHAIN) == []
    for fn, kw in ((many, {}), (tilted, dict(risk_premia_gammas=[1.0]))):
        with pytest.raises(ValueError, match="seeds has 3 entries for 2 parameter sets"):
            fn([p, p], seeds=[1, 2, 3], **CHAIN, **kw)
        for vt in (sv.VariableType.Q_VAR, sv.VariableType.SIGMA):
            with pytest.raises(NotImplementedError):
                fn([p], variable_type=vt, **CHAIN, **kw)
        with pytest.raises(NotImplementedError):                    # sharded: what the single pricers raise
            fn([p], devices=[0, 1], **CHAIN, **kw)
        with pytest.raises(NotImplementedError):
            fn([p], comm=type("World2", (), dict(world=2, rank=0))(), **CHAIN, **kw)
    for ragged in ([[1.0], [1.0, 2.0]], [[1.0, 2.0], [1.0]], [[1.0], [2.0], [3.0]], [1.0, [2.0]], [[1.0], []]):
        with pytest.raises(ValueError):
            tilted([p, p], risk_premia_gammas=ragged, **CHAIN)
    for bad in ([], [[], []], [np.nan], [[1.0], [np.inf]], list(np.zeros(engine.TILTED_MAX_GAMMAS + 1))):
        with pytest.raises(ValueError):
            tilted([p, p], risk_premia_gammas=bad, **CHAIN)
    with pytest.raises(ValueError, match="^not implemented$"):      # 'C' / 'P' only
        tilted([p], risk_premia_gammas=[1.0], **dict(CHAIN, optiontypes_ttms=[np.array(["P", "IC", "C"]), np.array(["P", "C"])]))
    chain = sv.OptionChain(ttms=CHAIN["ttms"], forwards=CHAIN["forwards"], discfactors=CHAIN["discfactors"],
                           strikes_ttms=tuple(CHAIN["strikes_ttms"]), optiontypes_ttms=tuple(CHAIN["optiontypes_ttms"]), ids=None)
    import dataclasses
    with pytest.raises(ValueError, match="risk_premia_gamma must be set for the risk-premia pricer"):
        sv.HawkesJDPricer().model_mc_price_chain_with_risk_premia_many(chain, [dataclasses.replace(p, risk_premia_gamma=1.0), p],
                                                                       nb_path=64)


def test_gammas_shared_or_per_job():
    assert np.array_equal(hp.many_job_gammas([-1, 0, 1], 2), [[-1.0, 0.0, 1.0]] * 2)
    assert np.array_equal(hp.many_job_gammas(np.array([0.5]), 3), [[0.5]] * 3)
    assert np.array_equal(hp.many_job_gammas([[1, 2], (3, 4), np.array([5, 6])], 3), [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    g = hp.many_job_gammas([[1.0]], 1)
    assert g.dtype == np.float64 and g.flags.c_contiguous and g.shape == (1, 1)


def test_the_many_kernel_uses_no_scratch_and_only_the_draw_tables_lds():
    path = os.path.join(ROOT, "stochvolmodels_amd", "libsvmc.isa.json")
    if not os.path.exists(path):
        from stochvolmodels_amd import build
        build.build()
    meta = json.load(open(path))["metadata"]
    many = [v for k, v in meta.items() if "hawkesjd_chain_rng_many_kernel" in k]
    assert len(many) == 1
    assert many[0]["scratch_bytes"] == 0 and many[0]["lds_bytes"] == 32768
    assert all(v["scratch_bytes"] == 0 for v in meta.values())              # no kernel of the library spills
