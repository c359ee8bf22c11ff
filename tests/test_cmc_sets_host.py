"""
Host checks of the conditional Monte Carlo calibration objective (include/svmc.h): the refusals of the Python
routes before any engine call, the dispatch of the calibrations without the new keyword, the two C symbols and the new kernels'
metadata in the build.  No GPU.
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

CHAIN = dict(ttms=np.array([0.25, 0.5]), forwards=np.array([1.0, 1.0]), discfactors=np.array([1.0, 0.99]),
             strikes_ttms=[np.array([0.9, 1.0, 1.1]), np.array([1.0])], optiontypes_ttms=[np.array(["C", "P", "C"]), np.array(["P"])])
SYMBOLS = ("svmc_logsv_chain_price_cmc_sets", "svmc_heston_chain_price_cmc_sets")
COUNTED_WORDS = ("cmc", "greeks", "cond_deriv", "cond_many_kernelE", "rng_kernel")


class Two:
    world, rank = 2, 0


@pytest.fixture
def fake(monkeypatch):
    """the recording fake engine where get_engine() returns the HipEngine; `requests` lists every get_engine call"""
    from stochvolmodels_amd.pricers import heston_pricer, logsv_pricer
    eng = FakeEngine(64)
    eng.requests = []
    for mod in (logsv_pricer, heston_pricer):
        monkeypatch.setattr(mod, "get_engine", lambda n, *a, **k: eng.requests.append(n) or eng)
    return eng


def option_chain(sv):
    vols = [np.full(3, 0.3), np.full(1, 0.3)]
    return sv.OptionChain(ids=np.array(["a", "b"]), bid_ivs=vols, ask_ivs=vols, **CHAIN)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_the_sets_functions_refuse_before_any_engine_call(fake):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import VariableType
    ic = dict(CHAIN, optiontypes_ttms=[np.array(["IC", "C", "C"]), np.array(["P"])])
    for fn, plist in ((sv.logsv_mc_chain_pricer_conditional_sets, [sv.LOGSV_BTC_PARAMS] * 2),
                      (sv.heston_mc_chain_pricer_conditional_sets, [sv.BTC_HESTON_PARAMS] * 2)):
        with pytest.raises(ValueError, match="not implemented"):
            fn(plist, nb_path=64, seed=1, **ic)
        with pytest.raises(NotImplementedError):
            fn(plist, nb_path=64, seed=1, variable_type=VariableType.Q_VAR, **CHAIN)
        with pytest.raises(NotImplementedError):
            fn(plist, nb_path=64, seed=1, comm=Two(), **CHAIN)
        with pytest.raises(NotImplementedError):
            fn(plist, nb_path=64, seed=1, devices=2, **CHAIN)
        assert fn([], nb_path=64, seed=1, **CHAIN) == []
    with pytest.raises(NotImplementedError):
        sv.logsv_mc_chain_pricer_conditional_sets([sv.LOGSV_BTC_PARAMS], nb_path=64, seed=1, is_spot_measure=False, **CHAIN)
    with pytest.raises(NotImplementedError):
        sv.heston_mc_chain_pricer_conditional_sets([sv.BTC_HESTON_PARAMS], nb_path=64, seed=1, scheme="qe", **CHAIN)
    assert fake.requests == [] and fake.calls == []


def test_the_conditional_calibrations_refuse_before_any_engine_call(fake):
    import stochvolmodels_amd as sv
    chain = option_chain(sv)
    mc = dict(calibration_engine=sv.CalibrationEngine.MC, estimator="conditional", nb_path=64, disp=False)
    logsv, heston = sv.LogSVPricer(), sv.HestonPricer()
    with pytest.raises(ValueError, match="hbm"):
        logsv.calibrate_model_params_to_chain(chain, sv.LOGSV_BTC_PARAMS, device_randoms="hbm", **mc)
    with pytest.raises(ValueError, match="estimator"):
        logsv.calibrate_model_params_to_chain(chain, sv.LOGSV_BTC_PARAMS, **dict(mc, estimator="plain"))
    for extra in (dict(comm=Two()), dict(devices=2)):
        with pytest.raises(NotImplementedError):
            logsv.calibrate_model_params_to_chain(chain, sv.LOGSV_BTC_PARAMS, **mc, **extra)
        with pytest.raises(NotImplementedError):
            heston.calibrate_model_params_to_chain(chain, estimator="conditional", nb_path=64, disp=False, **extra)
    with pytest.raises(NotImplementedError):
        heston.calibrate_model_params_to_chain(chain, estimator="conditional", nb_path=64, disp=False, scheme="qe")
    with pytest.raises(ValueError, match="estimator"):
        heston.calibrate_model_params_to_chain(chain, estimator="plain", disp=False)
    inverse = sv.OptionChain(ids=np.array(["a", "b"]), bid_ivs=chain.bid_ivs, ask_ivs=chain.ask_ivs,
                             **dict(CHAIN, optiontypes_ttms=[np.array(["IC", "C", "C"]), np.array(["P"])]))
    with pytest.raises(ValueError, match="not implemented"):
        logsv.calibrate_model_params_to_chain(inverse, sv.LOGSV_BTC_PARAMS, **mc)
    assert fake.requests == [] and fake.calls == []


# ---- dispatch -----------------------------------------------------------------------------------------------------------------------
def test_without_the_keyword_the_calibrations_call_what_they_called(fake, monkeypatch):
    """estimator absent: the LogSV MC engine prices on the frozen / uploaded randoms, Heston on the analytic pricer -- never on the
    new call"""
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.pricers import heston_pricer, logsv_pricer
    chain = option_chain(sv)
    seen = []

    class Stop(Exception):
        pass

    def stop(name):
        def raiser(*a, **k):
            seen.append(name)
            raise Stop(name)
        return raiser

    for mod, name in ((logsv_pricer, "logsv_mc_chain_pricer_conditional_sets"), (heston_pricer, "heston_mc_chain_pricer_conditional_sets")):
        monkeypatch.setattr(mod, name, stop("sets"))
    monkeypatch.setattr(logsv_pricer, "draw_fixed_randoms_on_device", stop("frozen"))
    monkeypatch.setattr(logsv_pricer, "get_randoms_for_chain_valuation", stop("host randoms"))
    monkeypatch.setattr(heston_pricer.HestonPricer, "compute_model_ivols_for_chain", stop("analytic"))
    monkeypatch.setattr(logsv_pricer.LogSVPricer, "compute_model_ivols_for_chain", stop("analytic"))
    MC, AN = sv.CalibrationEngine.MC, sv.CalibrationEngine.ANALYTIC
    for kw, want in ((dict(calibration_engine=MC, device_randoms=True), "frozen"), (dict(calibration_engine=MC), "host randoms"),
                     (dict(calibration_engine=AN), "analytic")):
        with pytest.raises(Stop, match=want):
            sv.LogSVPricer().calibrate_model_params_to_chain(chain, sv.LOGSV_BTC_PARAMS, nb_path=64, disp=False, **kw)
    with pytest.raises(Stop, match="analytic"):
        sv.HestonPricer().calibrate_model_params_to_chain(chain, disp=False)
    assert "sets" not in seen
    # ... and with it, the new call
    with pytest.raises(Stop, match="sets"):
        sv.LogSVPricer().calibrate_model_params_to_chain(chain, sv.LOGSV_BTC_PARAMS, calibration_engine=MC, estimator="conditional",
                                                         nb_path=64, disp=False)
    with pytest.raises(Stop, match="sets"):
        sv.HestonPricer().calibrate_model_params_to_chain(chain, estimator="conditional", nb_path=64, disp=False)


def test_lists_longer_than_eight_go_in_calls_of_eight_on_one_stream(monkeypatch):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.pricers import heston_pricer, logsv_pricer

    class Recorder:
        def __init__(self):
            self.calls = []

        def price_chain_cmc_sets_fused(self, ch, model, params, mode, spy, recenter, seed, call_id, want_ivols=True):
            self.calls.append((model, np.array(params), seed, call_id, want_ivols))
            row = lambda v: [np.full(sl.stop - sl.start, float(v)) for sl in ch["slices"]]      # noqa: E731
            return [(row(p[0]), row(-p[0]), row(2 * p[0]) if want_ivols else None, [{} for _ in range(ch["m"])]) for p in params]

    eng = Recorder()
    for mod in (logsv_pricer, heston_pricer):
        monkeypatch.setattr(mod, "get_engine", lambda n: eng)
    plist = [sv.HestonParams(v0=0.01 * (q + 1), theta=0.04, kappa=2.0, rho=-0.3, volvol=0.3) for q in range(11)]
    out = sv.heston_mc_chain_pricer_conditional_sets(plist, nb_path=64, return_ivols=True, return_stats=True, **CHAIN)
    assert [c[1].shape for c in eng.calls] == [(8, 5), (3, 5)] and len(out) == 11
    assert len({(c[2], c[3]) for c in eng.calls}) == 1                       # ONE (seed, call id) for every set
    assert all(len(o) == 4 and o[2][0].shape == (3,) and o[2][1].shape == (1,) for o in out)
    assert [o[0][0][0] for o in out] == [pytest.approx(0.01 * (q + 1)) for q in range(11)]
    first = eng.calls[0][3]
    sv.logsv_mc_chain_pricer_conditional_sets([sv.LOGSV_BTC_PARAMS] * 2, nb_path=64, **CHAIN)
    model, rows, seed, call_id, want = eng.calls[-1]
    assert (model, rows.shape, want) == ("logsv", (2, 8), False) and call_id == first + 1          # the NEXT call id, once
    assert sv.logsv_mc_chain_pricer_conditional_sets([sv.LOGSV_BTC_PARAMS], nb_path=64, seed=5, **CHAIN)[0][0][0].shape == (3,)
    assert eng.calls[-1][2:4] == (5, 0)


# ---- symbols ------------------------------------------------------------------------------------------------------------------------
def test_the_two_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "svmc.h")).read()
    binding = open(os.path.join(ROOT, "stochvolmodels_amd", "_lib.py")).read()
    for name in SYMBOLS:
        assert re.search(r"SVMC_API int " + name + r"\(", header), name
        assert f'"{name}"' in binding, name
    assert re.search(r"#define SVMC_CMC_SETS_MAX 8\b", header)
    from stochvolmodels_amd.engine import CMC_SETS_MAX
    assert CMC_SETS_MAX == 8


# ---- the build's metadata -----------------------------------------------------------------------------------------------------------
def test_cond_vols_kernels_metadata_and_the_counts_the_existing_tests_assert():
    from stochvolmodels_amd import _lib, build
    build.build()
    L = _lib.load()
    assert all(hasattr(L, name) for name in SYMBOLS)
    meta = json.load(open(build.ISA_JSON))["metadata"]
    new = [k for k in meta if "cond_vols_" in k]
    assert len(new) >= 1, sorted(meta)
    for k in new:
        assert meta[k]["scratch_bytes"] == 0, (k, meta[k])
        assert not any(word in k for word in COUNTED_WORDS), k
        assert not re.search(r"cond_sens_\w*_kernelE", k), k
    assert len([k for k in meta if "cmc" in k]) == 8
    assert len([k for k in meta if "greeks" in k]) == 2
    assert len([k for k in meta if "cond_deriv" in k]) == 2
