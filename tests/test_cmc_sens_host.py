"""
Host checks of the conditional estimator's parameter sensitivities (include/svmc.h): the estimator and its
error on a toy model through the long-double twin (tests/cmc_sens_twin.py), the keyword handling and the refusals of the Python
routes (no device work), and the new kernels' ISA metadata.  No GPU.
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cmc_sens_twin as st  # noqa: E402

# ---- 1: the error of the difference on the toy model --------------------------------------------------------------------------------
SEEDS = range(1, 65)
RHOS = (-0.3, -0.9)
TOY_K = np.array([0.7, 1.0, 1.3, 0.7, 1.0, 1.3])
TOY_T = np.array(["C", "C", "C", "P", "P", "P"])
BAND = (0.73, 1.27)        # spread of 64 samples over their true deviation: sqrt(chi2_63 / 63) stays inside at about 3 deviations


@pytest.fixture(scope="module")
def toy_ratios():
    """{(rho, recenter, mutate): spread of sens over the seeds / mean reported error, per quote}"""
    runs = {}
    for rho in RHOS:
        jobs = [st.toy_jobs(seed, rho) for seed in SEEDS]
        for recenter, mutate in ((True, None), (False, None), (True, "d_only")):
            res = [st.estimator(*job, st.TOY_BUMP, 1.0, TOY_K, TOY_T, 1.0, recenter, mutate) for job in jobs]
            sens, errs = np.array([r[0] for r in res]), np.array([r[1] for r in res])
            assert all(np.all(r[2] == st.TOY_PATHS) for r in res)
            runs[(rho, recenter, mutate)] = sens.std(axis=0, ddof=1) / errs.mean(axis=0)
    return runs


def test_reported_error_matches_the_spread_over_seeds_on_all_24_cases(toy_ratios):
    for rho in RHOS:
        for recenter in (True, False):
            r = toy_ratios[(rho, recenter, None)]
            print(f"cmc sens toy rho={rho} recenter={recenter} spread / error", np.round(r, 3))
            assert np.all((r >= BAND[0]) & (r <= BAND[1])), (rho, recenter, r)


def test_the_deviation_of_d_alone_misses_the_band_on_the_recentred_atm_put(toy_ratios):
    """without the delta-method term of the two recentring means the test above fails: it sees a missing term"""
    r = toy_ratios[(-0.3, True, "d_only")]
    print("cmc sens toy rho=-0.3 recentred, deviation of d alone: spread / error", np.round(r, 3))
    put_atm = 4                                                # K = 1.0, 'P'
    assert not (BAND[0] <= r[put_atm] <= BAND[1]), r


def test_twin_degenerate_cases():
    mu_up, cv_up, mu_dn, cv_dn = (a[:64].copy() for a in st.toy_jobs(3, -0.5))
    mu_up[5] = np.nan                                          # dropped in the up job only: the pair goes, the dn job keeps it
    cv_dn[9] = -1e-3
    s, e, n = st.estimator(mu_up, cv_up, mu_dn, cv_dn, 1e-3, 1.0, [1.0], ["P"])
    assert n[0] == 62 and np.isfinite(s[0]) and e[0] > 0.0
    same = st.estimator(np.full(8, -0.02), np.full(8, 0.04), np.full(8, -0.021), np.full(8, 0.041), 1e-3, 1.0, [0.9, 1.1], ["C", "P"])
    assert np.all(same[1] == 0.0) and np.all(np.isfinite(same[0]))          # identical paths: an error of exactly 0
    none = st.estimator(np.full(4, np.nan), np.ones(4), np.zeros(4), np.ones(4), 1e-3, 1.0, [1.0], ["C"])
    assert np.isnan(none[0][0]) and np.isnan(none[1][0]) and none[2][0] == 0


# ---- 2: keyword handling and refusals, before any device work -----------------------------------------------------------------------
CHAIN = dict(ttms=np.array([0.25, 0.5]), forwards=np.array([1.0, 1.0]), discfactors=np.array([1.0, 0.99]),
             strikes_ttms=[np.array([0.9, 1.0, 1.1]), np.array([1.0])], optiontypes_ttms=[np.array(["C", "P", "C"]), np.array(["P"])],
             nb_path=64, seed=1)
LKW = dict(v0=0.2, theta=0.25, kappa1=1.0, kappa2=1.5, beta=-0.3, volvol=0.4, vol_backbone_etas=np.array([1.0, 1.1]))
HKW = dict(v0=0.04, theta=0.05, kappa=4.0, rho=-0.5, volvol=0.4)


class RecordingEngine:
    """stands where get_engine() returns the HipEngine: records the fused calls and returns recognisable numbers"""

    def __init__(self):
        self.calls = []

    def _fields(self, ch):
        from stochvolmodels_amd.engine import CMC_GREEKS_FIELDS
        return {f: [np.full(sl.stop - sl.start, float(r)) for sl in ch["slices"]] for r, f in enumerate(CMC_GREEKS_FIELDS)}

    def price_logsv_chain_cmc_greeks_fused(self, ch, *args):
        self.calls.append(("f13", args))
        return self._fields(ch), [{} for _ in range(ch["m"])]

    price_heston_chain_cmc_greeks_fused = price_logsv_chain_cmc_greeks_fused

    def price_chain_cmc_sens_fused(self, ch, model, rows, steps, mode, nb_steps_per_year, recenter, seed, call_id):
        self.calls.append(("f14", model, np.array(rows), np.array(steps), recenter))
        sens = np.arange(len(steps) * 3 * ch["total"], dtype=np.float64).reshape(len(steps), 3, ch["total"])
        return self._fields(ch), [{} for _ in range(ch["m"])], sens


@pytest.fixture
def recorder(monkeypatch):
    from stochvolmodels_amd.pricers import heston_pricer, logsv_pricer
    eng = RecordingEngine()
    monkeypatch.setattr(logsv_pricer, "get_engine", lambda n: eng)
    monkeypatch.setattr(heston_pricer, "get_engine", lambda n: eng)
    return eng


def test_empty_wrt_is_the_f13_call_with_its_keys(recorder):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.engine import CMC_GREEKS_FIELDS
    for fn, kw in ((sv.logsv_mc_chain_greeks_conditional, LKW), (sv.heston_mc_chain_greeks_conditional, HKW)):
        for extra in ({}, {"wrt": ()}, {"wrt": []}):
            out = fn(**CHAIN, **kw, **extra)
            assert tuple(out) == CMC_GREEKS_FIELDS
        assert set(fn(return_stats=True, **CHAIN, **kw)) == set(CMC_GREEKS_FIELDS) | {"stats"}
    assert recorder.calls and all(c[0] == "f13" for c in recorder.calls)


def test_wrt_builds_the_job_table_and_shapes_the_sensitivities(recorder):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.engine import CMC_GREEKS_FIELDS
    out = sv.logsv_mc_chain_greeks_conditional(wrt=("sigma0", "volvol"), bumps={"volvol": 0.01}, **CHAIN, **LKW)
    kind, model, rows, h, recenter = recorder.calls[-1]
    assert (kind, model, recenter) == ("f14", "logsv", True)
    assert np.array_equal(h, [1e-3 * 0.2, 0.01]) and rows.shape == (5, 8)
    base = np.array([0.2, 0.25, 1.0, 1.5, -0.3, 0.4, 1.0, 1.1])
    assert np.array_equal(rows[0], base)
    assert rows[1, 0] == 0.2 + h[0] and rows[2, 0] == 0.2 - h[0] and rows[3, 5] == 0.4 + 0.01 and rows[4, 5] == 0.4 - 0.01
    assert np.array_equal(np.delete(rows[1], 0), np.delete(base, 0)) and np.array_equal(np.delete(rows[4], 5), np.delete(base, 5))
    assert tuple(out) == CMC_GREEKS_FIELDS + ("sens", "sens_stderr", "n_pairs")
    for key in ("sens", "sens_stderr", "n_pairs"):
        assert tuple(out[key]) == ("sigma0", "volvol")
        assert [a.shape for a in out[key]["volvol"]] == [(3,), (1,)]
    assert out["n_pairs"]["sigma0"][0].dtype == np.int64
    assert np.array_equal(out["sens"]["volvol"][1], [12.0 + 3.0]) and np.array_equal(out["sens_stderr"]["sigma0"][0], [4.0, 5.0, 6.0])
    for wrt in (None, "all"):
        out = sv.heston_mc_chain_greeks_conditional(wrt=wrt, recenter=False, **CHAIN, **HKW)
        kind, model, rows, h, recenter = recorder.calls[-1]
        assert (model, recenter, rows.shape) == ("heston", False, (11, 5)) and tuple(out["sens"]) == ("v0", "theta", "kappa", "rho", "volvol")
    option_chain = sv.OptionChain(ttms=CHAIN["ttms"], forwards=CHAIN["forwards"], discfactors=CHAIN["discfactors"],
                                  strikes_ttms=CHAIN["strikes_ttms"], optiontypes_ttms=CHAIN["optiontypes_ttms"], ids=np.array(["a", "b"]))
    out = sv.HestonPricer().model_mc_chain_greeks_conditional(option_chain, sv.BTC_HESTON_PARAMS, nb_path=64, seed=1, wrt=("volvol",))
    assert tuple(out["sens"]) == ("volvol",) and recorder.calls[-1][1] == "heston"
    out = sv.LogSVPricer().model_mc_chain_greeks_conditional(option_chain, sv.LOGSV_BTC_PARAMS, nb_path=64, seed=1, wrt=("beta",),
                                                             rel_bump=1e-2)
    assert tuple(out["sens"]) == ("beta",) and recorder.calls[-1][3][0] == 1e-2 * abs(sv.LOGSV_BTC_PARAMS.beta)


def test_refusals_and_bump_errors_come_before_any_device_work(recorder):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import VariableType

    class Two:
        world, rank = 2, 0

    for fn, kw, name in ((sv.logsv_mc_chain_greeks_conditional, LKW, "sigma0"), (sv.heston_mc_chain_greeks_conditional, HKW, "v0")):
        wrt = dict(wrt=(name,))
        with pytest.raises(ValueError, match="not implemented"):
            fn(**dict(CHAIN, optiontypes_ttms=[np.array(["IC", "C", "C"]), np.array(["P"])]), **kw, **wrt)
        with pytest.raises(NotImplementedError):
            fn(variable_type=VariableType.Q_VAR, **CHAIN, **kw, **wrt)
        with pytest.raises(NotImplementedError):
            fn(devices=2, **CHAIN, **kw, **wrt)
        with pytest.raises(NotImplementedError):
            fn(comm=Two(), **CHAIN, **kw, **wrt)
        with pytest.raises(ValueError, match="nonsense"):
            fn(wrt=("nonsense",), **CHAIN, **kw)
        with pytest.raises(ValueError, match="twice"):
            fn(wrt=(name, name), **CHAIN, **kw)
        with pytest.raises(ValueError, match=name):
            fn(wrt=(name,), bumps={name: -1.0}, **CHAIN, **kw)
        with pytest.raises(ValueError, match=f"{name}.*leaves its domain"):
            fn(wrt=(name,), bumps={name: 10.0}, **CHAIN, **kw)
        with pytest.raises(ValueError, match="volvol is zero"):
            fn(wrt=("volvol",), **CHAIN, **dict(kw, volvol=0.0))
        long = dict(CHAIN, ttms=np.linspace(0.1, 1.7, 17), forwards=np.ones(17), discfactors=np.ones(17),
                    strikes_ttms=[np.array([1.0])] * 17, optiontypes_ttms=[np.array(["C"])] * 17)
        lkw = dict(kw, vol_backbone_etas=np.ones(17)) if "vol_backbone_etas" in kw else kw
        with pytest.raises(NotImplementedError, match="16 expiries"):
            fn(**long, **lkw, **wrt)
    with pytest.raises(ValueError, match="rho.*leaves its domain"):
        sv.heston_mc_chain_greeks_conditional(wrt=("rho",), bumps={"rho": 0.6}, **CHAIN, **HKW)
    with pytest.raises(NotImplementedError):
        sv.logsv_mc_chain_greeks_conditional(is_spot_measure=False, wrt=("beta",), **CHAIN, **LKW)
    with pytest.raises(NotImplementedError):
        sv.heston_mc_chain_greeks_conditional(scheme="qe", wrt=("rho",), **CHAIN, **HKW)
    # the many-job pricers
    many = {k: v for k, v in CHAIN.items() if k != "seed"}
    for fn, plist in ((sv.logsv_mc_chain_pricer_conditional_many, [sv.LOGSV_BTC_PARAMS] * 2),
                      (sv.heston_mc_chain_pricer_conditional_many, [sv.BTC_HESTON_PARAMS] * 2)):
        with pytest.raises(ValueError, match="not implemented"):
            fn(plist, **dict(many, optiontypes_ttms=[np.array(["IP", "C", "C"]), np.array(["P"])]))
        with pytest.raises(NotImplementedError):
            fn(plist, variable_type=VariableType.Q_VAR, **many)
        with pytest.raises(NotImplementedError):
            fn(plist, devices=2, **many)
        with pytest.raises(NotImplementedError):
            fn(plist, comm=Two(), **many)
        with pytest.raises(ValueError, match="seeds has 3"):
            fn(plist, seeds=[1, 2, 3], **many)
        assert fn([], **many) == []
    with pytest.raises(NotImplementedError):
        sv.logsv_mc_chain_pricer_conditional_many([sv.LOGSV_BTC_PARAMS], is_spot_measure=False, **many)
    with pytest.raises(NotImplementedError):
        sv.heston_mc_chain_pricer_conditional_many([sv.BTC_HESTON_PARAMS], scheme="qe", **many)
    with pytest.raises(ValueError, match="not implemented"):
        sv.compute_mc_vars_sens_conditional(np.zeros(4), np.ones(4), np.zeros(4), np.ones(4), 1e-3, 1.0, np.array([1.0]), np.array(["IC"]))
    with pytest.raises(ValueError, match="step"):
        sv.compute_mc_vars_sens_conditional(np.zeros(4), np.ones(4), np.zeros(4), np.ones(4), 0.0, 1.0, np.array([1.0]), np.array(["C"]))
    assert recorder.calls == []


# ---- 3: the build's ISA metadata ----------------------------------------------------------------------------------------------------
NEW_KERNELS = ("logsv_chain_cond_many_kernelE", "logsv_chain_cond_many_lat_kernelE", "heston_chain_cond_many_kernelE",
               "heston_chain_cond_many_lat_kernelE", "cond_sens_jobs_kernelE", "cond_sens_pairs_kernelE", "cond_sens_finish_kernelE")


def test_new_kernels_metadata_and_the_counts_the_existing_tests_assert():
    from stochvolmodels_amd import build
    build.build()
    meta = json.load(open(build.ISA_JSON))["metadata"]
    for stem in NEW_KERNELS:
        hit = [k for k in meta if stem in k]
        assert len(hit) == 1, (stem, hit)
        assert meta[hit[0]]["scratch_bytes"] == 0, (stem, meta[hit[0]])
        assert not any(word in hit[0] for word in ("cmc", "greeks", "cond_deriv")), hit[0]
    # gfx950: 512 vector registers per lane of a SIMD in granules of 8, 160 KB of LDS per CU, 4 SIMDs (tests/test_cmc_host.py)
    for stem, block in (("logsv_chain_cond_many_kernelE", 1024), ("heston_chain_cond_many_kernelE", 512)):
        m = [v for k, v in meta.items() if stem in k][0]
        by_regs = 512 // (-(-m["vgpr"] // 8) * 8)
        by_lds = (160 * 1024 // m["lds_bytes"]) * (block // 64) // 4
        assert min(by_regs, by_lds, 8) == 8, (stem, m, by_regs, by_lds)
    assert len([k for k in meta if "cmc" in k]) == 8
    assert len([k for k in meta if "greeks" in k]) == 2
    assert len([k for k in meta if "cond_deriv" in k]) == 2
