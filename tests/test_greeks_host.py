"""
The Monte Carlo chain Greeks (include/svmc.h), checked without a device on the CPU twin tests/greeks_twin.py:

  1. closed form: on Gaussian log-returns (2^18 draws of NumPy's default_rng(20261019)) the twin's price, delta and dual delta sit
     within 4 of their own standard errors of Black-76, and so does the sigma sensitivity, whose up / dn rows are the same normals at
     sigma +- h;
  2. homogeneity: price = F delta + K dual_delta holds in the twin to long-double rounding;
  3. the job table: 1 + 2P rows, the base row untouched, up then dn per parameter; one seed and one call id for all rows;
  4. the refusals, each raised before an engine is touched: 'IC' / 'IP', other variables, devices=, a sharded communicator, the
     inverse measure, a zero parameter without a bump, a bump out of the parameter's domain;
  5. the build's metadata: the two new kernels use no scratch.

The sensitivity's error is the deviation of dt = d - s (q_up (spot_up - F) - q_dn (spot_dn - F)), d with the delta-method term of the
two recentring means; test_the_reported_error_of_the_sensitivity_is_true holds it to the spread over 256 independent samples, and
shows what the deviation of d alone reports on the same samples.
"""
import json

import numpy as np
import pytest

import greeks_twin as gt

L_ = np.longdouble
N = 1 << 18
F, DF, VOL, H = 1.3, 0.97, 0.4, 1e-3 * 0.4
TTMS = (0.25, 0.5)
STRIKES = {0.25: F * np.array([0.8, 0.9, 1.0, 1.1, 1.2]), 0.5: F * np.array([0.75, 0.9, 1.0, 1.15, 1.3])}
TYPES = {0.25: np.array(["P", "P", "P", "C", "C"]), 0.5: np.array(["P", "P", "C", "C", "C"])}


@pytest.fixture(scope="module")
def twin_runs():
    z = np.random.default_rng(20261019).standard_normal(N)
    out = {}
    for ttm in TTMS:
        rows = [gt.gaussian_rows(z, ttm, v) for v in (VOL, VOL + H, VOL - H)]
        out[ttm] = gt.greeks(rows[0], F, DF, STRIKES[ttm], TYPES[ttm], [rows[1]], [rows[2]], [H])
    return out


def test_twin_agrees_with_black76_within_four_standard_errors(twin_runs):
    for ttm in TTMS:
        r = twin_runs[ttm]
        price, delta, dual, vega = gt.black76(F, STRIKES[ttm], ttm, VOL, DF, TYPES[ttm])
        for name, got, err, want in (("price", r["price"], r["stderr"], price), ("delta", r["delta"], r["delta_stderr"], delta),
                                     ("dual_delta", r["dual_delta"], r["dual_delta_stderr"], dual),
                                     ("sens sigma", r["sens"][0], r["sens_stderr"][0], vega)):
            z = np.asarray((got - want) / err, dtype=np.float64)
            print(f"ttm={ttm} {name}: z = {np.round(z, 2)}")
            assert np.all(np.abs(z) <= 4.0), (ttm, name, z)
        assert np.all(r["n_pairs"][0] == N)


def test_the_paired_error_is_orders_below_the_unpaired_one(twin_runs):
    """what the feature is for: the error of the difference against sqrt(se_up^2 + se_dn^2) / (2h) of two independent prices"""
    for ttm in TTMS:
        r = twin_runs[ttm]
        unpaired = np.sqrt(2.0) * r["stderr"] / (2 * H)
        assert np.all(r["sens_stderr"][0] < 0.1 * unpaired), (ttm, r["sens_stderr"][0] / unpaired)


def test_the_reported_error_of_the_sensitivity_is_true():
    """256 independent samples of 4 096 paths, calls and puts from deep in to deep out of the money: the spread of the
    sensitivities over the mean reported error lies in [0.8, 1.25] (a chi-square with 255 degrees puts one sigma of the ratio at
    0.045; the far strikes' fat tails add to it).  The deviation of d alone, on the same samples, reports the error of the
    call at 0.7 F -- in the money on 19 paths of 20, where d is all but s (spot_up - spot_dn), whose mean the recentring fixes --
    more than twice too large: the ratio is below 0.5 there."""
    ttm, n, strikes = 0.25, 4096, np.array([0.7, 0.85, 1.0, 1.15, 1.3])
    sens, err, err_plain = [], [], []
    for seed in range(256):
        z = np.random.default_rng(1000 + seed).standard_normal(n)
        x, xu, xd = (gt.gaussian_rows(z, ttm, v) for v in (VOL, VOL + H, VOL - H))
        sp, su, sd = (1.0 * ((np.exp(a) - np.exp(a).mean()) + 1.0) for a in (x, xu, xd))
        row = []
        for s in (1.0, -1.0):
            for k in strikes:
                d = np.maximum(s * (su - k), 0.0) - np.maximum(s * (sd - k), 0.0)
                qu, qd = np.mean(s * (su - k) > 0.0), np.mean(s * (sd - k) > 0.0)
                dt = d - s * (qu * (su - 1.0) - qd * (sd - 1.0))
                row.append((d.mean() / (2 * H), dt.std() / np.sqrt(n) / (2 * H), d.std() / np.sqrt(n) / (2 * H)))
        sens.append([r[0] for r in row])
        err.append([r[1] for r in row])
        err_plain.append([r[2] for r in row])
    spread = np.std(sens, axis=0, ddof=1)
    ratio, ratio_plain = spread / np.mean(err, axis=0), spread / np.mean(err_plain, axis=0)
    print("calls then puts, K =", strikes, "\n with the delta-method term:", np.round(ratio, 2), "\n without:", np.round(ratio_plain, 2))
    assert np.all((ratio >= 0.8) & (ratio <= 1.25)), ratio
    assert ratio_plain[0] < 0.5, ratio_plain
    # and the twin's figure is this restatement's
    o = gt.greeks(x, 1.0, 1.0, strikes, ["P"] * 5, [xu], [xd], [H])
    np.testing.assert_allclose(np.asarray(o["sens_stderr"][0], dtype=np.float64), err[-1][5:], rtol=1e-9)


def test_price_is_forward_delta_plus_strike_dual_delta(twin_runs):
    for ttm in TTMS:
        r = twin_runs[ttm]
        resid = np.abs(r["price"] - (L_(F) * r["delta"] + STRIKES[ttm].astype(L_) * r["dual_delta"]))
        bound = 64 * np.finfo(L_).eps * F                          # a few roundings of sums of 2^18 terms of size F
        print(f"ttm={ttm} homogeneity residual {np.asarray(resid, dtype=np.float64)} bound {float(bound):.1e}")
        assert np.all(resid <= bound), (ttm, resid)


def test_the_indicator_is_strict_and_nan_paths_are_out_of_the_money():
    x = np.array([0.0, 0.1, -0.2, np.nan, 0.05])
    sums = gt.spot_sums(x, 2.0)
    spot0 = 2.0 * ((1.0 - (sums[0] / sums[1]) / 2.0) + 1.0)       # the spot of path 0, as the device forms it
    r = gt.greeks(x, 2.0, 1.0, [spot0, spot0], ["C", "P"], sums=[sums])
    itm_call = int(np.sum(2.0 * ((np.exp(x[[1, 2, 4]]) - (sums[0] / sums[1]) / 2.0) + 1.0) > spot0))
    assert r["n_itm"].tolist() == [itm_call, 3 - itm_call]        # the tie and the NaN path are in neither count
    # a NaN in an up row drops that pair only
    up, dn = x.copy(), x.copy()
    up[3], dn[3], up[1] = 0.0, 0.0, np.nan
    r = gt.greeks(np.nan_to_num(x), 2.0, 1.0, [2.0], ["C"], [up], [dn], [0.01])
    assert r["n_pairs"][0].tolist() == [4]


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
def test_job_table():
    from stochvolmodels_amd.mc_greeks import HESTON_GREEK_PARAMS, LOGSV_GREEK_PARAMS, greeks_bumps, greeks_job_table
    vals = dict(sigma0=0.4, theta=0.5, kappa1=2.0, kappa2=2.5, beta=-1.0, volvol=1.2)
    names, h = greeks_bumps("logsv", vals)
    assert names == LOGSV_GREEK_PARAMS and np.array_equal(h, 1e-3 * np.abs([vals[k] for k in names]))
    base = np.array([vals[k] for k in LOGSV_GREEK_PARAMS] + [1.0, 0.9, 1.1])                    # three expiries' etas ride along
    rows = greeks_job_table("logsv", base, names, h)
    assert rows.shape == (13, 9) and np.array_equal(rows[0], base)
    for j in range(6):
        up, dn = rows[1 + 2 * j].copy(), rows[2 + 2 * j].copy()
        assert up[j] == base[j] + h[j] and dn[j] == base[j] - h[j]
        up[j] = dn[j] = base[j]
        assert np.array_equal(up, base) and np.array_equal(dn, base)                             # nothing else moves
    names, h = greeks_bumps("logsv", vals, wrt=("volvol", "sigma0"), bumps={"sigma0": 0.01})
    assert names == ("volvol", "sigma0") and np.array_equal(h, [1.2e-3, 0.01])
    rows = greeks_job_table("logsv", base[:6], names, h)
    assert (rows.shape == (5, 6) and rows[1, 5] == 1.2 + 1.2e-3 and rows[2, 5] == 1.2 - 1.2e-3 and rows[3, 0] == 0.4 + 0.01 and
            rows[4, 0] == 0.4 - 0.01)
    assert greeks_job_table("heston", [0.04, 0.04, 4.0, -0.5, 0.4], (), np.zeros(0)).shape == (1, 5)     # P = 0
    names, h = greeks_bumps("heston", dict(v0=0.04, theta=0.04, kappa=4.0, rho=-0.5, volvol=0.4))
    assert names == HESTON_GREEK_PARAMS and h[3] == 1e-3 * 0.5


def test_one_seed_and_one_call_id_reach_the_engine(monkeypatch):
    """the pricers hand the whole table to ONE engine call with one (seed, call id): a recording engine in get_engine's place"""
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.pricers import heston_pricer, logsv_pricer
    calls = []

    class Recorder:
        def price_chain_greeks_fused(self, ch, model, rows, steps, mode, nb_steps_per_year, seed, call_id):
            calls.append((model, np.array(rows), np.array(steps), mode, nb_steps_per_year, seed, call_id))
            K, P = ch["total"], len(steps)
            return ([np.zeros(sl.stop - sl.start) for sl in ch["slices"]],) * 2 + (np.zeros((5, K)), np.zeros((P, 3, K)))

    monkeypatch.setattr(logsv_pricer, "get_engine", lambda n: Recorder())
    monkeypatch.setattr(heston_pricer, "get_engine", lambda n: Recorder())
    chain = dict(ttms=np.array([0.25, 0.5]), forwards=np.array([1.0, 1.0]), discfactors=np.array([1.0, 1.0]),
                 strikes_ttms=[np.array([0.9, 1.1]), np.array([1.0])], optiontypes_ttms=[np.array(["P", "C"]), np.array(["C"])])
    out = sv.logsv_mc_chain_greeks(sv.LogSvParams(sigma0=0.4, theta=0.5, kappa1=2.0, kappa2=2.5, beta=-1.0, volvol=1.2), nb_path=64,
                                   seed=11, wrt=("sigma0", "beta"), **chain)
    model, rows, steps, mode, spy, seed, call_id = calls[-1]
    assert (model, mode, spy, seed, call_id) == ("logsv", 1, 360, 11, 0)
    assert rows.shape == (5, 8) and np.array_equal(rows[0], [0.4, 0.5, 2.0, 2.5, -1.0, 1.2, 1.0, 1.0])
    assert np.array_equal(steps, [4e-4, 1e-3]) and rows[3, 4] == -1.0 + 1e-3 and rows[4, 4] == -1.0 - 1e-3
    assert set(out) == {"price", "stderr", "delta", "delta_stderr", "dual_delta", "dual_delta_stderr", "n_itm", "sens", "sens_stderr",
                        "n_pairs"}
    assert list(out["sens"]) == ["sigma0", "beta"] and [a.shape for a in out["sens"]["beta"]] == [(2,), (1,)]
    sv.HestonPricer().model_mc_chain_greeks(sv.OptionChain(ids=np.array(["a", "b"]), ttms=chain["ttms"], forwards=chain["forwards"],
                                                           discfactors=chain["discfactors"], strikes_ttms=chain["strikes_ttms"],
                                                           optiontypes_ttms=chain["optiontypes_ttms"]),
                                            sv.HestonParams(), nb_path=64, seed=5, scheme="qe", wrt="rho")
    model, rows, steps, mode, spy, seed, call_id = calls[-1]
    assert (model, mode, seed, call_id) == ("heston", 1, 5, 0) and rows.shape == (3, 5) and rows[1, 3] == -0.5 + 5e-4


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
def test_unsupported_requests_are_refused_before_an_engine_is_touched(monkeypatch):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import VariableType
    from stochvolmodels_amd.pricers import heston_pricer, logsv_pricer
    from stochvolmodels_amd.utils import mc_payoffs

    def touched(*a, **k):
        raise AssertionError("an engine was asked for")

    for mod in (logsv_pricer, heston_pricer, mc_payoffs):
        monkeypatch.setattr(mod, "get_engine", touched)
    chain = dict(ttms=np.array([0.25]), forwards=np.array([1.0]), discfactors=np.array([1.0]), strikes_ttms=[np.array([1.0])],
                 optiontypes_ttms=[np.array(["C"])], nb_path=64, seed=1)
    lp = sv.LogSvParams(sigma0=0.2, theta=0.2, kappa1=1.0, kappa2=1.0, beta=-0.3, volvol=0.4)
    hp = sv.HestonParams(v0=0.04, theta=0.04, kappa=4.0, rho=-0.5, volvol=0.4)

    class Two:
        world, rank = 2, 0

    for fn, p in ((sv.logsv_mc_chain_greeks, lp), (sv.heston_mc_chain_greeks, hp)):
        for bad in ("IC", "IP"):
            with pytest.raises(ValueError, match="not implemented"):
                fn(p, **dict(chain, optiontypes_ttms=[np.array([bad])]))
        for vt in (VariableType.Q_VAR, VariableType.SIGMA):
            with pytest.raises(NotImplementedError):
                fn(p, variable_type=vt, **chain)
        with pytest.raises(NotImplementedError):
            fn(p, devices=2, **chain)
        with pytest.raises(NotImplementedError):
            fn(p, comm=Two(), **chain)
        with pytest.raises(ValueError, match="nosuch"):
            fn(p, wrt=("nosuch",), **chain)
    with pytest.raises(NotImplementedError):
        sv.logsv_mc_chain_greeks(lp, is_spot_measure=False, **chain)
    # a zero parameter has no relative bump ...
    flat = sv.LogSvParams(sigma0=0.2, theta=0.2, kappa1=0.0, kappa2=0.0, beta=0.0, volvol=0.0)
    for name in ("kappa1", "kappa2", "beta", "volvol"):
        with pytest.raises(ValueError, match=name):
            sv.logsv_mc_chain_greeks(flat, wrt=(name,), **chain)
    with pytest.raises(ValueError, match="rho"):
        sv.heston_mc_chain_greeks(sv.HestonParams(rho=0.0), wrt=("rho",), **chain)
    # ... and no bump may leave the domain: nothing is made one-sided
    with pytest.raises(ValueError, match="volvol"):
        sv.logsv_mc_chain_greeks(flat, wrt=("volvol",), bumps={"volvol": 1e-3}, **chain)
    with pytest.raises(ValueError, match="sigma0"):
        sv.logsv_mc_chain_greeks(lp, wrt=("sigma0",), bumps={"sigma0": 0.3}, **chain)
    with pytest.raises(ValueError, match="v0"):
        sv.heston_mc_chain_greeks(hp, wrt=("v0",), bumps={"v0": 0.05}, **chain)
    with pytest.raises(ValueError, match="rho"):
        sv.heston_mc_chain_greeks(sv.HestonParams(rho=-0.9995), **chain)
    with pytest.raises(ValueError, match="rho"):
        sv.heston_mc_chain_greeks(hp, bumps={"rho": 0.5}, **chain)
    with pytest.raises(ValueError, match="beta"):
        sv.logsv_mc_chain_greeks(lp, bumps={"beta": -1e-3}, **chain)
    with pytest.raises(ValueError, match="not implemented"):
        sv.compute_mc_vars_greeks(np.zeros(4), 1.0, np.array([1.0]), np.array(["IC"]))


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch():
    from stochvolmodels_amd import build
    build.build()
    meta = json.load(open(build.ISA_JSON))["metadata"]
    greeks = {k: v for k, v in meta.items() if "greeks" in k}
    for stem in ("greeks_payoff_kernel", "greeks_finish_kernel"):
        hit = [k for k in greeks if stem in k]
        assert len(hit) == 1, (stem, sorted(greeks))
        assert greeks[hit[0]]["scratch_bytes"] == 0, (stem, greeks[hit[0]])
    assert len(greeks) == 2
