"""
Conditional Monte Carlo Greeks under the exponential risk-premia kernel on the GPU (include/svmc_est.h;
csrc/svmc_est.hip's tilted_cond_greeks_*_kernel in libsvmc_est.so): the arithmetic against the long-double twin of
tests/tilted_cond_greeks_twin.py on uploaded (mu, cv), bit-invariance against the company of a call, gamma = 0 against row f13, the
ties to row f17 (homogeneity, the call-minus-put identities, its statistics bit for bit), the density identity across gammas, the keep
rule and the degenerate cases, the Hawkes route against svmc_hawkesjd_chain_cond plus the two C tails, the refusals, and the
calibration of the reported errors over 64 seeds.

Deviations: |device - twin| / max(|twin|, 1e-4 scale), the measure of tests/test_gpu_tilted_cond.py, with scale 1 for delta and dual
delta and 1 / F for gamma and dual gamma (values and errors alike).  Every comparison prints its deviation and the module ends by
printing the largest of each quantity (run with -s).  The bounds in TOL are measured: ten times the largest deviation seen on the
MI355X against the twin, rounded up to one digit, as profiles/tilted_cond_greeks_observed_tolerances.txt records them, none above
the project's parity bound, 1e-12.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cmc_twin as ct
import hawkes_cmc_twin as hc
import tilted_cond_greeks_twin as tg
import tilted_cond_twin as tc
from test_gpu_tilted_cond import (COUNTS, EPS, GAMMAS, QUOTE_K, QUOTE_T, TTMS, c_tail, codes_of, cond_rows, deviation, hawkes_params,
                                  nine_expiries, sample, slice_of)
from test_tilted_cond_greeks_host import CAL_GAMMAS, calibration_ratios, check_calibration

pytestmark = pytest.mark.gpu

L_ = np.longdouble
FIELDS = ("delta", "delta_stderr", "dual_delta", "dual_delta_stderr", "gamma", "gamma_stderr", "dual_gamma", "dual_gamma_stderr")
# ten times the largest deviation observed on the MI355X, rounded up to one digit (profiles/tilted_cond_greeks_observed_tolerances.txt)
TOL = dict(delta=8e-14, delta_stderr=2e-13, dual_delta=8e-14, dual_delta_stderr=2e-13, gamma=8e-14, gamma_stderr=3e-13,
           dual_gamma=8e-14, dual_gamma_stderr=3e-13)
assert max(TOL.values()) <= 1e-12      # the project's parity bound: no bound here may exceed it
PARITY_BOUND = 1e-12                   # the identities with rows f13 and f17, which hold to rounding
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def largest_deviations():
    """after the module's tests: the largest deviation of every quantity over its twin comparisons (shown with -s; the lines of
    profiles/tilted_cond_greeks_observed_tolerances.txt)"""
    yield
    for k in FIELDS:
        dev, where = SEEN.get(k, (float("nan"), ""))
        print(f"\nlargest {k} deviation: {dev:.3e}  bound {TOL[k]:.0e}  {where}", end="")
    print()


def scale_of(field, forward):
    return 1.0 / forward if "gamma" in field else 1.0


def note(field, dev, what):
    if dev >= SEEN.get(field, (-1.0, ""))[0]:
        SEEN[field] = (dev, what)
    print(f"{what}: {field} deviation {dev:.3e} (bound {TOL[field]:.0e})")
    assert dev <= TOL[field], (what, field, dev)


def check_against_twin(out, mus, cvs, forwards, strikes, types, gammas, recenter, what, fields=FIELDS):
    """every value and every error against the twin at TOL; an error the twin gives as 0 has the floor 1e-4 scale for its denominator, so
    the device's is then held below TOL x 1e-4 scale"""
    greeks, stats = out
    for g, gamma in enumerate(gammas):
        for i, (mu, cv) in enumerate(zip(mus, cvs)):
            want, st = tg.estimator(mu, cv, forwards[i], strikes[i], types[i], gamma, recenter, with_price=False)
            assert stats[g, i, 1:].tolist() == [st["n_kept"], st["n_dropped"], st["n_zero_cv"]], (what, gamma, i, stats[g, i], st)
            tag = f"{what} gamma={gamma} expiry={i} n={mu.size} K={len(strikes[i])} recenter={recenter}"
            dev_w = deviation([stats[g, i, 0]], [st["sum_weights"]], 0.0) if st["n_kept"] else abs(stats[g, i, 0])
            assert dev_w <= 1e-13, (tag, dev_w)
            for f in fields:
                if f.endswith("_stderr") and st["n_kept"] == 1:
                    assert np.all(np.ravel(greeks[g][f][i]) == 0.0), (tag, f)          # one kept path gives error 0
                note(f, deviation(np.ravel(greeks[g][f][i]), want[f], scale_of(f, forwards[i])), tag)


def upload_rows(mus, cvs):
    from stochvolmodels_amd.engine import get_engine
    n, m = mus[0].size, len(mus)
    eng = get_engine(n)
    eng.reserve_snapshots(2 * m)
    for i, (mu, cv) in enumerate(zip(mus, cvs)):
        eng.upload(eng.snapshot_ptr(i), mu)
        eng.upload(eng.snapshot_ptr(m + i), cv)
    return eng


def run_on_uploaded(mus, cvs, forwards, strikes, types, gammas, recenter, rows=None, payoffs=False):
    """the Greeks tail (payoffs=True: the payoff tail of row f17) on state uploaded from the host: expiry i's mu in snapshot row i and
    its cv in row m + i (or the expiries given)"""
    m = len(mus)
    eng = upload_rows(mus, cvs)
    rows = list(range(m)) if rows is None else rows
    fn = eng.tilted_conditional_payoffs if payoffs else eng.tilted_conditional_greeks
    return fn([forwards[i] for i in rows], [strikes[i] for i in rows], [codes_of(types[i]) for i in rows], gammas, recenter,
              mu_rows=rows, cv_rows=[m + i for i in rows])


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
# 262 147 = 1024 x 256 + 3: every block of the grid's 1024 makes a full trip and three lanes of the first one more
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 262147])
@pytest.mark.parametrize("recenter", [False, True])
def test_arithmetic_against_the_twin_over_path_counts(n, recenter):
    mu, cv = sample(n, 100 + n)
    if n == 2:
        # Two paths: one below the forward and one above it, so that no strike has EVERY path across it from the forward and the host
        # shift of a quote's sums lies between its two values.  The sample's own two rows (both above the forward, path 0 a point mass)
        # make the error's sums cancel by construction: test_errors_where_the_sums_cancel_by_construction holds those rows
        mu = np.array([-abs(mu[0]), abs(mu[1])])
    k, t = slice_of(23, 1.3)                                    # 23: six strike groups of four, the last of three
    out = run_on_uploaded([mu], [cv], [1.3], [k], [t], GAMMAS, recenter)
    check_against_twin(out, [mu], [cv], [1.3], [k], [t], GAMMAS, recenter, "paths")


@pytest.mark.parametrize("recenter", [False, True])
def test_arithmetic_over_strike_counts_and_expiries(recenter):
    mus, cvs, fw, ks, ts = nine_expiries()
    assert COUNTS == [21, 22, 23, 45, 45, 1, 22, 23, 1] and mus[0].size == 257
    out = run_on_uploaded(mus, cvs, fw, ks, ts, GAMMAS, recenter)
    check_against_twin(out, mus, cvs, fw, ks, ts, GAMMAS, recenter, "nine expiries")


def test_low_volatility_against_the_twin():
    """mu = 0.01 z, cv = 1e-4: d1 and d2 are quotients by sd = 0.01"""
    mu = 0.01 * np.random.default_rng(11).standard_normal(4099)
    cv = np.full(4099, 1e-4)
    k, t = np.array([0.5 * 1.7, 0.99 * 1.7, 1.7, 1.02 * 1.7, 2.0 * 1.7]), np.array(["C", "P", "C", "C", "P"])
    for recenter in (False, True):
        out = run_on_uploaded([mu], [cv], [1.7], [k], [t], GAMMAS, recenter)
        check_against_twin(out, [mu], [cv], [1.7], [k], [t], GAMMAS, recenter, "low volatility")


# An error is the root of sum (W d)^2 - 2 e sum W^2 d + e^2 sum W^2, d = v - shift with the header's host shift: three sums whose
# roundings -- a few eps each, eight at most together -- are left in a difference that is sum (W d)^2 / cond, so the root carries up to
# 4 eps cond and 16 eps cond bounds it with room for the quotient and the root (cond: tilted_cond_greeks_twin.estimator's
# error_conditioning).
COND_EPS = 16 * EPS


def test_errors_where_the_sums_cancel_by_construction():
    """NOT one of the issue's twin comparisons, which hold every error at TOL: the two rows of sample(2, 102) without recentring.  Both
    paths lie above the forward (path 0 a point mass), so at the three calls struck just above the forward every d = v - shift is about
    -1 and the error, a difference of d's of 1e-3, is what three sums of size 1 leave.  Values are held to TOL; an error to TOL where
    16 eps cond is within the parity bound (cond <= 281) and to 16 eps cond elsewhere, and the test asserts that the case is what it
    claims: 15 such quotes, all of them dual delta's error.  Seen on the MI355X: cond 6.0e4 to 5.6e8; the largest deviation 8.8e-9 at
    cond 4.8e7 (gamma 3), 6.2e-9 at the largest cond 5.6e8; 5.07e-11 at cond 3.4e5 (gamma -3), the figure of the first run, which held
    these rows at TOL; at most 0.051 of the bound"""
    mu, cv = sample(2, 102)
    k, t = slice_of(23, 1.3)
    greeks, stats = run_on_uploaded([mu], [cv], [1.3], [k], [t], GAMMAS, False)
    ill, worst = 0, 0.0
    for g, gamma in enumerate(GAMMAS):
        want, st = tg.estimator(mu, cv, 1.3, k, t, gamma, False, with_price=False)
        assert stats[g, 0, 1:].tolist() == [2, 0, 1]
        tag = f"cancelling sums gamma={gamma}"
        for f in FIELDS:
            got = np.ravel(greeks[g][f][0])
            if not f.endswith("_stderr"):
                note(f, deviation(got, want[f], scale_of(f, 1.3)), tag)
                continue
            cond = st["error_conditioning"][f[:-len("_stderr")]]
            assert np.all(np.isfinite(cond))
            well = COND_EPS * cond <= PARITY_BOUND
            note(f, deviation(got[well], want[f][well], scale_of(f, 1.3)), tag)
            for j in np.flatnonzero(~well):
                assert f == "dual_delta_stderr"
                dev = deviation(got[j:j + 1], want[f][j:j + 1], scale_of(f, 1.3))
                print(f"{tag}: {f} quote {j} cond {cond[j]:.1e} deviation {dev:.3e} (bound {COND_EPS * cond[j]:.1e})")
                assert dev <= COND_EPS * cond[j], (tag, f, j, dev, cond[j])
                ill, worst = ill + 1, max(worst, dev / (COND_EPS * cond[j]))
    print(f"cancelling sums: {ill} quotes beyond cond 281, the largest deviation {worst:.3f} of its bound")
    assert ill == 15


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def same(a, b, i, j):
    return all(np.array_equal(a[f][i], b[f][j], equal_nan=True) for f in FIELDS)


def test_company_does_not_change_bits():
    mus, cvs, fw, ks, ts = nine_expiries()
    for recenter in (False, True):
        all_g, all_s = run_on_uploaded(mus, cvs, fw, ks, ts, GAMMAS, recenter)
        for g, gamma in enumerate(GAMMAS):
            one, s = run_on_uploaded(mus, cvs, fw, ks, ts, [gamma], recenter)                   # the gamma alone
            assert np.array_equal(s[0], all_s[g]) and all(same(one[0], all_g[g], i, i) for i in range(9))
        for i in (0, 3, 4, 8):                                                                  # the expiry alone
            one, s = run_on_uploaded(mus, cvs, fw, ks, ts, GAMMAS, recenter, rows=[i])
            for g in range(len(GAMMAS)):
                assert same(one[g], all_g[g], 0, i) and np.array_equal(s[g, 0], all_s[g, i])
        for i, j in ((3, 0), (3, 17), (4, 44), (6, 8)):                                         # the strike alone, one gamma
            one_k, one_t = list(ks), list(ts)
            one_k[i], one_t[i] = ks[i][j:j + 1], ts[i][j:j + 1]
            one, s = run_on_uploaded(mus, cvs, fw, one_k, one_t, [GAMMAS[3]], recenter, rows=[i])
            assert all(one[0][f][0][0] == all_g[3][f][i][j] for f in FIELDS) and np.array_equal(s[0, 0], all_s[3, i])


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_gamma_zero_is_row_f13():
    """at gamma = 0 every weight is 1: the values are svmc_cmc_greeks_chain's at discount factor 1; row f13 divides the deviation by
    sqrt(n_path), this estimator by sqrt(n_kept) -- the same number where nothing is dropped (tests/test_gpu_tilted_cond.py)"""
    mus, cvs, fw, ks, ts = nine_expiries()
    for mu in mus[:2]:
        mu[[5, 100]] = [np.nan, np.inf]
    m = len(mus)
    for recenter in (False, True):
        greeks, stats = run_on_uploaded(mus, cvs, fw, ks, ts, [3.0, 0.0], recenter)
        eng = upload_rows(mus, cvs)
        cg, cst = eng.conditional_greeks(fw, np.ones(m), ks, [codes_of(t) for t in ts], recenter, mu_rows=list(range(m)),
                                         cv_rows=list(range(m, 2 * m)))
        for i in range(m):
            assert stats[1, i].tolist() == [cst[i]["n_kept"], cst[i]["n_kept"], cst[i]["n_dropped"], cst[i]["n_zero_cv"]]
            scale_e = np.sqrt(cst[i]["n_kept"] / mus[i].size)
            worst = 0.0
            for f in FIELDS:
                got = greeks[1][f][i] * (scale_e if f.endswith("_stderr") else 1.0)
                worst = max(worst, deviation(got, cg[f][i], scale_of(f, fw[i])))
            print(f"gamma = 0 against conditional_greeks recenter={recenter} expiry={i}: {worst:.3e}")
            assert worst <= PARITY_BOUND
        assert stats[1, 0, 2] == 2.0


def test_ties_to_row_f17_on_the_device():
    """price = F delta + K dual_delta with tilted_conditional_payoffs' price; delta_C - delta_P = gamma_forward / F and
    dual_delta_C - dual_delta_P = -1 at one strike; sum W, n_kept and n_dropped are its statistics, bit for bit"""
    from stochvolmodels_amd.engine import TILTED_COND_STATS_FIELDS as SF
    mus, cvs, fw, _, _ = nine_expiries()
    mus, cvs, fw = mus[:4], cvs[:4], fw[:4]
    mus[1][5] = np.nan                                           # a path f11 drops
    ks = [np.repeat(f * np.linspace(0.6, 1.5, 11), 2) for f in fw]
    ts = [np.array(["C", "P"] * 11)] * 4
    for recenter in (False, True):
        greeks, stats = run_on_uploaded(mus, cvs, fw, ks, ts, GAMMAS, recenter)
        prices, _, pstats = run_on_uploaded(mus, cvs, fw, ks, ts, GAMMAS, recenter, payoffs=True)
        for g, gamma in enumerate(GAMMAS):
            for i in range(4):
                d, dd = greeks[g]["delta"][i], greeks[g]["dual_delta"][i]
                hom = np.max(np.abs(prices[g][i] - fw[i] * d - ks[i] * dd)) / fw[i]
                gf = pstats[g, i, SF.index("gamma_forward")]
                cp_d = np.max(np.abs(d[0::2] - d[1::2] - gf / fw[i]))
                cp_k = np.max(np.abs(dd[0::2] - dd[1::2] + 1.0))
                print(f"ties recenter={recenter} gamma={gamma} expiry={i}: homogeneity {hom:.3e} F, delta_C - delta_P {cp_d:.3e}, "
                      f"dual_delta_C - dual_delta_P + 1 {cp_k:.3e}")
                assert max(hom, cp_d, cp_k) <= PARITY_BOUND
        for name, col in (("sum_weights", 0), ("n_kept", 1), ("n_dropped", 2)):
            assert np.array_equal(stats[:, :, col], pstats[:, :, SF.index(name)]), name
        assert np.all(stats[:, 1, 2] == 1.0)


def test_the_statistics_are_row_f17s_bits_where_the_weight_drops_a_path():
    """a path of mu = 120 (its weight squared overflows at gamma = 3 alone, and it carries a forward of e^120, which leaves the ties
    above nothing to hold) beside a path f11 drops: sum W, n_kept and n_dropped are tilted_conditional_payoffs' bits at every gamma"""
    from stochvolmodels_amd.engine import TILTED_COND_STATS_FIELDS as SF
    mus, cvs, fw, ks, ts = nine_expiries()
    mus, cvs, fw, ks, ts = mus[:2], cvs[:2], fw[:2], ks[:2], ts[:2]
    mus[1][[5, 100]] = [np.nan, 120.0]
    for recenter in (False, True):
        _, stats = run_on_uploaded(mus, cvs, fw, ks, ts, GAMMAS, recenter)
        _, _, pstats = run_on_uploaded(mus, cvs, fw, ks, ts, GAMMAS, recenter, payoffs=True)
        for name, col in (("sum_weights", 0), ("n_kept", 1), ("n_dropped", 2)):
            assert np.array_equal(stats[:, :, col], pstats[:, :, SF.index(name)]), name
        assert stats[:, 1, 2].tolist() == [1.0, 1.0, 1.0, 1.0, 2.0] and np.all(stats[:, 0, 2] == 0.0)


def test_the_density_identity_across_gammas():
    """W_j N(x; mu_j + gamma cv_j, cv_j) = e^{gamma x} N(x; mu_j, cv_j): pdf_gamma(x) sum W / (n_kept e^{gamma x}) is one number for
    every gamma where no path is dropped (and none has cv = 0, which adds no density)"""
    rng = np.random.default_rng(31)
    n = 3001
    mu, cv = 0.2 * rng.standard_normal(n) - 0.02, 0.01 + 0.04 * rng.random(n)
    x = np.linspace(-0.45, 0.45, 7)
    greeks, stats = run_on_uploaded([mu], [cv], [1.0], [np.exp(x)], [np.array(["C"] * 7)], GAMMAS, False)
    assert np.all(stats[:, 0, 1] == n) and np.all(stats[:, 0, 3] == 0)
    base = [np.exp(x) * greeks[g]["dual_gamma"][0] * stats[g, 0, 0] / (n * np.exp(gamma * x)) for g, gamma in enumerate(GAMMAS)]
    want = np.array([np.mean(np.exp(-(xi - mu.astype(L_)) ** 2 / (2 * cv.astype(L_))) / np.sqrt(2 * L_(np.pi) * cv.astype(L_))) for xi in x])
    for g, gamma in enumerate(GAMMAS):
        dev = float(np.max(np.abs(base[g] / base[2] - 1.0)))
        dev_w = deviation(base[g], want, 0.0)
        print(f"density identity gamma={gamma}: against gamma = 0 {dev:.3e}, against the unweighted mixture {dev_w:.3e}")
        assert dev <= PARITY_BOUND and dev_w <= PARITY_BOUND


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recenter", [False, True])
def test_the_keep_rule(recenter):
    mu, cv = sample(300, 5)
    mu[[3, 70, 130]] = [np.nan, np.inf, -np.inf]
    cv[[10, 11, 12, 13]] = [-1e-3, np.nan, np.inf, -0.0]
    k, t = slice_of(5, 1.0)
    out = run_on_uploaded([mu], [cv], [1.0], [k], [t], GAMMAS, recenter)
    check_against_twin(out, [mu], [cv], [1.0], [k], [t], GAMMAS, recenter, "keep rule")
    assert out[1][:, 0, 1].tolist() == [294.0] * 5               # six dropped by f11's rule (-0.0 is a zero variance: kept)


def test_a_weight_that_overflows_only_at_gamma_three():
    """mu = 120: f11's rule keeps the path; W^2 overflows at gamma = 3 alone.  Where the path is kept with a weight far above the
    others' (gamma = 0.5: e^60) or a forward far above theirs (gamma = 0, -1) the errors are differences of sums it dominates --
    row f17's formation, ill-conditioned there by construction -- so they are held to the twin where the path is dropped (gamma = 3)
    or weightless (gamma = -3: W = e^-360), the values everywhere"""
    mu, cv = sample(300, 5)
    mu[200], cv[200] = 120.0, 0.01
    k, t = slice_of(5, 1.0)
    out = run_on_uploaded([mu], [cv], [1.0], [k], [t], GAMMAS, False)
    assert out[1][:, 0, 1].tolist() == [300.0, 300.0, 300.0, 300.0, 299.0] and out[1][:, 0, 2].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0]
    for g, gamma in enumerate(GAMMAS):
        fields = FIELDS if gamma in (3.0, -3.0) else FIELDS[0::2]
        check_against_twin(([out[0][g]], out[1][g:g + 1]), [mu], [cv], [1.0], [k], [t], [gamma], False, "overflowing weight", fields)


def test_every_path_dropped_gives_nan_and_says_so():
    mu, cv = np.full(70, np.nan), np.full(70, 0.01)
    k, t = slice_of(9, 1.0)
    for recenter in (False, True):
        greeks, s = run_on_uploaded([mu], [cv], [1.0], [k], [t], GAMMAS, recenter)
        for g in range(len(GAMMAS)):
            assert all(np.all(np.isnan(greeks[g][f][0])) for f in FIELDS)
            assert s[g, 0].tolist() == [0.0, 0.0, 70.0, 0.0]


def test_non_positive_recentred_strikes():
    mu, cv = sample(513, 9)
    forward = 1.7
    k = forward * np.array([-0.3, -0.3, -0.05, -0.05, 0.0, 0.0, 0.9, 0.9, 1.2, 1.2])
    t = np.array(["C", "P"] * 5)
    for recenter in (False, True):
        out = run_on_uploaded([mu], [cv], [forward], [k], [t], GAMMAS, recenter)
        check_against_twin(out, [mu], [cv], [forward], [k], [t], GAMMAS, recenter, "K' <= 0")
        corr = float(tc.corr_of(mu, cv, forward, recenter))
        dead = k + corr <= 0.0
        assert dead.sum() == (6 if corr <= 0.0 else 4)
        for g in range(len(GAMMAS)):
            d = out[0][g]
            assert np.all(d["dual_delta"][0][dead & (t == "C")] == -1.0) and np.all(d["dual_delta"][0][dead & (t == "P")] == 0.0)
            assert np.all(d["delta"][0][dead & (t == "P")] == 0.0) and np.all(d["dual_gamma"][0][dead] == 0.0)
            assert all(np.all(d[f][0][dead & (t == "P")] == 0.0) for f in FIELDS)


def test_all_variances_zero():
    """every path a point mass: both gammas 0, n_zero_cv == n_kept, and delta is the weighted mean of e^mu times the indicator"""
    mu = sample(1001, 4)[0]
    cv = np.zeros(1001)
    forward = 1.1
    k, t = slice_of(9, forward)
    out = run_on_uploaded([mu], [cv], [forward], [k], [t], GAMMAS, False)
    check_against_twin(out, [mu], [cv], [forward], [k], [t], GAMMAS, False, "cv = 0")
    greeks, stats = out
    for g, gamma in enumerate(GAMMAS):
        assert stats[g, 0, 3] == stats[g, 0, 1] == 1001.0
        for f in ("gamma", "gamma_stderr", "dual_gamma", "dual_gamma_stderr"):
            assert np.all(greeks[g][f][0] == 0.0)
        w = np.exp(gamma * mu)
        sg = np.where(t == "C", 1.0, -1.0)
        ind = sg[None, :] * (sg[None, :] * (forward * np.exp(mu)[:, None] - k[None, :]) > 0.0)
        want = (w[:, None] * np.exp(mu)[:, None] * ind).sum(axis=0) / w.sum()
        assert np.max(np.abs(greeks[g]["delta"][0] - want)) <= PARITY_BOUND
        assert np.max(np.abs(greeks[g]["dual_delta"][0] + (w[:, None] * ind).sum(axis=0) / w.sum())) <= PARITY_BOUND


def test_identical_paths_have_errors_of_zero_to_rounding():
    """identical paths: the estimate is every path's value and its error is zero in exact arithmetic.  The error is the root of
    sum (W d)^2 - 2 e sum W^2 d + e^2 sum W^2, d = v - shift, a difference of three sums of n equal terms, each carrying up to
    log2(n) + 3 <= 16 roundings: up to 3 x 16 x 2^-53 = 5.4e-15 of sum (W d)^2 = n (W d)^2 is left, so the error is below
    sqrt(5.4e-15 n) W |d| / (n W) < 1e-7 |d| / sqrt(n), as tests/test_gpu_tilted_cond.py derives it for the price.  |d| <= max(e_t, 1)
    for delta and dual delta (v and its shift, an indicator, have one sign), d = v for the dual gamma"""
    forward = 1.7
    k, t = forward * np.array([0.5, 1.0, 1.3, 2.0]), np.array(["C", "C", "P", "P"])
    for n in (2, 257, 4099):
        mu, cv = np.full(n, -0.03), np.full(n, 0.0225)
        greeks, stats = run_on_uploaded([mu], [cv], [forward], [k], [t], GAMMAS, False)
        for g, gamma in enumerate(GAMMAS):
            want, _ = tg.estimator(mu[:1], cv[:1], forward, k, t, gamma, False, with_price=False)
            et = float(np.exp(mu[0] + (gamma + 0.5) * cv[0]))
            worst = 0.0
            for f in FIELDS[0::2]:
                note(f, deviation(greeks[g][f][0], want[f], scale_of(f, forward)), f"identical paths n={n} gamma={gamma}")
                d_max = max(et, 1.0) if "delta" in f else np.abs(np.asarray(want[f], dtype=np.float64))
                ratio = np.max(greeks[g][f + "_stderr"][0] / (1e-7 * d_max / np.sqrt(n) + 1e-300))
                worst = max(worst, float(ratio))
            print(f"identical paths n={n} gamma={gamma}: largest error / bound {worst:.3e}")
            assert worst <= 1.0


def test_host_array_route():
    import stochvolmodels_amd as sv
    mu, cv = sample(1000, 3)
    k, t = slice_of(7, 1.1)
    k2, t2 = k[:6].reshape(2, 3), t[:6].reshape(2, 3)
    d = sv.compute_mc_vars_greeks_conditional_with_gamma(mu, cv, 1.1, k2, t2, -1.0, recenter=True, return_stats=True)
    want, st = tg.estimator(mu, cv, 1.1, k[:6], t[:6], -1.0, True)
    assert all(d[f].shape == (2, 3) for f in tg.FIELDS) and d["stats"]["n_kept"] == 1000 and d["stats"]["n_zero_cv"] == st["n_zero_cv"] > 0
    for f in FIELDS:
        note(f, deviation(d[f].ravel(), want[f], scale_of(f, 1.1)), "host route")
    p, e = sv.compute_mc_vars_payoff_conditional_with_gamma(mu, cv, 1.1, k2, t2, -1.0, recenter=True)
    assert np.array_equal(d["price"], p) and np.array_equal(d["stderr"], e)
    ds = sv.compute_mc_vars_greeks_conditional_with_gamma(mu, cv, 1.1, k2, t2, [0.5, -1.0], recenter=True)
    assert all(np.array_equal(ds[1][f], d[f]) for f in tg.FIELDS)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def c_greeks_tail(eng, m, forwards, strikes, types, gammas, recenter, bad=None):
    """svmc_tilted_cond_greeks_chain itself on snapshot rows [0, m) and [m, 2m) of the engine -> (status, greeks [G][8][K], stats)"""
    from stochvolmodels_amd import _lib
    E = _lib.load_est()
    dp = C.POINTER(C.c_double)
    k_all = np.ascontiguousarray(np.concatenate([np.ravel(k) for k in strikes]), dtype=np.float64)
    c_all = np.ascontiguousarray(np.concatenate([codes_of(t) for t in types]))
    offs = np.concatenate([[0], np.cumsum([np.size(k) for k in strikes])]).astype(np.uintp)
    fw, gm = np.ascontiguousarray(forwards, dtype=np.float64), np.ascontiguousarray(gammas, dtype=np.float64)
    a = dict(strikes=k_all, codes=c_all, forwards=fw, gammas=gm, n_gammas=gm.size, n_expiries=m, n_path=eng.n_path, mu_null=False,
             ws_bytes=None, offs=offs)
    a.update(bad or {})
    G, K = gm.size, k_all.size                                # (of the well-formed call: the outputs are sized by it)
    nbytes = C.c_size_t(0)
    assert E.svmc_tilted_cond_greeks_workspace_bytes(eng.n_path, m, K, G, C.byref(nbytes)) == _lib.OK
    ws_ptr, _ = eng.alloc_sums((nbytes.value + 7) // 8, "tilted_cond_greeks_workspace")
    greeks, stats = np.full(G * 8 * K, -7.0), np.full(G * m * 4, -7.0)
    mus = (C.c_void_p * m)(*[None if a["mu_null"] and i == m - 1 else eng.snapshot_ptr(i) for i in range(m)])
    cvs = (C.c_void_p * m)(*[eng.snapshot_ptr(m + i) for i in range(m)])
    rc = E.svmc_tilted_cond_greeks_chain(mus, cvs, a["n_path"], a["forwards"].ctypes.data_as(dp), a["n_expiries"],
                                         a["strikes"].ctypes.data_as(dp), a["codes"].ctypes.data_as(C.POINTER(C.c_int8)),
                                         a["offs"].ctypes.data_as(C.POINTER(C.c_size_t)), a["gammas"].ctypes.data_as(dp), a["n_gammas"],
                                         int(recenter), greeks.ctypes.data_as(dp), stats.ctypes.data_as(dp), ws_ptr,
                                         nbytes.value if a["ws_bytes"] is None else a["ws_bytes"], eng.stream)
    return rc, greeks.reshape(G, 8, K), stats.reshape(G, m, 4)


def flat(rows):
    return np.concatenate([np.ravel(a) for a in rows])


def check_route_is_cond_plus_two_c_tails(p, chain, n, seed, spy, gammas, recenter):
    from stochvolmodels_amd import _lib
    from stochvolmodels_amd.engine import TILTED_COND_GREEKS_STATS_FIELDS as GSF
    from stochvolmodels_amd.engine import get_engine
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    m = len(chain["ttms"])
    kw = dict(nb_path=n, seed=seed, nb_steps_per_year=spy, recenter_forward=recenter, **chain, **p)
    out = hp.hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas(risk_premia_gammas=gammas, return_stats=True, **kw)
    route_rows = get_engine(n).download(get_engine(n).snapshot_ptr(0), 2 * m * n).reshape(2 * m, n)
    # price and error are the conditional pricer's under the kernel at the seed, bit for bit, and so is its statistics block
    pr, sd, fwds = hp.hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas(risk_premia_gammas=gammas, return_forwards=True, **kw)
    for g in range(len(gammas)):
        assert all(np.array_equal(out[g]["price"][i], pr[g][i]) and np.array_equal(out[g]["stderr"][i], sd[g][i]) for i in range(m))
        assert all(out[g]["price"][i].shape == np.shape(chain["strikes_ttms"][i]) for i in range(m))
        block = np.array([[st[k] for k in GSF] for st in out[g]["stats"]])
        assert np.array_equal(block[:, :8], fwds[g][2])
    eng, cvs = cond_rows(p, chain["ttms"], n, seed, spy)
    try:
        rows = eng.download(eng.snapshot_ptr(0), 2 * m * n).reshape(2 * m, n)
        assert np.array_equal(rows, route_rows) and np.all(rows[m:] == cvs[:, None])
        rc, prices, stderrs, stats = c_tail(eng, m, chain["forwards"], chain["strikes_ttms"], chain["optiontypes_ttms"], gammas, recenter)
        rc2, greeks, gstats = c_greeks_tail(eng, m, chain["forwards"], chain["strikes_ttms"], chain["optiontypes_ttms"], gammas, recenter)
    finally:
        eng.close()
    assert rc == _lib.OK and rc2 == _lib.OK
    K = prices.size // len(gammas)
    for g in range(len(gammas)):
        assert np.array_equal(flat(out[g]["price"]), prices[g * K:(g + 1) * K])
        assert np.array_equal(flat(out[g]["stderr"]), stderrs[g * K:(g + 1) * K])
        for r, f in enumerate(FIELDS):
            assert np.array_equal(flat(out[g][f]), greeks[g, r], equal_nan=True), (g, f)
        assert [st["n_zero_cv"] for st in out[g]["stats"]] == gstats[g, :, 3].tolist()
        assert np.array_equal(gstats[g, :, :3], stats[g][:, [7, 5, 6]])
    return out, rows


def test_the_hawkes_route_is_the_conditional_pricers_rows_and_the_two_c_tails():
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    p, n, seed, spy = hawkes_params(), 700, 21, 480
    chain = dict(ttms=TTMS, forwards=np.full(3, 1.02), discfactors=np.array([0.999, 0.995, 0.99]),
                 strikes_ttms=[QUOTE_K.reshape(2, 3), QUOTE_K, QUOTE_K], optiontypes_ttms=[QUOTE_T.reshape(2, 3), QUOTE_T, QUOTE_T])
    for recenter in (False, True):
        out, rows = check_route_is_cond_plus_two_c_tails(p, chain, n, seed, spy, GAMMAS, recenter)
        one = hp.hawkesjd_mc_chain_greeks_conditional_with_risk_premia(risk_premia_gamma=GAMMAS[1], nb_path=n, seed=seed,
                                                                       nb_steps_per_year=spy, recenter_forward=recenter,
                                                                       return_stats=True, **chain, **p)
        assert all(np.array_equal(one[f][i], out[1][f][i], equal_nan=True) for f in tg.FIELDS for i in range(3))
        assert one["stats"] == out[1]["stats"]
        check_against_twin(([{f: [np.ravel(a) for a in out[g][f]] for f in FIELDS} for g in range(5)],
                            np.array([[[st["sum_weights"], st["n_kept"], st["n_dropped"], st["n_zero_cv"]] for st in out[g]["stats"]]
                                      for g in range(5)])),
                           list(rows[:3]), list(rows[3:]), chain["forwards"], [np.ravel(k) for k in chain["strikes_ttms"]],
                           [np.ravel(t) for t in chain["optiontypes_ttms"]], GAMMAS, recenter, "Hawkes route")
    # the mu rows are the conditional pricer's at this seed (its fused call leaves the terminal state behind)
    from stochvolmodels_amd.engine import get_engine
    hp.hawkesjd_mc_chain_pricer_conditional(nb_path=n, seed=seed, nb_steps_per_year=spy, recenter=True, **chain, **p)
    assert np.array_equal(get_engine(n).get_state()[0], rows[2])
    # the class route takes the parameter set's gamma
    import stochvolmodels_amd as sv
    oc = sv.OptionChain(ids=np.array(["a", "b", "c"]), **dict(chain, strikes_ttms=[QUOTE_K] * 3, optiontypes_ttms=[QUOTE_T] * 3))
    d = sv.HawkesJDPricer().model_mc_chain_greeks_conditional_with_risk_premia(oc, sv.HawkesJDParams(**dict(p, risk_premia_gamma=-1.0)),
                                                                               nb_path=n, seed=seed, nb_steps_per_year=spy,
                                                                               recenter_forward=True)
    assert all(np.array_equal(np.ravel(d[f][i]), np.ravel(out[1][f][i])) for f in tg.FIELDS for i in range(3))


def test_seventeen_expiries():
    p, n, seed, spy = hawkes_params(), 700, 8, 365
    ttms = np.arange(1, 18) / 365.0 * 1.5                         # two steps per slice: two stepping launches, 16 + 1
    assert [g[0] for g in ct.chain_grids(ttms, spy)] == [2] * 17
    chain = dict(ttms=ttms, forwards=np.full(17, 1.0), discfactors=np.full(17, 0.99), strikes_ttms=[np.array([0.95, 1.05])] * 17,
                 optiontypes_ttms=[np.array(["P", "C"])] * 17)
    out, rows = check_route_is_cond_plus_two_c_tails(p, chain, n, seed, spy, [-1.0, 1.0], True)
    stats = np.array([[[st["sum_weights"], st["n_kept"], st["n_dropped"], st["n_zero_cv"]] for st in out[g]["stats"]] for g in range(2)])
    check_against_twin((out, stats), list(rows[:17]), list(rows[17:]), chain["forwards"], chain["strikes_ttms"], chain["optiontypes_ttms"],
                       [-1.0, 1.0], True, "17 expiries")


def test_no_jumps_is_the_closed_form():
    """without jumps every path is (mu T, sigma^2 T) and every quantity is its closed form at e_t = exp(mu + (gamma + 1/2) cv), every
    error zero in exact arithmetic.  Bounds, derived as test_gpu_tilted_cond.test_no_jumps_is_the_tilted_black_76_closed_form derives
    its own: the sums are of n equal terms W d, so sum W d / sum W returns d to a few roundings of d.  delta = e_t B_f and
    dual delta = B_k are products of normal CDFs good to a few ulp: 64 eps max(e_t, 1).  The dual gamma is phi(d2) / (K sd): d2 carries
    the logarithms' roundings divided by sd, (2 (|ln F_t| + |ln K|) / sd + 2 |d2| + sd) eps, which the exponential multiplies by |d2|;
    with the exponential, the products and the quotient, (|d2| (2 (|ln F_t| + |ln K|) / sd + 2 |d2| + sd) + 64) eps relative.  The
    errors: below 1e-7 |d| / sqrt(n) as test_identical_paths_have_errors_of_zero_to_rounding derives"""
    p = hawkes_params()
    for k in ("lambda_p", "lambda_m", "theta_p", "theta_m", "beta1_p", "beta2_p", "beta1_m", "beta2_m"):
        p[k] = 0.0
    n, spy, forward = 1000, 480, 1.02
    chain = dict(ttms=TTMS, forwards=np.full(3, forward), discfactors=np.ones(3), strikes_ttms=[QUOTE_K] * 3, optiontypes_ttms=[QUOTE_T] * 3)
    out, rows = check_route_is_cond_plus_two_c_tails(p, chain, n, 3, spy, GAMMAS, False)
    for i in range(3):
        mu, cv = rows[i], rows[3 + i]
        assert np.all(mu == mu[0]) and np.all(cv == cv[0]) and cv[0] > 0.0
        sd = np.sqrt(cv[0])
        for g, gamma in enumerate(GAMMAS):
            lr = mu[0] + (gamma + 0.5) * cv[0]
            et, ln_ft = np.exp(lr), np.log(forward) + lr
            for j, (k, t) in enumerate(zip(QUOTE_K, QUOTE_T)):
                _, d, dd, dg = (float(v[0]) for v in tg.path_terms(mu[:1], cv[:1], forward, k, t == "P", gamma))
                d2 = (ln_ft - np.log(k)) / sd - 0.5 * sd
                rel = (abs(d2) * (2.0 * (abs(ln_ft) + abs(np.log(k))) / sd + 2.0 * abs(d2) + sd) + 64.0) * EPS
                got = {f: out[g][f][i][j] for f in tg.FIELDS}
                assert abs(got["delta"] - d) <= 64 * EPS * max(et, 1.0) and abs(got["dual_delta"] - dd) <= 64 * EPS * max(et, 1.0)
                assert abs(got["dual_gamma"] - dg) <= rel * dg, (i, gamma, k, abs(got["dual_gamma"] - dg) / dg, rel)
                assert abs(got["gamma"] - (k / forward) ** 2 * dg) <= (rel + 4 * EPS) * (k / forward) ** 2 * dg
                lim = 1e-7 / np.sqrt(n)
                assert got["delta_stderr"] <= lim * max(et, 1.0) and got["dual_delta_stderr"] <= lim * max(et, 1.0)
                assert got["dual_gamma_stderr"] <= lim * dg and got["gamma_stderr"] <= lim * (k / forward) ** 2 * dg
            assert [st["n_kept"] for st in out[g]["stats"]] == [n] * 3 and [st["n_zero_cv"] for st in out[g]["stats"]] == [0] * 3


def test_every_refusal_returns_its_status_code_and_leaves_the_outputs_untouched():
    from stochvolmodels_amd import _lib
    p, n, m = hawkes_params(), 257, 3
    eng, _ = cond_rows(p, TTMS, n, 5, 480)
    try:
        ks, ts, fw = [QUOTE_K] * 3, [QUOTE_T] * 3, np.full(3, 1.02)
        rc, good, _ = c_greeks_tail(eng, m, fw, ks, ts, [0.5], False)
        assert rc == _lib.OK and np.all(np.isfinite(good))
        K = 3 * QUOTE_K.size
        nan_k, bad_c = np.concatenate(ks), np.concatenate([codes_of(t) for t in ts])
        nan_k[4], bad_c[2] = np.nan, 2
        cases = [(dict(n_path=0), _lib.ERR_INVALID_ARGUMENT), (dict(n_expiries=0), _lib.ERR_INVALID_ARGUMENT),
                 (dict(n_gammas=0), _lib.ERR_INVALID_ARGUMENT), (dict(gammas=np.zeros(17), n_gammas=17), _lib.ERR_INVALID_ARGUMENT),
                 (dict(gammas=np.array([np.nan])), _lib.ERR_INVALID_ARGUMENT), (dict(forwards=np.array([1.0, np.inf, 1.0])), _lib.ERR_INVALID_ARGUMENT),
                 (dict(forwards=np.array([1.0, 0.0, 1.0])), _lib.ERR_INVALID_ARGUMENT), (dict(forwards=np.array([1.0, -1.0, 1.0])), _lib.ERR_INVALID_ARGUMENT),
                 (dict(strikes=nan_k), _lib.ERR_INVALID_ARGUMENT), (dict(offs=np.array([1, 6, 12, K], dtype=np.uintp)), _lib.ERR_INVALID_ARGUMENT),
                 (dict(offs=np.array([0, 12, 6, K], dtype=np.uintp)), _lib.ERR_INVALID_ARGUMENT),
                 (dict(mu_null=True), _lib.ERR_INVALID_ARGUMENT), (dict(codes=bad_c.astype(np.int8)), _lib.ERR_UNKNOWN_PAYOFF),
                 (dict(ws_bytes=1024), _lib.ERR_WORKSPACE)]
        for bad, status in cases:
            rc, greeks, stats = c_greeks_tail(eng, m, fw, ks, ts, [0.5], False, bad)
            assert rc == status, (bad, rc)
            assert np.all(greeks == -7.0) and np.all(stats == -7.0), bad      # nothing came back
        rc, again, _ = c_greeks_tail(eng, m, fw, ks, ts, [0.5], False)
        assert rc == _lib.OK and np.array_equal(again, good)
    finally:
        eng.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def test_the_reported_errors_are_calibrated_on_the_device():
    """tests/test_tilted_cond_greeks_host.py's experiment through the Hawkes route: 64 seeds at 4 096 paths, the median over the 42
    quotes of (deviation of the estimate over the seeds) / (root mean square of the reported error) within the project's band, per
    gamma and quantity.  SVMC_TCG_CALIBRATION=<file> keeps every ratio (profiles/tilted_cond_greeks_observed_tolerances.txt)."""
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    p = sv.HawkesJDParams().to_dict()
    p.pop("risk_premia_gamma")
    chain, _ = hc.stat_chain(p)

    def estimate(seed):
        out = hp.hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas(risk_premia_gammas=CAL_GAMMAS, nb_path=4096, seed=seed,
                                                                              nb_steps_per_year=hc.STAT_SPY, **chain, **p)
        return {gamma: {q: (flat(out[g][q]), flat(out[g][q + "_stderr"])) for q in tg.QUANTITIES} for g, gamma in enumerate(CAL_GAMMAS)}

    lines = []
    try:
        check_calibration(calibration_ratios(estimate, 42), lambda s: (print(s), lines.append(s)))
    finally:
        if os.environ.get("SVMC_TCG_CALIBRATION"):
            with open(os.environ["SVMC_TCG_CALIBRATION"], "w") as fh:
                fh.write("\n".join(lines) + "\n")


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def recorded_figures(nb_steps_per_year=28800, nb_path=1 << 20, seed=2025):
    """the paper's slice (one month, 20 strikes 0.5 .. 1.5) under gamma = -1 and +1: the L1 distance of the bandwidth-free density,
    normalised on the grid, to hawkesjd_pdf_under_risk_kernel, beside the weighted-KDE route's; and the dual delta against a
    central strike difference of hawkesjd_chain_pricer_with_risk_premia, in reported errors"""
    import dataclasses
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    p, pricer = hp.HawkesJDParams(), sv.HawkesJDPricer()
    ttm, gammas = 1.0 / 12.0, [-1.0, 1.0]
    x = np.linspace(-0.6, 0.6, 201)
    norm = lambda v: np.asarray(v, dtype=np.float64) / np.sum(v)      # noqa: E731
    pdf, err = pricer.get_log_return_mc_pdf_conditional_under_risk_kernel(p, ttm, x, gammas, nb_path=nb_path, seed=seed, return_stderr=True,
                                                                          nb_steps_per_year=nb_steps_per_year)
    kde = pricer.get_log_return_mc_pdf_device(ttm, p, x, nb_path=nb_path, seed=seed, nb_steps_per_year=nb_steps_per_year,
                                              risk_premia_gamma=gammas)
    k = np.linspace(0.5, 1.5, 20)
    h = 1e-3
    chain = dict(ttms=np.array([ttm]), forwards=np.array([1.0]), discfactors=np.array([1.0]), optiontypes_ttms=[np.where(k <= 1.0, "P", "C")])
    kw = p.to_dict()
    kw.pop("risk_premia_gamma")
    greeks = hp.hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas(risk_premia_gammas=gammas, nb_path=nb_path, seed=seed,
                                                                             nb_steps_per_year=nb_steps_per_year, strikes_ttms=[k],
                                                                             **chain, **kw)
    out = {}
    for g, gamma in enumerate(gammas):
        mp = dataclasses.replace(p, risk_premia_gamma=gamma)
        ref = hp.hawkesjd_pdf_under_risk_kernel(mp, gamma, ttm, x)
        up = hp.hawkesjd_chain_pricer_with_risk_premia(model_params=mp, strikes_ttms=[k + h], **chain)[0]
        dn = hp.hawkesjd_chain_pricer_with_risk_premia(model_params=mp, strikes_ttms=[k - h], **chain)[0]
        fd = (up - dn) / (2.0 * h)
        out[f"gamma={gamma:+.0f}"] = dict(
            density_l1_conditional=float(np.abs(norm(pdf[g]) - norm(ref)).sum()), density_l1_weighted_kde=float(np.abs(norm(kde[g]) - norm(ref)).sum()),
            density_mass_on_grid=float(np.sum(pdf[g]) * (x[1] - x[0])), density_largest_relative_error=float(np.max(err[g] / pdf[g])),
            dual_delta=greeks[g]["dual_delta"][0].tolist(), dual_delta_stderr=greeks[g]["dual_delta_stderr"][0].tolist(),
            dual_delta_fourier_difference=fd.tolist(), strike_step=h,
            dual_delta_z=((greeks[g]["dual_delta"][0] - fd) / greeks[g]["dual_delta_stderr"][0]).tolist())
    return out


def test_recorded_figures_against_the_fourier_routes():
    """RECORDED, not asserted (profiles/hawkes_tilted_cond_greeks_z_scores.json, written with SVMC_TCG_Z_SCORES=<file>): the Fourier
    density's own accuracy is unpinned in this project (tests/test_gpu_kde_weighted.py holds it only to a mass of 1 +- 1e-2) and the
    difference quotient's truncation error is not known in advance, so neither figure is given a bound; the test asserts only that
    the figures exist and are finite."""
    z = recorded_figures()
    print("conditional Greeks under the kernel, recorded figures:", json.dumps(z))
    if os.environ.get("SVMC_TCG_Z_SCORES"):
        with open(os.environ["SVMC_TCG_Z_SCORES"], "w") as fh:
            json.dump(z, fh, indent=1)
    for v in z.values():
        assert np.isfinite(v["density_l1_conditional"]) and np.isfinite(v["density_l1_weighted_kde"])
        assert len(v["dual_delta_z"]) == 20 and np.all(np.isfinite(v["dual_delta_z"]))
