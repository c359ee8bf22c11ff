"""
Conditional Monte Carlo under the exponential risk-premia kernel on the GPU (include/svmc_ext.h; csrc/svmc_ext.hip's
tilted_cond_*_kernel in libsvmc_ext.so): the arithmetic against the long-double twin of tests/tilted_cond_twin.py on uploaded (mu, cv),
bit-invariance against the company of a call, the identities with rows f11 (gamma = 0) and f8 (cv = 0), the keep rule and the
degenerate cases, the standard error under cancellation, the Hawkes route against svmc_hawkesjd_chain_cond plus the C tail, and the
Monte Carlo against the Fourier pricer under the kernel and against the plain estimator under it.

Deviations: |device - twin| / max(|twin|, 1e-4 scale), the measure of tests/test_gpu_tilted.py with its scales (the forward for
prices, gamma forwards and their errors; 1 for the normalizer and its error; none for the effective sample size).  Every comparison
prints its deviation and the module ends by printing the largest of each quantity (run with -s).  The bounds in TOL are measured: ten
times the largest deviation seen on the MI355X against the twin, rounded up to one digit, as
profiles/tilted_cond_observed_tolerances.txt records them, none above the project's parity bound for prices and states, 1e-12.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cmc_twin as ct
import tilted_cond_twin as tc

pytestmark = pytest.mark.gpu

L_ = np.longdouble
EPS = 2.0 ** -52
GAMMAS = [-3.0, -1.0, 0.0, 0.5, 3.0]
FIELDS = ("price", "stderr", "normalizer", "normalizer_stderr", "gamma_forward", "gamma_forward_stderr", "effective_sample_size")
# ten times the largest deviation observed on the MI355X, rounded up to one digit (profiles/tilted_cond_observed_tolerances.txt)
TOL = dict(price=3e-13, stderr=2e-13, normalizer=3e-15, normalizer_stderr=8e-15, gamma_forward=6e-14, gamma_forward_stderr=9e-15,
           effective_sample_size=6e-15)
assert max(TOL.values()) <= 1e-12      # the project's parity bound for prices and states: no bound here may exceed it
PARITY_BOUND = 1e-12                   # the identities with rows f8 and f11, which hold to rounding
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def largest_deviations():
    """after the module's tests: the largest deviation of every quantity over its twin comparisons (shown with -s; the lines of
    profiles/tilted_cond_observed_tolerances.txt)"""
    yield
    for k in FIELDS:
        dev, where = SEEN.get(k, (float("nan"), ""))
        print(f"\nlargest {k} deviation: {dev:.3e}  bound {TOL[k]:.0e}  {where}", end="")
    print()


def deviation(got, want, scale):
    want = np.asarray(want, dtype=L_)
    got = np.asarray(got, dtype=L_)
    if np.any(np.isnan(want)):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        got, want = got[~np.isnan(want)], want[~np.isnan(want)]
    if want.size == 0:
        return 0.0
    floor = 1e-4 * scale if scale else 0.0
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), floor))) if floor else float(np.max(np.abs(got - want) / np.abs(want)))


def note(field, dev, what):
    if dev >= SEEN.get(field, (-1.0, ""))[0]:
        SEEN[field] = (dev, what)
    print(f"{what}: {field} deviation {dev:.3e} (bound {TOL[field]:.0e})")
    assert dev <= TOL[field], (what, field, dev)


def check_against_twin(out, mus, cvs, forwards, strikes, types, gammas, recenter, what):
    prices, stderrs, stats = out
    from stochvolmodels_amd.engine import TILTED_COND_STATS_FIELDS as SF
    for g, gamma in enumerate(gammas):
        for i, (mu, cv) in enumerate(zip(mus, cvs)):
            p, e, st = tc.estimator(mu, cv, forwards[i], strikes[i], types[i], gamma, recenter)
            row = dict(zip(SF, stats[g, i]))
            assert (row["n_kept"], row["n_dropped"]) == (st["n_kept"], st["n_dropped"]), (what, gamma, i)
            tag = f"{what} gamma={gamma} expiry={i} n={mu.size} K={len(strikes[i])} recenter={recenter}"
            note("price", deviation(prices[g][i], p, forwards[i]), tag)
            note("stderr", deviation(stderrs[g][i], e, forwards[i]), tag)
            for k in FIELDS[2:]:
                scale = forwards[i] if k.startswith("gamma_forward") else (1.0 if k.startswith("normalizer") else 0.0)
                note(k, deviation([row[k]], [st[k]], scale), tag)


def codes_of(types):
    return np.array([0 if t == "C" else 1 for t in np.ravel(types)], dtype=np.int8)


def run_on_uploaded(mus, cvs, forwards, strikes, types, gammas, recenter, rows=None, shifts=None):
    """the tail on state uploaded from the host: expiry i's mu in snapshot row i and its cv in row m + i (or the expiries given)"""
    from stochvolmodels_amd.engine import get_engine
    n, m = mus[0].size, len(mus)
    eng = get_engine(n)
    eng.reserve_snapshots(2 * m)
    for i, (mu, cv) in enumerate(zip(mus, cvs)):
        eng.upload(eng.snapshot_ptr(i), mu)
        eng.upload(eng.snapshot_ptr(m + i), cv)
    rows = list(range(m)) if rows is None else rows
    return eng.tilted_conditional_payoffs([forwards[i] for i in rows], [strikes[i] for i in rows], [codes_of(types[i]) for i in rows],
                                          gammas, recenter, mu_rows=rows, cv_rows=[m + i for i in rows], shifts=shifts)


def slice_of(n_strikes, forward):
    """n_strikes strikes around the forward, puts at or below it, calls above"""
    k = forward * (np.linspace(0.6, 1.5, n_strikes) if n_strikes > 1 else np.array([1.05]))
    return k, np.where(k <= forward, "P", "C")


def sample(n, seed, vol=0.2, cv_max=0.05):
    """(mu, cv): mu normal around -vol^2 / 2, cv uniform in [0, cv_max] per path with every seventh an exact zero"""
    rng = np.random.default_rng(seed)
    mu = vol * rng.standard_normal(n) - 0.5 * vol * vol
    cv = cv_max * rng.random(n)
    cv[::7] = 0.0
    return mu, cv


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
# 262 147 = 1024 x 256 + 3: every block of the grid's 1024 makes a full trip and three lanes of the first one more
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 262147])
@pytest.mark.parametrize("recenter", [False, True])
def test_arithmetic_against_the_twin_over_path_counts(n, recenter):
    mu, cv = sample(n, 100 + n)
    k, t = slice_of(23, 1.3)                                    # 23: three strike groups of the tail, two of row f8's
    out = run_on_uploaded([mu], [cv], [1.3], [k], [t], GAMMAS, recenter)
    check_against_twin(out, [mu], [cv], [1.3], [k], [t], GAMMAS, recenter, "paths")


COUNTS = [21, 22, 23, 45, 45, 1, 22, 23, 1]


def nine_expiries(n=257):
    forwards = [1.0 + 0.05 * i for i in range(9)]
    mcs = [sample(n, 7 + i, 0.1 + 0.03 * i, 0.01 + 0.005 * i) for i in range(9)]
    ks, ts = zip(*[slice_of(c, f) for c, f in zip(COUNTS, forwards)])
    return [a for a, _ in mcs], [b for _, b in mcs], forwards, list(ks), list(ts)


@pytest.mark.parametrize("recenter", [False, True])
def test_arithmetic_over_strike_counts_and_expiries(recenter):
    mus, cvs, fw, ks, ts = nine_expiries()
    out = run_on_uploaded(mus, cvs, fw, ks, ts, GAMMAS, recenter)
    check_against_twin(out, mus, cvs, fw, ks, ts, GAMMAS, recenter, "nine expiries")


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def test_company_does_not_change_bits():
    mus, cvs, fw, ks, ts = nine_expiries()
    for recenter in (False, True):
        all_p, all_e, all_s = run_on_uploaded(mus, cvs, fw, ks, ts, GAMMAS, recenter)
        for g, gamma in enumerate(GAMMAS):
            p, e, s = run_on_uploaded(mus, cvs, fw, ks, ts, [gamma], recenter)                 # the gamma alone
            assert np.array_equal(s[0], all_s[g], equal_nan=True)
            for i in range(9):
                assert np.array_equal(p[0][i], all_p[g][i]) and np.array_equal(e[0][i], all_e[g][i])
        for i in (0, 3, 4, 8):                                                                  # the expiry alone
            p, e, s = run_on_uploaded(mus, cvs, fw, ks, ts, GAMMAS, recenter, rows=[i])
            for g in range(len(GAMMAS)):
                assert np.array_equal(p[g][0], all_p[g][i]) and np.array_equal(e[g][0], all_e[g][i])
                assert np.array_equal(s[g, 0], all_s[g, i])
        for i, j in ((3, 0), (3, 17), (4, 44), (6, 8)):                                         # the strike alone, one gamma
            one_k, one_t = list(ks), list(ts)
            one_k[i], one_t[i] = ks[i][j:j + 1], ts[i][j:j + 1]
            p, e, s = run_on_uploaded(mus, cvs, fw, one_k, one_t, [GAMMAS[3]], recenter, rows=[i])
            assert p[0][0][0] == all_p[3][i][j] and e[0][0][0] == all_e[3][i][j] and np.array_equal(s[0, 0], all_s[3, i])


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def forward_block(eng, m, strike_counts, n_gammas):
    """[m][4] = (sum (e - 1), sum (e - 1)^2, kept, corr) of the last tail call on this engine, read where csrc/svmc_ext.hip's
    tc_workspace puts it: after the image (40 bytes an expiry, 16 a strike group of up to 8, three doubles a strike, the gammas) and
    the two device-computed strike columns"""
    K = int(sum(strike_counts))
    G = int(sum(max((c + 7) // 8, 1) for c in strike_counts))
    ptr, _ = eng.alloc_sums(1, "tilted_cond_workspace")
    return eng.download(ptr + 40 * m + 16 * G + 8 * (3 * K + n_gammas) + 16 * K, 4 * m).reshape(m, 4)


def test_gamma_zero_is_the_conditional_estimator_and_corr_is_its_corr():
    from stochvolmodels_amd.engine import get_engine
    mus, cvs, fw, ks, ts = nine_expiries()
    for mu in mus[:2]:
        mu[[5, 100]] = [np.nan, np.inf]                          # f11's rule drops them from corr as well
    m = len(mus)
    for recenter in (False, True):
        p, e, s = run_on_uploaded(mus, cvs, fw, ks, ts, [3.0, 0.0], recenter)
        eng = get_engine(mus[0].size)
        fwd = forward_block(eng, m, COUNTS, 2)
        cp, ce, cst = eng.conditional_payoffs(fw, np.ones(m), ks, [codes_of(t) for t in ts], recenter, mu_rows=list(range(m)),
                                              cv_rows=list(range(m, 2 * m)))
        for i in range(m):
            # bit for bit, whatever gammas the call carried: f11's unweighted recentring over the paths f11 keeps
            assert fwd[i, 3] == cst[i]["corr"] and fwd[i, 2] == cst[i]["n_kept"], (recenter, i, fwd[i], cst[i])
            # (row f11 divides the deviation by sqrt(n_path), this estimator by sqrt(n_kept): the same number where nothing is dropped)
            scale_e = np.sqrt(cst[i]["n_kept"] / mus[i].size)
            dp, de = deviation(p[1][i], cp[i], fw[i]), deviation(e[1][i] * scale_e, ce[i], fw[i])
            print(f"gamma = 0 against conditional_payoffs recenter={recenter} expiry={i}: prices {dp:.3e}, stderrs {de:.3e}")
            assert dp <= PARITY_BOUND and de <= PARITY_BOUND
            assert s[1, i, 0] == 1.0 and s[1, i, 4] == s[1, i, 5] == cst[i]["n_kept"]     # normalizer 1, effective sample size n_kept
    assert np.any(fwd[:, 3] != 0.0)


def test_zero_variance_is_the_plain_estimator_under_the_kernel():
    from stochvolmodels_amd.engine import get_engine
    mus, _, fw, ks, ts = nine_expiries()
    mus, fw, ks, ts = mus[:3], fw[:3], ks[:3], ts[:3]
    zeros = [np.zeros(mus[0].size)] * 3
    for recenter in (False, True):
        p, e, s = run_on_uploaded(mus, zeros, fw, ks, ts, GAMMAS, recenter)
        tp, te, tst = get_engine(mus[0].size).tilted_payoffs(fw, ks, [codes_of(t) for t in ts], GAMMAS, recenter, snap_rows=[0, 1, 2])
        for g in range(len(GAMMAS)):
            for i in range(3):
                dp, de = deviation(p[g][i], tp[g][i], fw[i]), deviation(e[g][i], te[g][i], fw[i])
                ds = [deviation([s[g, i, c]], [tst[g, i, c]], sc) for c, sc in enumerate((1.0, 1.0, fw[i], fw[i], 0.0))]
                print(f"cv = 0 against tilted_payoffs recenter={recenter} gamma={GAMMAS[g]} expiry={i}: prices {dp:.3e}, stderrs {de:.3e}, "
                      f"stats {max(ds):.3e}")
                assert max([dp, de] + ds) <= PARITY_BOUND
                assert np.array_equal(s[g, i, 5:7], tst[g, i, 5:7]) and deviation([s[g, i, 7]], [tst[g, i, 7]], 0.0) <= PARITY_BOUND


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recenter", [False, True])
def test_the_keep_rule(recenter):
    from stochvolmodels_amd.engine import TILTED_COND_STATS_FIELDS as SF
    mu, cv = sample(300, 5)
    mu[[3, 70, 130]] = [np.nan, np.inf, -np.inf]
    cv[[10, 11, 12, 13]] = [-1e-3, np.nan, np.inf, -0.0]
    k, t = slice_of(5, 1.0)
    out = run_on_uploaded([mu], [cv], [1.0], [k], [t], GAMMAS, recenter)
    check_against_twin(out, [mu], [cv], [1.0], [k], [t], GAMMAS, recenter, "keep rule")
    assert out[2][:, 0, SF.index("n_kept")].tolist() == [294.0] * 5      # six dropped by f11's rule (-0.0 is a zero variance: kept)


def test_a_weight_that_overflows_only_at_gamma_three():
    """mu = 120: e = exp(mu + cv / 2) is finite and f11's rule keeps the path; W^2 = exp(2 gamma mu + ...) overflows at gamma = 3 alone.
    Where the path is kept with a weight far above the others' (gamma = 0.5: e^60) or a forward far above theirs (gamma = 0, -1) the two
    errors and the normalizer's are differences of sums it dominates -- row f8's formation, ill-conditioned there by construction -- so
    those three are held to the twin where the path is dropped (gamma = 3) or weightless (gamma = -3: W = e^-360), the ratios everywhere"""
    from stochvolmodels_amd.engine import TILTED_COND_STATS_FIELDS as SF
    mu, cv = sample(300, 5)
    mu[200], cv[200] = 120.0, 0.01
    k, t = slice_of(5, 1.0)
    prices, stderrs, stats = run_on_uploaded([mu], [cv], [1.0], [k], [t], GAMMAS, False)
    assert stats[:, 0, SF.index("n_kept")].tolist() == [300.0, 300.0, 300.0, 300.0, 299.0]
    assert stats[:, 0, SF.index("n_dropped")].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0]
    for g, gamma in enumerate(GAMMAS):
        p, e, st = tc.estimator(mu, cv, 1.0, k, t, gamma, False)
        row = dict(zip(SF, stats[g, 0]))
        assert (row["n_kept"], row["n_dropped"]) == (st["n_kept"], st["n_dropped"])
        tag = f"overflowing weight gamma={gamma}"
        note("price", deviation(prices[g][0], p, 1.0), tag)
        note("normalizer", deviation([row["normalizer"]], [st["normalizer"]], 1.0), tag)
        note("effective_sample_size", deviation([row["effective_sample_size"]], [st["effective_sample_size"]], 0.0), tag)
        if gamma in (3.0, -3.0):
            note("gamma_forward", deviation([row["gamma_forward"]], [st["gamma_forward"]], 1.0), tag)
        else:                                                    # (the forward's own scale is e^120 here)
            note("gamma_forward", deviation([row["gamma_forward"]], [st["gamma_forward"]], 0.0), tag)
        if gamma == 3.0:
            note("stderr", deviation(stderrs[g][0], e, 1.0), tag)
            for f, sc in (("normalizer_stderr", 1.0), ("gamma_forward_stderr", 1.0)):
                note(f, deviation([row[f]], [st[f]], sc), tag)


def test_every_path_dropped_gives_nan_prices_and_says_so():
    from stochvolmodels_amd.engine import TILTED_COND_STATS_FIELDS as SF
    mu, cv = np.full(70, np.nan), np.full(70, 0.01)
    k, t = slice_of(9, 1.0)
    for recenter in (False, True):
        p, e, s = run_on_uploaded([mu], [cv], [1.0], [k], [t], GAMMAS, recenter)
        for g in range(len(GAMMAS)):
            assert np.all(np.isnan(p[g][0])) and np.all(np.isnan(e[g][0]))
            assert s[g, 0, SF.index("n_kept")] == 0.0 and s[g, 0, SF.index("n_dropped")] == 70.0 and s[g, 0, SF.index("sum_weights")] == 0.0


def test_non_positive_recentred_strikes_and_put_call_parity():
    from stochvolmodels_amd.engine import TILTED_COND_STATS_FIELDS as SF
    mu, cv = sample(513, 9)
    forward = 1.7
    # K' = K + corr <= 0: negative strikes (corr is about +0.01 F here), and K = 0, whose K' is corr itself
    k = forward * np.array([-0.3, -0.3, -0.05, -0.05, 0.0, 0.0, 0.9, 0.9, 1.2, 1.2])
    t = np.array(["C", "P"] * 5)
    for recenter in (False, True):
        out = run_on_uploaded([mu], [cv], [forward], [k], [t], GAMMAS, recenter)
        check_against_twin(out, [mu], [cv], [forward], [k], [t], GAMMAS, recenter, "K' <= 0")
        corr = float(tc.corr_of(mu, cv, forward, recenter))
        assert (corr != 0.0) == recenter and np.sum(k + corr <= 0.0) == (6 if corr <= 0.0 else 4), corr
        p, _, s = out
        for g, gamma in enumerate(GAMMAS):
            parity = p[g][0][0::2] - p[g][0][1::2] - (s[g, 0, SF.index("gamma_forward")] - k[0::2])
            print(f"put-call parity gamma={gamma} recenter={recenter}: {np.max(np.abs(parity)) / forward:.3e} F")
            assert np.max(np.abs(parity)) <= 1e-12 * forward
            assert np.all(p[g][0][1::2][k[1::2] + corr <= 0.0] == 0.0)      # a put at K' <= 0 pays nothing


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def test_the_standard_error_survives_cancellation():
    """identical paths: the estimate is every path's price and its error is zero.  The sums are of d = B - shift (include/svmc_ext.h):
    with the shift at the price -- the twin's, rounded to double -- the device's error stays below 1e-13 F at every path count"""
    forward = 1.7
    k, t = forward * np.array([0.5, 1.0, 1.3, 2.0]), np.array(["C", "C", "P", "P"])
    for n in (2, 257, 4099):
        mu, cv = np.full(n, -0.03), np.full(n, 0.0225)
        for gamma in GAMMAS:
            want = tc.estimator(mu[:1], cv[:1], forward, k, t, gamma)[0]
            p, e, s = run_on_uploaded([mu], [cv], [forward], [k], [t], [gamma], False, shifts=[want.astype(np.float64)])
            print(f"identical paths n={n} gamma={gamma}: largest error {np.max(e[0][0]) / forward:.3e} F, price deviation "
                  f"{deviation(p[0][0], want, forward):.3e}")
            assert np.all(e[0][0] <= 1e-13 * forward)
            note("price", deviation(p[0][0], want, forward), f"identical paths n={n} gamma={gamma}")


def test_low_volatility_against_the_twin():
    """mu = 0.01 z, cv = 1e-4 and a call at half the forward: the price is 0.5 F +- 1 %, its error two orders below it"""
    mu = 0.01 * np.random.default_rng(11).standard_normal(4099)
    cv = np.full(4099, 1e-4)
    k, t = np.array([0.5 * 1.7, 1.7, 2.0 * 1.7]), np.array(["C", "C", "P"])
    for recenter in (False, True):
        out = run_on_uploaded([mu], [cv], [1.7], [k], [t], GAMMAS, recenter)
        check_against_twin(out, [mu], [cv], [1.7], [k], [t], GAMMAS, recenter, "low volatility")


def test_host_array_route():
    import stochvolmodels_amd as sv
    mu, cv = sample(1000, 3)
    k, t = slice_of(7, 1.1)
    k2, t2 = k[:6].reshape(2, 3), t[:6].reshape(2, 3)
    p, e, st = sv.compute_mc_vars_payoff_conditional_with_gamma(mu, cv, 1.1, k2, t2, -1.0, recenter=True, return_stats=True)
    assert p.shape == e.shape == (2, 3) and isinstance(st["n_kept"], int) and st["n_kept"] == 1000
    bp, be, bst = tc.estimator(mu, cv, 1.1, k[:6], t[:6], -1.0, True)
    note("price", deviation(p.ravel(), bp, 1.1), "host route")
    note("stderr", deviation(e.ravel(), be, 1.1), "host route")
    note("gamma_forward", deviation([st["gamma_forward"]], [bst["gamma_forward"]], 1.1), "host route")
    ps, es = sv.compute_mc_vars_payoff_conditional_with_gamma(mu, cv, 1.1, k2, t2, [0.5, -1.0], recenter=True)
    assert np.array_equal(ps[1], p) and np.array_equal(es[1], e)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def hawkes_params(name="hawkes_mc"):
    import hawkes_twin as ht
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    return dict(zip(ht.PARAM_NAMES, (float(v) for v in g["params"])))


def c_tail(eng, m, forwards, strikes, types, gammas, recenter, bad=None):
    """svmc_tilted_cond_payoff_chain itself on snapshot rows [0, m) and [m, 2m) of the engine -> (status, prices, stderrs, stats)"""
    from stochvolmodels_amd import _lib
    from stochvolmodels_amd.engine import payoff_shifts
    E = _lib.load_ext()
    dp = C.POINTER(C.c_double)
    k_all = np.ascontiguousarray(np.concatenate([np.ravel(k) for k in strikes]), dtype=np.float64)
    c_all = np.ascontiguousarray(np.concatenate([codes_of(t) for t in types]))
    sh = np.ascontiguousarray(np.concatenate([payoff_shifts(np.ravel(k), codes_of(t), float(f), 1) for k, t, f in zip(strikes, types, forwards)]))
    offs = np.concatenate([[0], np.cumsum([np.size(k) for k in strikes])]).astype(np.uintp)
    fw, gm = np.ascontiguousarray(forwards, dtype=np.float64), np.ascontiguousarray(gammas, dtype=np.float64)
    a = dict(strikes=k_all, codes=c_all, shifts=sh, forwards=fw, gammas=gm, n_gammas=gm.size, n_expiries=m,
             n_path=eng.n_path, mu_null=False, ws_bytes=None)
    a.update(bad or {})
    G, K = gm.size, k_all.size                                # (of the well-formed call: the outputs are sized by it)
    nbytes = C.c_size_t(0)
    assert E.svmc_tilted_cond_workspace_bytes(eng.n_path, m, K, G, C.byref(nbytes)) == _lib.OK
    ws_ptr, _ = eng.alloc_sums((nbytes.value + 7) // 8, "tilted_cond_workspace")
    prices, stderrs, stats = np.full(G * K, -7.0), np.full(G * K, -7.0), np.full(G * m * 8, -7.0)
    mus = (C.c_void_p * m)(*[None if a["mu_null"] and i == m - 1 else eng.snapshot_ptr(i) for i in range(m)])
    cvs = (C.c_void_p * m)(*[eng.snapshot_ptr(m + i) for i in range(m)])
    rc = E.svmc_tilted_cond_payoff_chain(mus, cvs, a["n_path"], a["forwards"].ctypes.data_as(dp), a["n_expiries"],
                                         a["strikes"].ctypes.data_as(dp), a["codes"].ctypes.data_as(C.POINTER(C.c_int8)),
                                         a["shifts"].ctypes.data_as(dp), offs.ctypes.data_as(C.POINTER(C.c_size_t)),
                                         a["gammas"].ctypes.data_as(dp), a["n_gammas"], int(recenter), prices.ctypes.data_as(dp),
                                         stderrs.ctypes.data_as(dp), stats.ctypes.data_as(dp), ws_ptr,
                                         nbytes.value if a["ws_bytes"] is None else a["ws_bytes"],
                                         eng.stream)
    return rc, prices, stderrs, stats.reshape(G, m, 8)


def cond_rows(p, ttms, n, seed, spy):
    """svmc_hawkesjd_chain_cond from the origin on an engine of its own: mu in rows [0, m), cv in [m, 2m) -> (engine, host cvs)"""
    from stochvolmodels_amd.engine import HipEngine
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    grids = ct.chain_grids(ttms, spy)
    eng = HipEngine(n)
    eng.set_state(np.zeros(n), np.full(n, p["lambda_p"]), np.full(n, p["lambda_m"]))
    cvs = eng.hawkesjd_chain_cond([g[0] for g in grids], [g[1] for g in grids], hp.params_block(**p), seed, 0)
    return eng, cvs


def check_route_is_cond_plus_c_tail(p, chain, n, seed, spy, gammas, recenter):
    from stochvolmodels_amd import _lib
    from stochvolmodels_amd.engine import get_engine
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    m = len(chain["ttms"])
    pr, sd, fwds = hp.hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas(
        risk_premia_gammas=gammas, nb_path=n, seed=seed, nb_steps_per_year=spy, recenter_forward=recenter, return_forwards=True,
        **chain, **p)
    route_rows = get_engine(n).download(get_engine(n).snapshot_ptr(0), 2 * m * n).reshape(2 * m, n)
    eng, cvs = cond_rows(p, chain["ttms"], n, seed, spy)
    try:
        rows = eng.download(eng.snapshot_ptr(0), 2 * m * n).reshape(2 * m, n)
        assert np.array_equal(rows, route_rows) and np.all(rows[m:] == cvs[:, None])
        rc, prices, stderrs, stats = c_tail(eng, m, chain["forwards"], chain["strikes_ttms"], chain["optiontypes_ttms"], gammas, recenter)
    finally:
        eng.close()
    assert rc == _lib.OK
    K = prices.size // len(gammas)
    for g in range(len(gammas)):
        assert np.array_equal(np.concatenate([np.ravel(a) for a in pr[g]]), prices[g * K:(g + 1) * K])
        assert np.array_equal(np.concatenate([np.ravel(a) for a in sd[g]]), stderrs[g * K:(g + 1) * K])
        assert np.array_equal(fwds[g][2], stats[g]) and np.array_equal(fwds[g][0], stats[g][:, 0]) and np.array_equal(fwds[g][1], stats[g][:, 2])
    return pr, sd, fwds, rows


TTMS = np.array([1.0 / 52.0, 1.0 / 12.0, 0.25])
QUOTE_K, QUOTE_T = np.array([0.85, 0.95, 1.0, 1.02, 1.1, 1.25]), np.array(["P", "P", "P", "C", "C", "C"])


def test_the_hawkes_route_steps_the_conditional_pricers_rows_and_is_the_two_c_calls():
    from stochvolmodels_amd.engine import get_engine
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    p, n, seed, spy = hawkes_params(), 700, 21, 480
    chain = dict(ttms=TTMS, forwards=np.full(3, 1.02), discfactors=np.array([0.999, 0.995, 0.99]), strikes_ttms=[QUOTE_K] * 3,
                 optiontypes_ttms=[QUOTE_T] * 3)
    for recenter in (False, True):
        pr, sd, fwds, rows = check_route_is_cond_plus_c_tail(p, chain, n, seed, spy, GAMMAS, recenter)
        # one gamma is the list form at that gamma
        p1, e1, f1 = hp.hawkesjd_mc_chain_pricer_conditional_with_risk_premia(risk_premia_gamma=GAMMAS[1], nb_path=n, seed=seed,
                                                                              nb_steps_per_year=spy, recenter_forward=recenter,
                                                                              return_forwards=True, **chain, **p)
        for i in range(3):
            assert np.array_equal(p1[i], pr[1][i]) and np.array_equal(e1[i], sd[1][i])
        assert np.array_equal(f1[2], fwds[1][2])
    # the rows are the conditional pricer's at this seed: the same terminal state, bit for bit, the last mu row is it, and the
    # conditional tail on the route's rows gives the conditional pricer's prices
    eng = get_engine(n)
    state = eng.get_state()
    tail = eng.conditional_payoffs(chain["forwards"], chain["discfactors"], chain["strikes_ttms"], [codes_of(t) for t in chain["optiontypes_ttms"]],
                                   True, mu_rows=[0, 1, 2], cv_rows=[3, 4, 5])
    cp, ce = hp.hawkesjd_mc_chain_pricer_conditional(nb_path=n, seed=seed, nb_steps_per_year=spy, recenter=True, **chain, **p)
    for a, b in zip(state, eng.get_state()):
        assert np.array_equal(a, b)
    assert np.array_equal(state[0], rows[2])
    for i in range(3):
        assert np.array_equal(tail[0][i], cp[i]) and np.array_equal(tail[1][i], ce[i])


def test_seventeen_expiries():
    p, n, seed, spy = hawkes_params(), 700, 8, 365
    ttms = np.arange(1, 18) / 365.0 * 1.5                         # two steps per slice: two stepping launches, 16 + 1
    assert [g[0] for g in ct.chain_grids(ttms, spy)] == [2] * 17
    chain = dict(ttms=ttms, forwards=np.full(17, 1.0), discfactors=np.full(17, 0.99), strikes_ttms=[np.array([0.95, 1.05])] * 17,
                 optiontypes_ttms=[np.array(["P", "C"])] * 17)
    pr, sd, fwds, rows = check_route_is_cond_plus_c_tail(p, chain, n, seed, spy, [-1.0, 1.0], True)
    out = ([[np.asarray(a) for a in g] for g in pr], [[np.asarray(a) for a in g] for g in sd], np.stack([f[2] for f in fwds]))
    check_against_twin(out, list(rows[:17]), list(rows[17:]), chain["forwards"], chain["strikes_ttms"], chain["optiontypes_ttms"],
                       [-1.0, 1.0], True, "17 expiries")


def test_no_jumps_is_the_tilted_black_76_closed_form():
    """without jumps every path is (mu T, sigma^2 T): the price is the Black-76 price of F exp(mu + (gamma + 1/2) cv) at variance cv,
    every error zero in exact arithmetic.  Bounds: the sums are of n equal terms W d, so sum W d / sum W returns d to a few roundings of d,
    |d| <= max(F_t, K), and the Black-76 value itself is a difference of two products of that size by normal CDFs good to a few ulp: 64
    eps max(F_t, K) for the price.  The error is the root of a difference of three such sums of squares, each carrying up to
    log2(n) + 3 = 13 roundings, so of up to 3 x 13 x 2^-53 = 5e-15 of sum (W d)^2: 1e-7 max(F_t, K) / sqrt(n) (the route's shift is the
    intrinsic value at the forward, not this path's price)"""
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    p = hawkes_params()
    for k in ("lambda_p", "lambda_m", "theta_p", "theta_m", "beta1_p", "beta2_p", "beta1_m", "beta2_m"):
        p[k] = 0.0
    n, spy, forward = 1000, 480, 1.02
    chain = dict(ttms=TTMS, forwards=np.full(3, forward), discfactors=np.ones(3), strikes_ttms=[QUOTE_K] * 3, optiontypes_ttms=[QUOTE_T] * 3)
    pr, sd, fwds, rows = check_route_is_cond_plus_c_tail(p, chain, n, 3, spy, GAMMAS, False)
    for i in range(3):
        mu, cv = rows[i], rows[3 + i]
        assert np.all(mu == mu[0]) and np.all(cv == cv[0]) and cv[0] > 0.0
        for g, gamma in enumerate(GAMMAS):
            ft = forward * np.exp(mu[0] + (gamma + 0.5) * cv[0])
            for j, (k, t) in enumerate(zip(QUOTE_K, QUOTE_T)):
                want = float(tc.path_terms(mu[:1], cv[:1], forward, k, t == "P", gamma)[2][0])
                err = abs(pr[g][i][j] - want) / max(ft, k)
                assert err <= 64 * EPS, (i, gamma, k, err)
            assert np.all(sd[g][i] <= 1e-7 * max(ft, QUOTE_K.max()) / np.sqrt(n)) and fwds[g][2][i, 5] == n
            assert abs(fwds[g][2][i, 2] - ft) <= 64 * EPS * ft and fwds[g][2][i, 4] == pytest.approx(n, rel=1e-13)


def test_every_refusal_returns_its_status_code_and_launches_nothing():
    from stochvolmodels_amd import _lib
    p, n, m = hawkes_params(), 257, 3
    eng, _ = cond_rows(p, TTMS, n, 5, 480)
    try:
        ks, ts, fw = [QUOTE_K] * 3, [QUOTE_T] * 3, np.full(3, 1.02)
        rc, good, _, _ = c_tail(eng, m, fw, ks, ts, [0.5], False)
        assert rc == _lib.OK and np.all(np.isfinite(good))
        K = 3 * QUOTE_K.size
        nan_k, inf_s, bad_c = np.concatenate(ks), np.zeros(K), np.concatenate([codes_of(t) for t in ts])
        nan_k[4], inf_s[7], bad_c[2] = np.nan, np.inf, 2
        cases = [(dict(n_path=0), _lib.ERR_INVALID_ARGUMENT), (dict(n_expiries=0), _lib.ERR_INVALID_ARGUMENT),
                 (dict(n_gammas=0), _lib.ERR_INVALID_ARGUMENT), (dict(gammas=np.zeros(17), n_gammas=17), _lib.ERR_INVALID_ARGUMENT),
                 (dict(gammas=np.array([np.nan])), _lib.ERR_INVALID_ARGUMENT), (dict(forwards=np.array([1.0, np.inf, 1.0])), _lib.ERR_INVALID_ARGUMENT),
                 (dict(forwards=np.array([1.0, 0.0, 1.0])), _lib.ERR_INVALID_ARGUMENT), (dict(forwards=np.array([1.0, -1.0, 1.0])), _lib.ERR_INVALID_ARGUMENT),
                 (dict(strikes=nan_k), _lib.ERR_INVALID_ARGUMENT), (dict(shifts=inf_s), _lib.ERR_INVALID_ARGUMENT),
                 (dict(mu_null=True), _lib.ERR_INVALID_ARGUMENT), (dict(codes=bad_c.astype(np.int8)), _lib.ERR_UNKNOWN_PAYOFF),
                 (dict(ws_bytes=1024), _lib.ERR_WORKSPACE)]
        for bad, status in cases:
            rc, prices, stderrs, stats = c_tail(eng, m, fw, ks, ts, [0.5], False, bad)
            assert rc == status, (bad, rc)
            assert np.all(prices == -7.0) and np.all(stderrs == -7.0) and np.all(stats == -7.0), bad      # nothing came back
        rc, again, _, _ = c_tail(eng, m, fw, ks, ts, [0.5], False)
        assert rc == _lib.OK and np.array_equal(again, good)
    finally:
        eng.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def tilted_cond_z_scores(nb_steps_per_year, nb_path=1 << 20, seed=2025):
    """the paper's slice of test_gpu_tilted.tilted_z_scores under gamma = -1 and +1 in one call: z-scores of the 20 options and of
    (normalizer, gamma forward) per gamma against the Fourier pricer under the kernel, and against the plain Monte Carlo under it at
    equal settings (independent streams, the same discretisation)"""
    import dataclasses
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    p = hp.HawkesJDParams()
    k = np.linspace(0.5, 1.5, 20)
    chain = dict(ttms=np.array([1.0 / 12.0]), forwards=np.array([1.0]), discfactors=np.array([1.0]), strikes_ttms=[k],
                 optiontypes_ttms=[np.where(k <= 1.0, "P", "C")])
    gammas = [-1.0, 1.0]
    kw = p.to_dict()
    kw.pop("risk_premia_gamma")
    common = dict(risk_premia_gammas=gammas, nb_path=nb_path, seed=seed, nb_steps_per_year=nb_steps_per_year, return_forwards=True, **chain, **kw)
    pr, sd, fwds = hp.hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas(**common)
    qr, qd, qwds = hp.hawkesjd_mc_chain_pricer_with_risk_premia_gammas(**common)
    out = {}
    for g, gamma in enumerate(gammas):
        ref, (norm, gfwd) = hp.hawkesjd_chain_pricer_with_risk_premia(model_params=dataclasses.replace(p, risk_premia_gamma=gamma),
                                                                      return_forwards=True, **chain)
        st, qt = fwds[g][2][0], qwds[g][2][0]
        out[f"gamma={gamma:+.0f}"] = dict(
            options=((pr[g][0] - ref[0]) / sd[g][0]).tolist(), normalizer=float((st[0] - norm[0]) / st[1]),
            gamma_forward=float((st[2] - gfwd[0]) / st[3]), effective_sample_size=float(st[4]),
            options_vs_plain=((pr[g][0] - qr[g][0]) / np.hypot(sd[g][0], qd[g][0])).tolist(),
            normalizer_vs_plain=float((st[0] - qt[0]) / np.hypot(st[1], qt[1])),
            gamma_forward_vs_plain=float((st[2] - qt[2]) / np.hypot(st[3], qt[3])), plain_effective_sample_size=float(qt[4]),
            error_squared_ratio=((qd[g][0] / sd[g][0]) ** 2).tolist())
    return out


def test_mc_agrees_with_fourier_and_with_the_plain_estimator_under_the_kernel():
    """independent of any stream: 2^20 paths at 28 800 steps per year (test_gpu_tilted's settings); every option within 4 of its
    standard errors of hawkesjd_chain_pricer_with_risk_premia, the normalizer and the gamma forward within 4 of theirs of
    hawkesjd_forwards_under_risk_kernel; and every figure within 4 combined errors of the plain Monte Carlo under the kernel.  The 4
    is the reference's own criterion; a miss is to be examined at twice the steps (a step bias halves, a defect stays), never
    answered by a wider bound.  SVMC_TILTED_COND_Z_SCORES=<file> keeps the z-scores (profiles/hawkes_tilted_cond_z_scores.json)."""
    z = tilted_cond_z_scores(28800)
    print("conditional tilted z-scores at 28800 steps/yr, 2^20 paths:", json.dumps(z))
    if os.environ.get("SVMC_TILTED_COND_Z_SCORES"):
        with open(os.environ["SVMC_TILTED_COND_Z_SCORES"], "w") as fh:
            json.dump(z, fh, indent=1)
    allz = np.concatenate([np.array(v["options"] + [v["normalizer"], v["gamma_forward"]]) for v in z.values()])
    assert allz.size == 44 and np.all(np.abs(allz) <= 4.0), allz
    both = np.concatenate([np.array(v["options_vs_plain"] + [v["normalizer_vs_plain"], v["gamma_forward_vs_plain"]]) for v in z.values()])
    assert both.size == 44 and np.all(np.abs(both) <= 4.0), both
