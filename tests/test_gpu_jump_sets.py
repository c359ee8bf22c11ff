"""
Many (sigma, gamma) sets on one set of jump rows on the GPU (include/svmc_est.h svmc_jump_sets_payoff_chain;
csrc/svmc_est.hip's jump_sets_*_kernel in libsvmc_est.so):

  1. the arithmetic against the long-double twin of tests/jump_sets_twin.py on uploaded rows;
  2. HawkesJumpRows.price_sets against the existing route at the same seed: the same jumps, so the two differ by the rounding of mu;
  3. the exact identities: corr is svmc_cmc_payoff_chain's on (a, 0), the rows are svmc_hawkesjd_chain_cond's at sigma = 0, and no
     bit depends on a call's company (sets, the 16-set chunking, expiries, strikes);
  4. the degenerate and keep cases;
  5. the handle survives other work on its engine;
  6. every refusal of the C entry; 17 expiries;
  7. the calibration with estimator="conditional";
  8. the statistics against the Fourier pricer under the kernel, independent of any stream.

Deviations: |device - twin| / max(|twin|, 1e-4 scale), the measure of tests/test_gpu_tilted_cond.py with its scales (the forward for
prices, gamma forwards and their errors; 1 for the normalizer and its error; none for the effective sample size).  Every comparison
prints its deviation and the module ends by printing the largest of each quantity (run with -s).  The bounds in TOL follow that
module's rule: ten times the largest deviation seen on the MI355X against the twin, rounded up to one digit, as
profiles/hawkes_jump_sets_observed_tolerances.txt records them, none above the project's parity bound 1e-12.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cmc_twin as ct
import jump_sets_twin as js
import tilted_cond_twin as tc

pytestmark = pytest.mark.gpu

L_ = np.longdouble
EPS = 2.0 ** -52
GAMMAS = [-3.0, -1.0, 0.0, 0.5, 3.0]
VARIANCES = [0.0, 1e-4, 0.04]
FIELDS = ("price", "stderr", "normalizer", "normalizer_stderr", "gamma_forward", "gamma_forward_stderr", "effective_sample_size")
# ten times the largest deviation observed on the MI355X, rounded up to one digit (profiles/hawkes_jump_sets_observed_tolerances.txt)
TOL = dict(price=7e-13, stderr=3e-13, normalizer=3e-15, normalizer_stderr=8e-15, gamma_forward=5e-14, gamma_forward_stderr=8e-15,
           effective_sample_size=5e-15)
assert max(TOL.values()) <= 1e-12      # the project's parity bound for prices and states: no bound here may exceed it
PARITY_BOUND = 1e-12
ROUTE_BOUND = 1e-10                    # item 2: rows that differ by about 1e-13 move a price by F_t |delta| times that (module doc)
SEEN = {}
TTMS = np.array([1.0 / 52.0, 1.0 / 12.0, 0.25])
QUOTE_K, QUOTE_T = np.array([0.85, 0.95, 1.0, 1.02, 1.1, 1.25]), np.array(["P", "P", "P", "C", "C", "C"])
# item 7: the calibration of tests/test_jump_sets_host.py, and ten times the |x_fit - x*| its CPU twin run recorded
CAL_RECOVERY = (10 * 2.055e-02, 10 * 1.157e+00)


@pytest.fixture(scope="module", autouse=True)
def largest_deviations():
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


def codes_of(types):
    return np.array([0 if t == "C" else 1 for t in np.ravel(types)], dtype=np.int8)


def slice_of(n_strikes, forward):
    """n_strikes strikes around the forward, puts at or below it, calls above"""
    k = forward * (np.linspace(0.6, 1.5, n_strikes) if n_strikes > 1 else np.array([1.05]))
    return k, np.where(k <= forward, "P", "C")


def sample(n, seed, vol=0.2):
    rng = np.random.default_rng(seed)
    return vol * rng.standard_normal(n) - 0.5 * vol * vol


def hawkes_params(name="hawkes_mc"):
    import hawkes_twin as ht
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    return dict(zip(ht.PARAM_NAMES, (float(v) for v in g["params"])))


def model_kw(p):
    return {k: v for k, v in p.items() if k != "sigma"}


def run_on_uploaded(rows_a, forwards, strikes, types, variances, gammas, recenter, rows=None, shifts=None):
    """the tail on rows uploaded from the host: expiry i's a in snapshot row i (or the expiries given)"""
    from stochvolmodels_amd.engine import get_engine
    n, m = rows_a[0].size, len(rows_a)
    eng = get_engine(n)
    eng.reserve_snapshots(2 * m)
    for i, a in enumerate(rows_a):
        eng.upload(eng.snapshot_ptr(i), a)
        eng.upload(eng.snapshot_ptr(m + i), np.zeros(n))
    rows = list(range(m)) if rows is None else rows
    var = np.asarray(variances, dtype=np.float64)[:, rows]
    return eng.jump_sets_payoffs([forwards[i] for i in rows], [strikes[i] for i in rows], [codes_of(types[i]) for i in rows], var, gammas,
                                 recenter, a_rows=rows, shifts=shifts)


def check_against_twin(out, rows_a, forwards, strikes, types, variances, gammas, recenter, what):
    prices, stderrs, stats, corr = out
    from stochvolmodels_amd.engine import TILTED_COND_STATS_FIELDS as SF
    for i, a in enumerate(rows_a):
        want_corr = float(js.corr_of(a, forwards[i], recenter))
        assert abs(corr[i] - want_corr) <= 1e-12 * forwards[i] or (np.isnan(corr[i]) and np.isnan(want_corr)), (what, i, corr[i], want_corr)
    for q, gamma in enumerate(gammas):
        for i, a in enumerate(rows_a):
            v = variances[q][i]
            p, e, st = js.estimator(a, v, forwards[i], strikes[i], types[i], gamma, recenter)
            row = dict(zip(SF, stats[q, i]))
            assert (row["n_kept"], row["n_dropped"]) == (st["n_kept"], st["n_dropped"]), (what, gamma, v, i)
            tag = f"{what} gamma={gamma} v={v} expiry={i} n={a.size} K={len(strikes[i])} recenter={recenter}"
            note("price", deviation(prices[q][i], p, forwards[i]), tag)
            note("stderr", deviation(stderrs[q][i], e, forwards[i]), tag)
            for k in FIELDS[2:]:
                scale = forwards[i] if k.startswith("gamma_forward") else (1.0 if k.startswith("normalizer") else 0.0)
                note(k, deviation([row[k]], [st[k]], scale), tag)
            assert deviation([row["sum_weights"]], [st["sum_weights"]], 0.0) <= PARITY_BOUND


def sets_of(n_sets, m):
    """(gammas [Q], variances [Q][m]): the gammas and the variances cycle through GAMMAS and VARIANCES at different periods; expiry i's
    variance is (i + 1) times the first's"""
    g = [GAMMAS[q % len(GAMMAS)] for q in range(n_sets)]
    v = [[VARIANCES[(q + 1) % len(VARIANCES)] * (i + 1) for i in range(m)] for q in range(n_sets)]
    return g, v


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4099])
@pytest.mark.parametrize("recenter", [False, True])
def test_arithmetic_against_the_twin_over_path_counts(n, recenter):
    a = sample(n, 100 + n)
    k, t = slice_of(9, 1.3)
    g, v = sets_of(3, 1)
    out = run_on_uploaded([a], [1.3], [k], [t], v, g, recenter)
    check_against_twin(out, [a], [1.3], [k], [t], v, g, recenter, "paths")


@pytest.mark.parametrize("n_sets", [1, 3, 16])
@pytest.mark.parametrize("recenter", [False, True])
def test_arithmetic_over_sets_strike_counts_and_expiries(n_sets, recenter):
    n = 257
    forwards = [1.0, 1.05, 1.7]
    rows_a = [sample(n, 7 + i, 0.1 + 0.05 * i) for i in range(3)]
    ks, ts = zip(*[slice_of(c, f) for c, f in zip((1, 9, 22), forwards)])
    g, v = sets_of(n_sets, 3)
    out = run_on_uploaded(rows_a, forwards, list(ks), list(ts), v, g, recenter)
    check_against_twin(out, rows_a, forwards, list(ks), list(ts), v, g, recenter, f"{n_sets} sets, three expiries")
    # one expiry of eight strikes: exactly one full strike group
    k8, t8 = slice_of(8, 1.05)
    v1 = [row[:1] for row in v]
    out = run_on_uploaded(rows_a[1:2], [1.05], [k8], [t8], v1, g, recenter)
    check_against_twin(out, rows_a[1:2], [1.05], [k8], [t8], v1, g, recenter, f"{n_sets} sets, eight strikes")


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [700, 65537])
def test_price_sets_against_the_existing_route_at_one_seed(n):
    """streams 9 and 10 of (seed, call id) give both routes the same jumps; the existing route's mu carries -sigma^2 dt / 2 step by
    step, this one's a - v / 2 in one subtraction: tests/test_jump_sets_host.py item 1 bounds the rows' difference by (steps + 2) eps
    max |mu|, about 1e-13 under 1 000 steps.  A price moves by at most F_t |delta| times that, plus |gamma| times that relatively
    through the weight: 1e-10 F is three orders above it, and a wrong sign or a missing v / 2 shows at 1e-4 or more."""
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.engine import TILTED_COND_STATS_FIELDS as SF
    p, seed, spy, forward = hawkes_params(), 21, 480, 1.02
    chain = dict(ttms=TTMS, forwards=np.full(3, forward), discfactors=np.array([0.999, 0.995, 0.99]), strikes_ttms=[QUOTE_K] * 3,
                 optiontypes_ttms=[QUOTE_T] * 3)
    worst = 0.0
    for recenter in (False, True):
        for sigma in (p["sigma"], 0.2):
            ref = sv.hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas(
                risk_premia_gammas=GAMMAS, nb_path=n, seed=seed, nb_steps_per_year=spy, recenter_forward=recenter, return_forwards=True,
                **chain, **dict(p, sigma=sigma))
            got = sv.hawkesjd_mc_chain_pricer_conditional_sets([sigma] * len(GAMMAS), GAMMAS, nb_path=n, seed=seed, nb_steps_per_year=spy,
                                                               recenter_forward=recenter, return_forwards=True, **chain, **model_kw(p))
            for g in range(len(GAMMAS)):
                for i in range(3):
                    dp = float(np.max(np.abs(got[0][g][i] - ref[0][g][i]))) / forward
                    de = float(np.max(np.abs(got[1][g][i] - ref[1][g][i]))) / forward
                    a, b = dict(zip(SF, got[2][g][2][i])), dict(zip(SF, ref[2][g][2][i]))
                    assert (a["n_kept"], a["n_dropped"]) == (b["n_kept"], b["n_dropped"]) == (n, 0)
                    ds = [abs(a[k] - b[k]) / s for k, s in (("normalizer", 1.0), ("normalizer_stderr", 1.0), ("gamma_forward", forward),
                                                            ("gamma_forward_stderr", forward), ("effective_sample_size", b["effective_sample_size"]),
                                                            ("sum_weights", b["sum_weights"]))]
                    worst = max([worst, dp, de] + ds)
                    assert max([dp, de] + ds) <= ROUTE_BOUND, (recenter, sigma, GAMMAS[g], i, dp, de, ds)
    print(f"n={n}: largest difference to the existing route (in F, or relative): {worst:.3e}  bound {ROUTE_BOUND:.0e}")


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def cond_rows(p, ttms, n, seed, spy):
    """svmc_hawkesjd_chain_cond from the origin on an engine of its own: mu in rows [0, m), cv in [m, 2m) -> (engine, host cvs)"""
    from stochvolmodels_amd.engine import HipEngine
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    grids = ct.chain_grids(ttms, spy)
    eng = HipEngine(n)
    eng.set_state(np.zeros(n), np.full(n, p["lambda_p"]), np.full(n, p["lambda_m"]))
    cvs = eng.hawkesjd_chain_cond([g[0] for g in grids], [g[1] for g in grids], hp.params_block(**p), seed, 0)
    return eng, cvs


def three_expiries(n=257):
    forwards = [1.0, 1.05, 1.7]
    rows_a = [sample(n, 7 + i, 0.1 + 0.05 * i) for i in range(3)]
    for a in rows_a[:2]:
        a[[5, 100]] = [np.nan, np.inf]                           # f11's rule drops them from corr as well
    ks, ts = zip(*[slice_of(c, f) for c, f in zip((22, 9, 1), forwards)])
    return rows_a, forwards, list(ks), list(ts)


def test_corr_is_the_conditional_estimators_on_the_rows_a_zero():
    from stochvolmodels_amd.engine import get_engine
    rows_a, fw, ks, ts = three_expiries()
    for n_sets in (1, 16):
        g, v = sets_of(n_sets, 3)
        for recenter in (False, True):
            _, _, _, corr = run_on_uploaded(rows_a, fw, ks, ts, v, g, recenter)
            eng = get_engine(rows_a[0].size)                     # (rows [3, 6) hold zeros)
            _, _, cst = eng.conditional_payoffs(fw, np.ones(3), ks, [codes_of(t) for t in ts], recenter, mu_rows=[0, 1, 2], cv_rows=[3, 4, 5])
            for i in range(3):
                assert corr[i] == cst[i]["corr"], (n_sets, recenter, i, corr[i], cst[i]["corr"])    # bit for bit, whatever the sets
            assert (corr != 0.0).all() == recenter


def test_the_jump_rows_are_the_conditional_steppings_at_sigma_zero():
    import stochvolmodels_amd as sv
    p, n, seed, spy = hawkes_params(), 700, 21, 480
    rows = sv.hawkesjd_jump_rows(TTMS, nb_path=n, seed=seed, nb_steps_per_year=spy, sigma=0.3, risk_premia_gamma=2.0, **model_kw(p))
    eng, cvs = cond_rows(dict(p, sigma=0.0), TTMS, n, seed, spy)
    try:
        want = eng.download(eng.snapshot_ptr(0), 6 * n).reshape(6, n)
    finally:
        eng.close()
    assert np.array_equal(rows.numpy(), want[:3]) and np.all(want[3:] == 0.0) and np.all(cvs == 0.0)
    # ... and its variances are that entry's cv row at the sigma asked for
    eng, cvs = cond_rows(p, TTMS, n, seed, spy)
    eng.close()
    assert np.array_equal(rows.variances(p["sigma"]), cvs)
    rows.free()


def test_company_does_not_change_bits():
    import stochvolmodels_amd as sv
    rows_a, fw, ks, ts = three_expiries()
    g16, v16 = sets_of(16, 3)
    for recenter in (False, True):
        all_p, all_e, all_s, all_c = run_on_uploaded(rows_a, fw, ks, ts, v16, g16, recenter)
        # a set alone, first of three, last of sixteen
        for q, company in ((0, [0]), (15, [15]), (15, [15, 3, 7]), (7, [2, 9, 7])):
            p, e, s, c = run_on_uploaded(rows_a, fw, ks, ts, [v16[j] for j in company], [g16[j] for j in company], recenter)
            at = company.index(q)
            assert np.array_equal(s[at], all_s[q], equal_nan=True) and np.array_equal(c, all_c)
            for i in range(3):
                assert np.array_equal(p[at][i], all_p[q][i]) and np.array_equal(e[at][i], all_e[q][i])
        for i in (0, 1, 2):                                      # the expiry alone
            p, e, s, c = run_on_uploaded(rows_a, fw, ks, ts, v16, g16, recenter, rows=[i])
            assert c[0] == all_c[i]
            for q in range(16):
                assert np.array_equal(p[q][0], all_p[q][i]) and np.array_equal(e[q][0], all_e[q][i]) and np.array_equal(s[q, 0], all_s[q, i])
        for i, j in ((0, 0), (0, 17), (0, 8), (1, 8)):           # the strike alone, one set
            one_k, one_t = list(ks), list(ts)
            one_k[i], one_t[i] = ks[i][j:j + 1], ts[i][j:j + 1]
            p, e, s, c = run_on_uploaded(rows_a, fw, one_k, one_t, v16[3:4], g16[3:4], recenter, rows=[i])
            assert p[0][0][0] == all_p[3][i][j] and e[0][0][0] == all_e[3][i][j] and np.array_equal(s[0, 0], all_s[3, i])
    # the 16-set chunking of the Python route: 17 sets, each the same bits as alone
    pp, n, seed, spy = hawkes_params(), 700, 4, 480
    rows = sv.hawkesjd_jump_rows(TTMS, nb_path=n, seed=seed, nb_steps_per_year=spy, **model_kw(pp))
    sigmas, gammas = np.linspace(0.05, 0.85, 17), np.linspace(-3.0, 3.0, 17)
    chain = (np.full(3, 1.02), [QUOTE_K] * 3, [QUOTE_T] * 3)
    many = rows.price_sets(sigmas, gammas, *chain, recenter_forward=True, return_forwards=True)
    assert len(many[0]) == 17
    for q in (0, 15, 16):
        one = rows.price_sets([sigmas[q]], [gammas[q]], *chain, recenter_forward=True, return_forwards=True)
        for i in range(3):
            assert np.array_equal(one[0][0][i], many[0][q][i]) and np.array_equal(one[1][0][i], many[1][q][i])
        assert np.array_equal(one[2][0][2], many[2][q][2])
    rows.free()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def test_zero_variance_is_the_plain_estimator_under_the_kernel_on_a():
    from stochvolmodels_amd.engine import get_engine
    rows_a, fw, ks, ts = three_expiries()
    rows_a = [sample(257, 40 + i, 0.15) for i in range(3)]
    zeros = [[0.0] * 3 for _ in GAMMAS]
    for recenter in (False, True):
        p, e, s, _ = run_on_uploaded(rows_a, fw, ks, ts, zeros, GAMMAS, recenter)
        tp, te, tst = get_engine(257).tilted_payoffs(fw, ks, [codes_of(t) for t in ts], GAMMAS, recenter, snap_rows=[0, 1, 2])
        for g in range(len(GAMMAS)):
            for i in range(3):
                dp, de = deviation(p[g][i], tp[g][i], fw[i]), deviation(e[g][i], te[g][i], fw[i])
                ds = [deviation([s[g, i, c]], [tst[g, i, c]], sc) for c, sc in enumerate((1.0, 1.0, fw[i], fw[i], 0.0))]
                print(f"v = 0 against tilted_payoffs recenter={recenter} gamma={GAMMAS[g]} expiry={i}: prices {dp:.3e}, stderrs {de:.3e}, "
                      f"stats {max(ds):.3e}")
                assert max([dp, de] + ds) <= PARITY_BOUND
                assert np.array_equal(s[g, i, 5:7], tst[g, i, 5:7]) and deviation([s[g, i, 7]], [tst[g, i, 7]], 0.0) <= PARITY_BOUND


def test_a_weight_that_overflows_only_at_gamma_three():
    """a = 120: exp(a) is finite and f11's rule keeps the path; W^2 overflows at gamma = 3 alone, so that set counts one dropped path and
    the others none.  Where the path is kept it dominates every sum (tests/test_gpu_tilted_cond.py's note): the prices and the ratios
    are held to the twin everywhere, the errors where the path is dropped (gamma = 3) or weightless (gamma = -3)."""
    from stochvolmodels_amd.engine import TILTED_COND_STATS_FIELDS as SF
    a = sample(300, 5)
    a[200] = 120.0
    k, t = slice_of(5, 1.0)
    v = [[0.01]] * len(GAMMAS)
    prices, stderrs, stats, _ = run_on_uploaded([a], [1.0], [k], [t], v, GAMMAS, False)
    assert stats[:, 0, SF.index("n_kept")].tolist() == [300.0, 300.0, 300.0, 300.0, 299.0]
    assert stats[:, 0, SF.index("n_dropped")].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0]
    for g, gamma in enumerate(GAMMAS):
        p, e, st = js.estimator(a, 0.01, 1.0, k, t, gamma, False)
        row = dict(zip(SF, stats[g, 0]))
        assert (row["n_kept"], row["n_dropped"]) == (st["n_kept"], st["n_dropped"])
        tag = f"overflowing weight gamma={gamma}"
        note("price", deviation(prices[g][0], p, 1.0), tag)
        note("normalizer", deviation([row["normalizer"]], [st["normalizer"]], 1.0), tag)
        note("effective_sample_size", deviation([row["effective_sample_size"]], [st["effective_sample_size"]], 0.0), tag)
        note("gamma_forward", deviation([row["gamma_forward"]], [st["gamma_forward"]], 1.0 if gamma in (3.0, -3.0) else 0.0), tag)
        if gamma == 3.0:
            note("stderr", deviation(stderrs[g][0], e, 1.0), tag)
            for f, sc in (("normalizer_stderr", 1.0), ("gamma_forward_stderr", 1.0)):
                note(f, deviation([row[f]], [st[f]], sc), tag)


def test_every_path_dropped_gives_nan_prices_and_says_so():
    from stochvolmodels_amd.engine import TILTED_COND_STATS_FIELDS as SF
    a = np.full(70, np.nan)
    k, t = slice_of(9, 1.0)
    g, v = sets_of(5, 1)
    for recenter in (False, True):
        p, e, s, corr = run_on_uploaded([a], [1.0], [k], [t], v, g, recenter)
        assert np.isnan(corr[0]) if recenter else corr[0] == 0.0
        for q in range(5):
            assert np.all(np.isnan(p[q][0])) and np.all(np.isnan(e[q][0]))
            assert s[q, 0, SF.index("n_kept")] == 0.0 and s[q, 0, SF.index("n_dropped")] == 70.0 and s[q, 0, SF.index("sum_weights")] == 0.0


def test_non_positive_recentred_strikes_and_put_call_parity():
    from stochvolmodels_amd.engine import TILTED_COND_STATS_FIELDS as SF
    a = sample(513, 9)
    forward = 1.7
    k = forward * np.array([-0.3, -0.3, -0.05, -0.05, 0.0, 0.0, 0.9, 0.9, 1.2, 1.2])
    t = np.array(["C", "P"] * 5)
    g, v = sets_of(5, 1)
    for recenter in (False, True):
        out = run_on_uploaded([a], [forward], [k], [t], v, g, recenter)
        check_against_twin(out, [a], [forward], [k], [t], v, g, recenter, "K' <= 0")
        p, _, s, corr = out
        assert (corr[0] != 0.0) == recenter and np.sum(k + corr[0] <= 0.0) == (6 if corr[0] <= 0.0 else 4), corr
        for q, gamma in enumerate(g):
            parity = p[q][0][0::2] - p[q][0][1::2] - (s[q, 0, SF.index("gamma_forward")] - k[0::2])
            print(f"put-call parity gamma={gamma} v={v[q][0]} recenter={recenter}: {np.max(np.abs(parity)) / forward:.3e} F")
            assert np.max(np.abs(parity)) <= 1e-12 * forward
            assert np.all(p[q][0][1::2][k[1::2] + corr[0] <= 0.0] == 0.0)       # a put at K' <= 0 pays nothing


def test_host_array_route():
    import stochvolmodels_amd as sv
    a = sample(1000, 3)
    k, t = slice_of(6, 1.1)
    k2, t2 = k.reshape(2, 3), t.reshape(2, 3)
    p, e, st = sv.compute_mc_vars_payoff_jump_sets(a, [0.04, 0.0, 1e-4], [-1.0, 0.5, 3.0], 1.1, k2, t2, recenter=True, return_stats=True)
    for q, (v, g) in enumerate(((0.04, -1.0), (0.0, 0.5), (1e-4, 3.0))):
        assert p[q].shape == e[q].shape == (2, 3) and st[q]["n_kept"] == 1000
        bp, be, bst = js.estimator(a, v, 1.1, k, t, g, True)
        note("price", deviation(p[q].ravel(), bp, 1.1), "host route")
        note("stderr", deviation(e[q].ravel(), be, 1.1), "host route")
        note("gamma_forward", deviation([st[q]["gamma_forward"]], [bst["gamma_forward"]], 1.1), "host route")


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def test_the_handle_survives_other_work_on_its_engine():
    import stochvolmodels_amd as sv
    p, n, seed, spy = hawkes_params(), 4099, 12, 480
    chain = dict(ttms=TTMS, forwards=np.full(3, 1.02), discfactors=np.array([0.999, 0.995, 0.99]), strikes_ttms=[QUOTE_K] * 3,
                 optiontypes_ttms=[QUOTE_T] * 3)
    rows = sv.hawkesjd_jump_rows(TTMS, nb_path=n, seed=seed, nb_steps_per_year=spy, **model_kw(p))
    args = ([0.45, 0.2], [-1.0, 2.0], chain["forwards"], chain["strikes_ttms"], chain["optiontypes_ttms"])
    first = rows.price_sets(*args, recenter_forward=True, return_forwards=True)
    kept = rows.numpy().copy()
    sv.hawkesjd_mc_chain_pricer_conditional(nb_path=n, seed=seed + 1, nb_steps_per_year=spy, **chain, **p)
    lp = sv.LOGSV_BTC_PARAMS
    sv.logsv_mc_chain_pricer(v0=lp.sigma0, theta=lp.theta, kappa1=lp.kappa1, kappa2=lp.kappa2, beta=lp.beta, volvol=lp.volvol,
                             vol_backbone_etas=lp.get_vol_backbone_etas(ttms=TTMS), nb_path=n, seed=3, **chain)
    assert np.array_equal(rows.numpy(), kept)
    second = rows.price_sets(*args, recenter_forward=True, return_forwards=True)
    for q in range(2):
        for i in range(3):
            assert np.array_equal(first[0][q][i], second[0][q][i]) and np.array_equal(first[1][q][i], second[1][q][i])
        assert np.array_equal(first[2][q][2], second[2][q][2])
    rows.free()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def c_tail(eng, m, forwards, strikes, types, variances, gammas, recenter, bad=None):
    """svmc_jump_sets_payoff_chain itself on snapshot rows [0, m) of the engine -> (status, prices, stderrs, stats, corr)"""
    from stochvolmodels_amd import _lib
    from stochvolmodels_amd.engine import payoff_shifts
    E = _lib.load_est()
    dp = C.POINTER(C.c_double)
    k_all = np.ascontiguousarray(np.concatenate([np.ravel(k) for k in strikes]), dtype=np.float64)
    c_all = np.ascontiguousarray(np.concatenate([codes_of(t) for t in types]))
    sh = np.ascontiguousarray(np.concatenate([payoff_shifts(np.ravel(k), codes_of(t), float(f), 1) for k, t, f in zip(strikes, types, forwards)]))
    offs = np.concatenate([[0], np.cumsum([np.size(k) for k in strikes])]).astype(np.uintp)
    fw, gm = np.ascontiguousarray(forwards, dtype=np.float64), np.ascontiguousarray(gammas, dtype=np.float64)
    var = np.ascontiguousarray(variances, dtype=np.float64)
    a = dict(strikes=k_all, codes=c_all, shifts=sh, forwards=fw, gammas=gm, variances=var, n_sets=gm.size, n_expiries=m, n_path=eng.n_path,
             a_null=False, ws_bytes=None, offs=offs)
    a.update(bad or {})
    Q, K = gm.size, k_all.size                                # (of the well-formed call: the outputs are sized by it)
    nbytes = C.c_size_t(0)
    assert E.svmc_jump_sets_workspace_bytes(eng.n_path, m, K, Q, C.byref(nbytes)) == _lib.OK
    ws_ptr, _ = eng.alloc_sums((nbytes.value + 7) // 8, "jump_sets_workspace")
    prices, stderrs, stats, corr = np.full(Q * K, -7.0), np.full(Q * K, -7.0), np.full(Q * m * 8, -7.0), np.full(m, -7.0)
    rows = (C.c_void_p * m)(*[None if a["a_null"] and i == m - 1 else eng.snapshot_ptr(i) for i in range(m)])
    rc = E.svmc_jump_sets_payoff_chain(rows, a["n_path"], a["forwards"].ctypes.data_as(dp), a["n_expiries"], a["strikes"].ctypes.data_as(dp),
                                       a["codes"].ctypes.data_as(C.POINTER(C.c_int8)), a["shifts"].ctypes.data_as(dp),
                                       a["offs"].ctypes.data_as(C.POINTER(C.c_size_t)), a["variances"].ctypes.data_as(dp),
                                       a["gammas"].ctypes.data_as(dp), a["n_sets"], int(recenter), prices.ctypes.data_as(dp),
                                       stderrs.ctypes.data_as(dp), stats.ctypes.data_as(dp), corr.ctypes.data_as(dp), ws_ptr,
                                       nbytes.value if a["ws_bytes"] is None else a["ws_bytes"], eng.stream)
    return rc, prices, stderrs, stats.reshape(Q, m, 8), corr


def test_every_refusal_returns_its_status_code_and_launches_nothing():
    from stochvolmodels_amd import _lib
    p, n, m = hawkes_params(), 257, 3
    eng, _ = cond_rows(dict(p, sigma=0.0), TTMS, n, 5, 480)
    try:
        ks, ts, fw = [QUOTE_K] * 3, [QUOTE_T] * 3, np.full(3, 1.02)
        var = np.array([[0.004, 0.017, 0.05], [0.0, 0.0, 0.0]])
        gm = [0.5, -2.0]
        rc, good, _, gstats, gcorr = c_tail(eng, m, fw, ks, ts, var, gm, True)
        assert rc == _lib.OK and np.all(np.isfinite(good)) and np.all(gstats[:, :, 5] == n) and np.all(gcorr != -7.0)
        K = 3 * QUOTE_K.size
        nan_k, inf_s, bad_c = np.concatenate(ks), np.zeros(K), np.concatenate([codes_of(t) for t in ts])
        nan_k[4], inf_s[7], bad_c[2] = np.nan, np.inf, 2
        neg_v, nan_v, inf_v = var.copy(), var.copy(), var.copy()
        neg_v[1, 2], nan_v[0, 0], inf_v[1, 1] = -1e-12, np.nan, np.inf
        bad_offs0, bad_offs1 = np.array([1, 6, 12, 18], dtype=np.uintp), np.array([0, 12, 6, 18], dtype=np.uintp)
        INV = _lib.ERR_INVALID_ARGUMENT
        cases = [(dict(n_path=0), INV), (dict(n_expiries=0), INV), (dict(n_sets=0), INV), (dict(n_sets=-1), INV),
                 (dict(gammas=np.zeros(17), variances=np.zeros((17, 3)), n_sets=17), INV),
                 (dict(gammas=np.array([np.nan, 0.0])), INV), (dict(gammas=np.array([0.0, np.inf])), INV),
                 (dict(variances=neg_v), INV), (dict(variances=nan_v), INV), (dict(variances=inf_v), INV),
                 (dict(forwards=np.array([1.0, np.inf, 1.0])), INV), (dict(forwards=np.array([1.0, 0.0, 1.0])), INV),
                 (dict(forwards=np.array([1.0, -1.0, 1.0])), INV), (dict(strikes=nan_k), INV), (dict(shifts=inf_s), INV),
                 (dict(offs=bad_offs0), INV), (dict(offs=bad_offs1), INV), (dict(a_null=True), INV),
                 (dict(codes=bad_c.astype(np.int8)), _lib.ERR_UNKNOWN_PAYOFF), (dict(ws_bytes=1024), _lib.ERR_WORKSPACE)]
        for bad, status in cases:
            rc, prices, stderrs, stats, corr = c_tail(eng, m, fw, ks, ts, var, gm, True, bad)
            assert rc == status, (bad, rc)
            assert np.all(prices == -7.0) and np.all(stderrs == -7.0) and np.all(stats == -7.0) and np.all(corr == -7.0), bad
        E = _lib.load_est()
        nb = C.c_size_t(0)
        for args in ((0, 3, 18, 2), (n, 0, 18, 2), (n, 3, 18, 0), (n, 3, 18, 17)):
            assert E.svmc_jump_sets_workspace_bytes(*args, C.byref(nb)) == INV
        assert E.svmc_jump_sets_workspace_bytes(n, 3, 18, 2, None) == INV
        rc, again, _, _, _ = c_tail(eng, m, fw, ks, ts, var, gm, True)
        assert rc == _lib.OK and np.array_equal(again, good)
    finally:
        eng.close()


def test_seventeen_expiries():
    import stochvolmodels_amd as sv
    p, n, seed, spy = hawkes_params(), 700, 8, 365
    ttms = np.arange(1, 18) / 365.0 * 1.5                         # two steps per slice: two stepping launches, 16 + 1
    assert [g[0] for g in ct.chain_grids(ttms, spy)] == [2] * 17
    rows = sv.hawkesjd_jump_rows(ttms, nb_path=n, seed=seed, nb_steps_per_year=spy, **model_kw(p))
    eng, _ = cond_rows(dict(p, sigma=0.0), ttms, n, seed, spy)
    try:
        want = eng.download(eng.snapshot_ptr(0), 17 * n).reshape(17, n)
    finally:
        eng.close()
    a = rows.numpy()
    assert np.array_equal(a, want) and rows.nb_steps == [2] * 17
    ks, ts, fw = [np.array([0.95, 1.05])] * 17, [np.array(["P", "C"])] * 17, np.full(17, 1.0)
    sigmas, gammas = [0.45, 0.3], [-1.0, 1.0]
    prices, stderrs, extra = rows.price_sets(sigmas, gammas, fw, ks, ts, recenter_forward=True, return_forwards=True)
    var = [rows.variances(s) for s in sigmas]
    out = (prices, stderrs, np.stack([x[2] for x in extra]), np.array([float(js.corr_of(a[i], 1.0, True)) for i in range(17)]))
    check_against_twin(out, list(a), fw, ks, ts, var, gammas, True, "17 expiries")
    rows.free()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def test_calibration_with_the_conditional_estimator():
    import stochvolmodels_amd as sv
    import test_jump_sets_host as host
    pricer = sv.HawkesJDPricer()
    p = host.hawkes_params()
    mc = dict(nb_path=host.CAL_N, nb_steps_per_year=host.CAL_SPY, seed=host.CAL_SEED)
    vols = host.market_vols(sv, pricer, sv.HawkesJDParams(**p), **mc)        # the route's own prices at the seed
    chain = host.cal_chain(sv, vols)
    fits = {}
    for batched in (True, False):
        params0 = sv.HawkesJDParams(**dict(p, sigma=host.CAL_START[0]), risk_premia_gamma=host.CAL_START[1])
        fit = pricer.calibrate_risk_premia_gamma_to_chain(chain, params0, estimator="conditional", print_iter=False, disp=False,
                                                          batched_gradient=batched, **mc)
        last = dict(pricer.last_calibration)
        assert fit is params0 and last["estimator"] == "conditional" and last["n_stepping_calls"] == 1
        assert (last["n_gradient_batches"] > 0) == batched
        fits[batched] = last
    # company changes no bits: the batch's vols are the single evaluations', so SLSQP walks the same path
    np.testing.assert_allclose(fits[True]["x"], fits[False]["x"], rtol=0, atol=1e-12)
    x = fits[True]["x"]
    err = np.abs(np.array([x[0], 8.0 * x[1]]) - np.array(host.CAL_TRUE))
    print(f"device calibration: x_fit = ({x[0]!r}, {8.0 * x[1]!r})  |x_fit - x*| = ({err[0]:.3e}, {err[1]:.3e})  bound {CAL_RECOVERY}  "
          f"objective {fits[True]['objective']:.3e}  nit {fits[True]['nit']}  status {fits[True]['status']}")
    assert err[0] <= CAL_RECOVERY[0] and err[1] <= CAL_RECOVERY[1]
    # the Fourier mode is untouched: its result dict has no new key
    params0 = sv.HawkesJDParams(**dict(p, sigma=host.CAL_START[0]), risk_premia_gamma=host.CAL_START[1])
    pricer.calibrate_risk_premia_gamma_to_chain(chain, params0, maxiter=2, print_iter=False, disp=False)
    assert set(pricer.last_calibration) == {"n_eval", "n_gradient_batches", "objective", "success", "status", "message", "nit", "nfev", "x"}
    pricer.calibrate_risk_premia_gamma_to_chain(chain, params0, maxiter=2, print_iter=False, disp=False, estimator="fourier")
    assert "estimator" not in pricer.last_calibration and "n_stepping_calls" not in pricer.last_calibration


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
# THE SIGMAS of item 8 come from the reference's own error, not from this estimator's results.  hawkesjd_chain_pricer_with_risk_premia
# integrates on 500 points up to 5.6 / (clip(sigma, 0.2, 0.5) sqrt(T)): the lower sigma, the coarser its grid, while the jumps' share of
# the transform does not shrink with it.  Its own error is read off by pricing the same set on the neighbouring grid scale (0.5 for a
# scale below 0.5, 0.45 at 0.5).  Measured on the MI355X in units of this estimator's standard error at 2^20 paths, the largest over
# the 20 options and the three gammas (profiles/hawkes_jump_sets_observed_tolerances.txt, 6.): sigma 0.60: 0.008; 0.45: 0.009; 0.30: 4.9
# (the put at 0.5 F: 1.874e-05 on its own grid, 1.634e-05, 1.600e-05 and 1.587e-05 on the scales 0.35, 0.45 and 0.5; the mean of 32
# seeds of this estimator is 1.603e-05 +- 1.4e-07); 0.20: 237.  A 4-standard-error criterion against that reference means something
# only where the reference's own error is a small part of one standard error: the parameter set's own 0.45, on which the committed
# z-scores of the existing route stand, and 0.60, whose grid is the finest the reference uses.  The test asserts that precondition
# (REFERENCE_SHARE) before it asserts the criterion.
Z_SIGMAS, Z_GAMMAS = (0.45, 0.6), (-1.0, 0.0, 1.0)
REFERENCE_SHARE = 0.1                  # of a standard error: the most the reference may move between neighbouring grid scales


def jump_sets_z_scores(nb_steps_per_year, nb_path=1 << 20, seed=2025, sigmas=Z_SIGMAS, gammas=Z_GAMMAS):
    """the chain of tests/test_gpu_tilted_cond.tilted_cond_z_scores (F = 1, one month, 20 strikes) at two sigmas and three gammas from ONE
    stepping launch: z-scores of the 20 options and of (normalizer, gamma forward) per set against the Fourier pricer under the kernel,
    and reference_shift: how far the reference moves on the neighbouring grid scale, in this estimator's standard errors"""
    import dataclasses
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    p = hp.HawkesJDParams()
    k = np.linspace(0.5, 1.5, 20)
    ttm = 1.0 / 12.0
    chain = dict(ttms=np.array([ttm]), forwards=np.array([1.0]), discfactors=np.array([1.0]), strikes_ttms=[k],
                 optiontypes_ttms=[np.where(k <= 1.0, "P", "C")])
    sets = [(s, g) for s in sigmas for g in gammas]
    kw = p.to_dict()
    kw.pop("risk_premia_gamma")
    kw.pop("sigma")
    pr, sd, fwds = hp.hawkesjd_mc_chain_pricer_conditional_sets([s for s, _ in sets], [g for _, g in sets], nb_path=nb_path, seed=seed,
                                                                nb_steps_per_year=nb_steps_per_year, return_forwards=True, **chain, **kw)
    out = {}
    for q, (sigma, gamma) in enumerate(sets):
        model = dataclasses.replace(p, sigma=sigma, risk_premia_gamma=gamma)
        ref, (norm, gfwd) = hp.hawkesjd_chain_pricer_with_risk_premia(model_params=model, return_forwards=True, **chain)
        own = float(np.clip(sigma, 0.2, 0.5))                    # hawkes_jd_pricer.set_vol_scaler's clip
        other = hp.hawkesjd_chain_pricer_with_risk_premia(model_params=model, vol_scaler=(0.5 if own < 0.5 else 0.45) * np.sqrt(ttm), **chain)
        st = fwds[q][2][0]
        out[f"sigma={sigma:.2f} gamma={gamma:+.0f}"] = dict(
            options=((pr[q][0] - ref[0]) / sd[q][0]).tolist(),
            normalizer=float((st[0] - norm[0]) / st[1]) if st[1] > 0.0 else float(st[0] - norm[0]),
            gamma_forward=float((st[2] - gfwd[0]) / st[3]), effective_sample_size=float(st[4]),
            reference_shift=(np.abs(other[0] - ref[0]) / sd[q][0]).tolist())
    return out


def test_every_set_agrees_with_the_fourier_pricer_under_the_kernel():
    """independent of any stream: 2^20 paths at 28 800 steps per year (test_gpu_tilted_cond's settings); every option of every set
    within 4 of its standard errors of hawkesjd_chain_pricer_with_risk_premia -- the reference's own criterion; a miss is to be
    examined at twice the steps (a step bias halves, a defect stays), never answered by a wider bound.  The sets: Z_SIGMAS x Z_GAMMAS,
    chosen by the reference's own error (the note above), which the test checks first.
    SVMC_JUMP_SETS_Z_SCORES=<file> keeps the z-scores (profiles/hawkes_jump_sets_z_scores.json)."""
    z = jump_sets_z_scores(28800)
    print("jump sets z-scores at 28800 steps/yr, 2^20 paths:", json.dumps(z))
    if os.environ.get("SVMC_JUMP_SETS_Z_SCORES"):
        with open(os.environ["SVMC_JUMP_SETS_Z_SCORES"], "w") as fh:
            json.dump(z, fh, indent=1)
    assert len(z) == 6
    shift = np.concatenate([np.array(v["reference_shift"]) for v in z.values()])
    print(f"the reference between neighbouring grid scales: at most {shift.max():.4f} standard errors (bound {REFERENCE_SHARE})")
    assert shift.size == 120 and np.all(shift <= REFERENCE_SHARE), shift
    allz = np.concatenate([np.array(v["options"]) for v in z.values()])
    assert allz.size == 120 and np.all(np.abs(allz) <= 4.0), allz


def test_the_reference_is_not_a_yardstick_at_low_sigma():
    """why item 8 stops at sigma 0.45: at 0.30 the reference moves by more than a standard error of this estimator between its own grid
    and the next finer one, at the low strikes; a z-score against it there measures the reference"""
    z = jump_sets_z_scores(28800, sigmas=(0.3,))
    shift = np.array([v["reference_shift"] for v in z.values()])
    print("sigma 0.30: the reference between neighbouring grid scales, in standard errors, per gamma:", shift.max(axis=1).tolist(),
          "z-scores of the put at 0.5 F:", [v["options"][0] for v in z.values()])
    assert shift.max() > 1.0
