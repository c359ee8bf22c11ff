"""
Monte Carlo prices under the exponential risk-premia kernel on the GPU (csrc/svmc_kernels.hip's
tilted_payoff_group_kernel / tilted_finish_kernel, svmc_hawkesjd_chain_price_tilted): the arithmetic against a long-double
brute force of include/svmc.h's estimator on uploaded state, bit-invariance against the company of a launch, gamma = 0 against
the plain pricer, one stepping launch for many gammas and the C ABI against the Python route, and the Monte Carlo against the
Fourier pricer under the kernel.

Deviations: |device - brute| / max(|brute|, 1e-4 scale), the parity measure of the other GPU tests (scale: the forward for
prices, gamma forwards and their errors; 1 for the normalizer and its error; none for the effective sample size).  Every
comparison prints its deviation and the module ends by printing the largest of each quantity (run with -s).  The bounds in TOL are
measured: ten times the largest deviation seen on the MI355X, rounded up to one digit, as profiles/tilted_observed_tolerances.txt
records them, and none above the project's parity bound for prices and states, 1e-12.  The prices' and errors' largest deviation
(7.5e-14) is the conditioning of a payoff spot - K that one path of 65 reaches, in the money by 1.4e-3, not the sums' order.
"""
import ctypes as C

import numpy as np
import pytest

import hawkes_twin as twin

pytestmark = pytest.mark.gpu

L_ = np.longdouble
GAMMAS = [-3.0, -1.0, 0.0, 0.5, 3.0]
FIELDS = ("price", "stderr", "normalizer", "normalizer_stderr", "gamma_forward", "gamma_forward_stderr", "effective_sample_size")
# ten times the largest deviation observed on the MI355X, rounded up to one digit (profiles/tilted_observed_tolerances.txt)
TOL = dict(price=8e-13, stderr=8e-13, normalizer=2e-15, normalizer_stderr=8e-15, gamma_forward=3e-15, gamma_forward_stderr=9e-15,
           effective_sample_size=5e-15)
assert max(TOL.values()) <= 1e-12      # the project's parity bound for prices and states: no bound here may exceed it
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def largest_deviations():
    """after the module's tests: the largest deviation of every quantity over its brute-force comparisons (shown with -s; the
    lines of profiles/tilted_observed_tolerances.txt)"""
    yield
    for k in FIELDS:
        print(f"\nlargest {k} deviation: {SEEN.get(k, float('nan')):.3e}  bound {TOL[k]:.0e}", end="")
    print()


def brute(x, forward, strikes, types, gamma, recenter):
    """include/svmc.h's estimator in long double; the keep rule is decided in double, as the device decides it"""
    with np.errstate(all="ignore"):
        corr64 = (np.nanmean(forward * np.exp(x)) - forward) if recenter else 0.0
        w64 = np.exp(gamma * x)
        s64 = forward * np.exp(x) - corr64
        keep = np.isfinite(x) & np.isfinite(w64 * w64) & np.isfinite((w64 * s64) ** 2)
        xl = x.astype(L_)
        corr = (np.nanmean(L_(forward) * np.exp(xl)) - L_(forward)) if recenter else L_(0)
        xk = xl[keep]
        w = np.exp(L_(gamma) * xk)
        spot = L_(forward) * np.exp(xk) - corr
        W, n = w.sum(), int(keep.sum())
        sg = np.where(np.asarray(types) == "C", 1.0, -1.0).astype(L_)
        pay = np.maximum(sg[None, :] * (spot[:, None] - np.asarray(strikes, dtype=L_)[None, :]), L_(0))
        price = (w[:, None] * pay).sum(axis=0) / W
        stderr = np.sqrt(((w[:, None] * (pay - price[None, :])) ** 2).sum(axis=0)) / W
        N = L_(n) / W
        gf = (w * spot).sum() / W
        stats = dict(normalizer=N, normalizer_stderr=np.sqrt(((1 - N * w) ** 2).sum()) / W, gamma_forward=gf,
                     gamma_forward_stderr=np.sqrt(((w * (spot - gf)) ** 2).sum()) / W, effective_sample_size=W * W / (w * w).sum())
    return price, stderr, stats, n, x.size - n


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
    SEEN[field] = max(SEEN.get(field, 0.0), dev)
    print(f"{what}: {field} deviation {dev:.3e} (bound {TOL[field]:.0e})")
    assert dev <= TOL[field], (what, field, dev)


def check_against_brute(out, xs, forwards, strikes, types, gammas, recenter, what):
    prices, stderrs, stats = out
    from stochvolmodels_amd.engine import TILTED_STATS_FIELDS as SF
    for g, gamma in enumerate(gammas):
        for i, x in enumerate(xs):
            p, e, st, n_kept, n_dropped = brute(x, forwards[i], strikes[i], types[i], gamma, recenter)
            row = dict(zip(SF, stats[g, i]))
            assert (row["n_kept"], row["n_dropped"]) == (n_kept, n_dropped), (what, gamma, i)
            tag = f"{what} gamma={gamma} expiry={i} n={x.size} K={len(strikes[i])} recenter={recenter}"
            note("price", deviation(prices[g][i], p, forwards[i]), tag)
            note("stderr", deviation(stderrs[g][i], e, forwards[i]), tag)
            for k in FIELDS[2:]:
                scale = forwards[i] if k.startswith("gamma_forward") else (1.0 if k.startswith("normalizer") else 0.0)
                note(k, deviation([row[k]], [st[k]], scale), tag)


def run_on_uploaded(xs, forwards, strikes, types, gammas, recenter, rows=None):
    """the reduction on state uploaded from the host: expiry i in snapshot row i (or the rows given)"""
    from stochvolmodels_amd.engine import get_engine, tilted_type_codes
    n = xs[0].size
    eng = get_engine(n)
    eng.reserve_snapshots(len(xs))
    for i, x in enumerate(xs):
        eng.upload(eng.snapshot_ptr(i), x)
    rows = list(range(len(xs))) if rows is None else rows
    return eng.tilted_payoffs([forwards[i] for i in rows], [strikes[i] for i in rows], [tilted_type_codes(types[i]) for i in rows],
                              gammas, recenter, snap_rows=rows)


def slice_of(n_strikes, forward):
    """n_strikes strikes around the forward, puts at or below it, calls above"""
    k = forward * (np.linspace(0.6, 1.5, n_strikes) if n_strikes > 1 else np.array([1.05]))
    return k, np.where(k <= forward, "P", "C")


def sample(n, seed, vol=0.2):
    return vol * np.random.default_rng(seed).standard_normal(n) - 0.5 * vol * vol


# 262 147 = PAYOFF_BLOCKS x BLOCK + 3: the grid-stride loop makes full trips through the prefetching loop and a ragged last one
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 262147])
@pytest.mark.parametrize("recenter", [False, True])
def test_arithmetic_against_long_double_over_path_counts(n, recenter):
    x = sample(n, 100 + n)
    k, t = slice_of(23, 1.3)                                    # 23: two strike groups
    out = run_on_uploaded([x], [1.3], [k], [t], GAMMAS, recenter)
    check_against_brute(out, [x], [1.3], [k], [t], GAMMAS, recenter, "paths")


COUNTS = [21, 22, 23, 45, 45, 1, 22, 23, 1]   # 15 strike groups: two launch pairs (8 + 7), the fifth expiry split between them


def nine_expiries(n=257):
    forwards = [1.0 + 0.05 * i for i in range(9)]
    xs = [sample(n, 7 + i, 0.1 + 0.03 * i) for i in range(9)]
    ks, ts = zip(*[slice_of(c, f) for c, f in zip(COUNTS, forwards)])
    return xs, forwards, list(ks), list(ts)


@pytest.mark.parametrize("recenter", [False, True])
def test_arithmetic_over_strike_counts_and_expiries(recenter):
    xs, fw, ks, ts = nine_expiries()
    out = run_on_uploaded(xs, fw, ks, ts, GAMMAS, recenter)                                  # 9 expiries: PAYOFF_GROUPS + 1
    check_against_brute(out, xs, fw, ks, ts, GAMMAS, recenter, "nine expiries")
    out = run_on_uploaded(xs[:2], fw[:2], ks[:2], ts[:2], GAMMAS, recenter)                  # 2 expiries
    check_against_brute(out, xs[:2], fw[:2], ks[:2], ts[:2], GAMMAS, recenter, "two expiries")
    for gamma in GAMMAS:                                                                     # 1 expiry, each gamma alone
        out = run_on_uploaded(xs[3:4], fw[3:4], ks[3:4], ts[3:4], [gamma], recenter)
        check_against_brute(out, xs[3:4], fw[3:4], ks[3:4], ts[3:4], [gamma], recenter, "one expiry, one gamma")


@pytest.mark.parametrize("recenter", [False, True])
def test_the_keep_rule(recenter):
    x = sample(300, 5)
    x[[3, 70, 130, 200, 250, 299]] = [np.nan, np.inf, -np.inf, 400.0, -400.0, np.nan]
    k, t = slice_of(5, 1.0)
    out = run_on_uploaded([x], [1.0], [k], [t], GAMMAS, recenter)
    check_against_brute(out, [x], [1.0], [k], [t], GAMMAS, recenter, "keep rule")
    from stochvolmodels_amd.engine import TILTED_STATS_FIELDS as SF
    kept = out[2][:, 0, SF.index("n_kept")]
    if recenter:       # the unweighted mean of F exp(x) holds exp(+inf): the recentring is infinite and no path is kept
        assert np.all(kept == 0) and np.all(np.isnan(np.concatenate([p[0] for p in out[0]])))
    else:              # NaN, NaN, +inf, -inf dropped everywhere, and under every gamma here one of +-400: -400 where gamma < 0
        assert kept.tolist() == [295.0] * 5          # overflows w^2, +400 where gamma >= 0 overflows (w spot)^2


def test_the_standard_error_survives_cancellation():
    """x = 0.01 z and a call at half the forward: the payoff is 0.5 F +- 1 %, its error two orders below it"""
    x = 0.01 * np.random.default_rng(11).standard_normal(4099)
    k, t = np.array([0.5 * 1.7, 1.7, 2.0 * 1.7]), np.array(["C", "C", "P"])
    for recenter in (False, True):
        out = run_on_uploaded([x], [1.7], [k], [t], GAMMAS, recenter)
        check_against_brute(out, [x], [1.7], [k], [t], GAMMAS, recenter, "low volatility")


def test_company_does_not_change_bits():
    xs, fw, ks, ts = nine_expiries()
    for recenter in (False, True):
        all_p, all_e, all_s = run_on_uploaded(xs, fw, ks, ts, GAMMAS, recenter)
        for g, gamma in enumerate(GAMMAS):
            p, e, s = run_on_uploaded(xs, fw, ks, ts, [gamma], recenter)                       # the gamma alone
            assert np.array_equal(s[0], all_s[g], equal_nan=True)
            for i in range(9):
                assert np.array_equal(p[0][i], all_p[g][i]) and np.array_equal(e[0][i], all_e[g][i])
        for i in (0, 3, 4, 8):                                                                  # the expiry alone
            p, e, s = run_on_uploaded(xs, fw, ks, ts, GAMMAS, recenter, rows=[i])
            for g in range(len(GAMMAS)):
                assert np.array_equal(p[g][0], all_p[g][i]) and np.array_equal(e[g][0], all_e[g][i])
                assert np.array_equal(s[g, 0], all_s[g, i])
        p, e, s = run_on_uploaded(xs, fw, ks, ts, [GAMMAS[3]], recenter, rows=[4])              # one gamma, one expiry
        assert np.array_equal(p[0][0], all_p[3][4]) and np.array_equal(e[0][0], all_e[3][4]) and np.array_equal(s[0, 0], all_s[3, 4])


def test_host_array_route():
    import stochvolmodels_amd as sv
    x = sample(1000, 3)
    k, t = slice_of(7, 1.1)
    k2 = k[:6].reshape(2, 3)
    p, e, st = sv.compute_mc_vars_payoff_with_gamma(x, 1.1, k2, t[:6].reshape(2, 3), -1.0, recenter_forward=True, return_stats=True)
    assert p.shape == e.shape == (2, 3) and isinstance(st["n_kept"], int) and st["n_kept"] == 1000
    bp, be, bst, _, _ = brute(x, 1.1, k[:6], t[:6], -1.0, True)
    note("price", deviation(p.ravel(), bp, 1.1), "host route")
    note("stderr", deviation(e.ravel(), be, 1.1), "host route")
    note("gamma_forward", deviation([st["gamma_forward"]], [bst["gamma_forward"]], 1.1), "host route")


def _chain(f):
    m = f["ttms"].size
    return (f["ttms"], f["forwards"], f["discfactors"], [f[f"strikes_{i}"] for i in range(m)], [f[f"types_{i}"] for i in range(m)])


def _kw(f):
    return dict(zip(twin.PARAM_NAMES, (float(v) for v in f["params"])))


def test_gamma_zero_recentred_is_the_plain_pricer(golden):
    from stochvolmodels_amd.engine import TILTED_STATS_FIELDS as SF
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    f = golden("hawkes_mc")
    ttms, fw, df, ks, ts = _chain(f)
    assert np.all(df == 1.0)
    n, seed = 1 << 14, 5150
    pr, sd = hp.hawkesjd_mc_chain_pricer(ttms=ttms, forwards=fw, discfactors=df, strikes_ttms=ks, optiontypes_ttms=ts, nb_path=n,
                                         seed=seed, **_kw(f))
    tp, te, fwd = hp.hawkesjd_mc_chain_pricer_with_risk_premia(ttms=ttms, forwards=fw, discfactors=df, strikes_ttms=ks,
                                                               optiontypes_ttms=ts, risk_premia_gamma=0.0, nb_path=n, seed=seed,
                                                               recenter_forward=True, return_forwards=True, **_kw(f))
    scale = np.repeat(fw, [k.size for k in ks])
    dp = np.max(np.abs(np.concatenate(tp) - np.concatenate(pr)) / np.maximum(np.abs(np.concatenate(pr)), 1e-4 * scale))
    de = np.max(np.abs(np.concatenate(te) - np.concatenate(sd)) / np.maximum(np.abs(np.concatenate(sd)), 1e-4 * scale))
    print(f"gamma = 0 against the plain pricer: prices {dp:.3e}, stderrs {de:.3e}")
    assert dp <= 1e-12 and de <= 1e-12
    normalizers, gamma_forwards, stats = fwd
    assert np.all(normalizers == 1.0)
    assert np.array_equal(stats[:, SF.index("effective_sample_size")], stats[:, SF.index("n_kept")])
    assert np.all(stats[:, SF.index("n_kept")] == n) and np.all(stats[:, SF.index("n_dropped")] == 0)
    np.testing.assert_allclose(gamma_forwards, fw, rtol=1e-12)      # recentred: the weighted mean spot IS the forward


def test_one_stepping_launch_and_the_c_abi(golden):
    from stochvolmodels_amd import _lib
    from stochvolmodels_amd.engine import get_engine, tilted_type_codes
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    f = golden("hawkes_mc")
    ttms, fw, df, ks, ts = _chain(f)
    n, seed = 20000, 777
    kw = dict(ttms=ttms, forwards=fw, discfactors=df, strikes_ttms=ks, optiontypes_ttms=ts, nb_path=n, seed=seed, **_kw(f))
    eng = get_engine(n)
    eng.start_kernel_timing()
    p5, e5, f5 = hp.hawkesjd_mc_chain_pricer_with_risk_premia_gammas(risk_premia_gammas=GAMMAS, return_forwards=True, **kw)
    timed = eng.stop_kernel_timing()
    state5 = eng.get_state()
    assert list(timed) == ["hawkesjd_chain_rng_kernel"] and len(timed["hawkesjd_chain_rng_kernel"]) == 1
    assert timed["hawkesjd_chain_rng_kernel"][0] > 0.0
    # each gamma is bit-equal to its single call ...
    p1, e1, f1 = hp.hawkesjd_mc_chain_pricer_with_risk_premia(risk_premia_gamma=GAMMAS[1], return_forwards=True, **kw)
    py_state = eng.get_state()
    for a, b in zip(state5, py_state):       # five gammas stepped the paths once: the terminal state of the one-gamma call
        assert np.array_equal(a, b)
    for i in range(ttms.size):
        assert np.array_equal(p1[i], p5[1][i]) and np.array_equal(e1[i], e5[1][i])
    assert np.array_equal(f1[2], f5[1][2])
    # ... and the single-gamma Python route to the C ABI on a session of its own
    L = _lib.load()
    dp = C.POINTER(C.c_double)
    strikes = np.concatenate(ks)
    codes = np.concatenate([tilted_type_codes(t) for t in ts])
    offs = np.concatenate([[0], np.cumsum([k.size for k in ks])]).astype(np.uintp)
    block = hp.params_block(**_kw(f))
    gam = np.array([GAMMAS[1]])
    prices, stderrs, stats = np.empty(strikes.size), np.empty(strikes.size), np.empty(8 * ttms.size)
    sess = C.c_void_p()
    _lib.check(L.svmc_session_create(C.byref(sess), n, ttms.size, strikes.size))
    try:
        _lib.check(L.svmc_hawkesjd_chain_price_tilted(sess, ttms.ctypes.data_as(dp), fw.ctypes.data_as(dp), ttms.size,
                                                      strikes.ctypes.data_as(dp), codes.ctypes.data_as(C.POINTER(C.c_int8)),
                                                      offs.ctypes.data_as(C.POINTER(C.c_size_t)), block.ctypes.data_as(dp), 1800, seed,
                                                      0, gam.ctypes.data_as(dp), 1, 0, prices.ctypes.data_as(dp),
                                                      stderrs.ctypes.data_as(dp), stats.ctypes.data_as(dp)))
        st = [np.empty(n) for _ in range(3)]
        _lib.check(L.svmc_session_state(sess, *[a.ctypes.data for a in st]))
        # everything is checked before anything is launched
        bad = np.array([np.nan])
        args = lambda g, ng, c: (sess, ttms.ctypes.data_as(dp), fw.ctypes.data_as(dp), ttms.size, strikes.ctypes.data_as(dp),   # noqa: E731
                                 c.ctypes.data_as(C.POINTER(C.c_int8)), offs.ctypes.data_as(C.POINTER(C.c_size_t)),
                                 block.ctypes.data_as(dp), 1800, seed, 0, g.ctypes.data_as(dp), ng, 0, prices.ctypes.data_as(dp),
                                 stderrs.ctypes.data_as(dp), stats.ctypes.data_as(dp))
        assert L.svmc_hawkesjd_chain_price_tilted(*args(bad, 1, codes)) == _lib.ERR_INVALID_ARGUMENT
        assert L.svmc_hawkesjd_chain_price_tilted(*args(gam, 0, codes)) == _lib.ERR_INVALID_ARGUMENT
        assert L.svmc_hawkesjd_chain_price_tilted(*args(np.zeros(17), 17, codes)) == _lib.ERR_INVALID_ARGUMENT
        inv = codes.copy()
        inv[0] = 2
        assert L.svmc_hawkesjd_chain_price_tilted(*args(gam, 1, inv)) == _lib.ERR_UNKNOWN_PAYOFF
    finally:
        L.svmc_session_destroy(sess)
    assert np.array_equal(prices, np.concatenate(p1)) and np.array_equal(stderrs, np.concatenate(e1))
    assert np.array_equal(stats.reshape(-1, 8), f1[2])
    for a, b in zip(st, py_state):
        assert np.array_equal(a, b)


def tilted_z_scores(nb_steps_per_year, nb_path=1 << 20, seed=2025):
    """the paper's slice under gamma = -1 and +1 in one call against the Fourier pricer under the kernel: z-scores of the 20
    options and of (normalizer, gamma forward) per gamma"""
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    p = hp.HawkesJDParams()
    ttms, fw, df = np.array([1.0 / 12.0]), np.array([1.0]), np.array([1.0])
    k = np.linspace(0.5, 1.5, 20)
    chain = dict(ttms=ttms, forwards=fw, discfactors=df, strikes_ttms=[k], optiontypes_ttms=[np.where(k <= 1.0, "P", "C")])
    gammas = [-1.0, 1.0]
    kw = p.to_dict()
    kw.pop("risk_premia_gamma")
    pr, sd, fwds = hp.hawkesjd_mc_chain_pricer_with_risk_premia_gammas(risk_premia_gammas=gammas, nb_path=nb_path, seed=seed,
                                                                       nb_steps_per_year=nb_steps_per_year, return_forwards=True,
                                                                       **chain, **kw)
    out = {}
    for g, gamma in enumerate(gammas):
        import dataclasses
        ref, (norm, gfwd) = hp.hawkesjd_chain_pricer_with_risk_premia(model_params=dataclasses.replace(p, risk_premia_gamma=gamma),
                                                                      return_forwards=True, **chain)
        st = fwds[g][2][0]
        out[f"gamma={gamma:+.0f}"] = dict(options=((pr[g][0] - ref[0]) / sd[g][0]).tolist(),
                                          normalizer=float((st[0] - norm[0]) / st[1]), gamma_forward=float((st[2] - gfwd[0]) / st[3]),
                                          effective_sample_size=float(st[4]))
    return out


def test_mc_agrees_with_fourier_under_the_kernel():
    """independent of any stream: 2^20 paths at 28 800 steps per year (test_mc_agrees_with_analytic_in_distribution's settings);
    every option within 4 of its standard errors of hawkesjd_chain_pricer_with_risk_premia, the normalizer and the gamma forward
    within 4 of theirs of hawkesjd_forwards_under_risk_kernel.  The 4 is the reference's own criterion; a miss is to be
    examined at twice the steps (a step bias halves, a defect stays), never answered by a wider bound."""
    import json
    z = tilted_z_scores(28800)
    print("tilted z-scores at 28800 steps/yr, 2^20 paths:", json.dumps(z))
    allz = np.concatenate([np.array(v["options"] + [v["normalizer"], v["gamma_forward"]]) for v in z.values()])
    assert allz.size == 44 and np.all(np.abs(allz) <= 4.0), allz
