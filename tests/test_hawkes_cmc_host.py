"""
The specification of conditional Monte Carlo for the Hawkes jump-diffusion, checked on the CPU: the twin
tests/hawkes_cmc_twin.py and the fixture tests/golden/hawkes_cmc_steps.npz (tests/golden/make_golden_hawkes_cmc.py).  Nothing here
runs the library, which has no kernel for this estimator yet; these are the yardsticks a device test is to use.

  1. the NumPy twin on the fixture's recorded inputs reproduces the errors the fixture stores for it, per path count -- the
     yardstick of a device test's bound (mc_steps_worker.bound with the Hawkes margins, as tests/test_gpu_mc_steps.py applies it to
     the plain step) -- and the fixture holds every case of its table with what its generator enforces: jumps on both sides
     wherever a case has at least 64 paths and 64 steps, at most one fragile path per case;
  2. the fixture sees a step constant off by 1e-13 (as tests/test_mc_steps_host.py shows for the plain step) and a swap of the two
     steps' word pairs of a stream-9 call; a slice may begin inside a call; the host formula of the variance;
  3. slicing, continuation and sharding by the global path index do not change the twin's bits;
  4. the estimator on the twin's (mu, cv): no jumps give Black-76 at sigma^2 T within 8 eps max(F, K) with every error exactly 0;
     sigma = 0 (cv == 0: the intrinsic value) is the plain estimator on the jump path to 1e-12 max(F, K);
  5. statistics at 2^16 paths on a 3-expiry chain of at most 120 steps: the twins of the conditional and of the plain estimator
     agree within 4.5 joint errors on every quote at hawkes_cmc_twin.STAT_SEED, and at the forward the plain error is the larger;
  6. the build's metadata: what the rows f11 to f15 tests count kernels by still counts what it did, and the library has no
     kernel for this estimator.
"""
import json
import math
import os
import re

import numpy as np
import pytest

import cmc_twin as ct
import hawkes_cmc_twin as hc
import hawkes_twin as ht
import mc_steps_worker as mw

MOVE = 1e-13
REPRO_FACTOR, REPRO_ULPS = 2.0, 2.0            # as tests/test_mc_steps_host.py: libm's exp / log may round differently


@pytest.fixture(scope="module")
def fx():
    return mw.Fixture(hc.FIXTURE)


def hawkes_params(name="hawkes_mc"):
    g = np.load(os.path.join(os.path.dirname(hc.FIXTURE), name + ".npz"))
    return dict(zip(ht.PARAM_NAMES, (float(v) for v in g["params"])))


def error_n(fx, case, state, n):
    """the fixture's error measure over the first n paths of a case"""
    hi, lo, fragile = fx.truth(case)
    return np.array(mw.measure(np.asarray(state)[:, :n], hi[:, :n], lo[:, :n], fragile[:n], case["scales"]))


def reproduced(got, stored):
    got, stored = np.asarray(got), np.asarray(stored)
    slack = REPRO_ULPS * mw.ULP
    return bool(np.all(got <= REPRO_FACTOR * stored + slack) and np.all(got >= stored / REPRO_FACTOR - slack))


def runs(fx):
    """{(set, offset): [case per expiry]}"""
    out = {}
    for c in fx.cases:
        out.setdefault((c["set"], c["offset"]), []).append(c)
    return out


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
def test_twin_reproduces_the_stored_errors(fx):
    m = fx.meta
    for (sname, offset), cases in runs(fx).items():
        p = cases[0]["params"]
        d = hc.draws(cases[0]["seed"], cases[0]["n"], sum(m["steps"]), offset)
        assert mw.checksum(*[d[k] for k in ("u_p", "u_m", "v_p", "v_m")]) == cases[0]["checksum"], \
            (sname, offset, "the random inputs moved: regenerate tests/golden/hawkes_cmc_steps.npz")
        twin = hc.np_chain(p, cases[0]["seed"], cases[0]["n"], m["steps"], m["dts"], offset)
        for case in cases:
            for n in m["path_counts"]:
                err = error_n(fx, case, np.stack(twin[case["expiry"]]), n)
                assert reproduced(err, case["oracle_err_n"][str(n)]), (case["id"], n, err, case["oracle_err_n"][str(n)])
                assert np.all(np.isfinite(case["oracle_err_n"][str(n)]))


def test_every_case_of_the_table_is_there(fx):
    m = fx.meta
    assert m["steps"] == [1, 2, 3, 7, 64, 451] and m["offsets"] == [0, 1] and m["path_counts"] == [1, 63, 64, 65, 513, 700]
    assert m["stream_tags"] == [hc.UNIFORM_TAG, hc.JUMP_TAG] == [9, 10] and m["prec"] == 256
    header = open(os.path.join(mw.ROOT, "include", "svmc.h")).read()
    assert m["rng_stream_version"] == int(re.search(r"#define SVMC_RNG_STREAM_VERSION (\d+)", header).group(1))
    ids = set(fx.by_id)
    for s in ("hawkes_mc", "hawkes_mc_excited"):
        for off in (0, 1):
            for i, steps in enumerate(m["steps"]):
                case = fx.by_id[f"{s}-o{off}-e{i}"]
                assert case["steps"] == steps and case["n"] == 700 and case["nq"] == 3
                fragile = fx.truth(case)[2]
                assert int(fragile.sum()) == case["fragile_paths"] <= m["max_fragile_paths"] == 1, case["id"]
                for n in m["path_counts"]:
                    assert int(fragile[:n].sum()) == case["fragile_n"][str(n)]
                    if n >= 64 and steps >= 64:
                        assert min(case["jumped_n"][str(n)]) >= 1, (case["id"], n)
    assert len(ids) == 24
    # an odd and an even step offset and odd and even step counts: boundaries fall on a call's edge and inside a call
    ends = {(off + c["end"]) & 1 for off in (0, 1) for c in fx.cases if c["offset"] == off}
    assert ends == {0, 1}
    assert os.path.getsize(hc.FIXTURE) < 1 << 20


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------
def test_a_slice_may_start_inside_a_call():
    """the stream's layout: the draws of steps [offset, offset + steps) are a window of the run from step 0, and a call's four words
    are two consecutive steps' pairs"""
    full = hc.draws(7, 5, 21, 0)
    for off in (1, 2, 3, 6):
        win = hc.draws(7, 5, 9, off)
        for k in ("u_p", "u_m", "v_p", "v_m"):
            assert np.array_equal(win[k], full[k][off:off + 9]), (off, k)
    w = np.stack(ht.stream_words(7, 0, hc.UNIFORM_TAG, 0, 5, 0, 2))           # [4][2 calls][5]
    w_p, w_m = hc.uniform_words(7, 5, 4, 0)
    assert np.array_equal(w_p, np.stack([w[0, 0], w[2, 0], w[0, 1], w[2, 1]]))
    assert np.array_equal(w_m, np.stack([w[1, 0], w[3, 0], w[1, 1], w[3, 1]]))
    e = ht.stream_words(7, 0, hc.JUMP_TAG, 0, 5, 3, 2)
    assert np.array_equal(hc.draws(7, 5, 2, 3)["v_p"], ht.uniform_from_words(e[0]))
    # independent of the plain pricer's draws at the same (seed, call id): another stream tag, other words
    plain = ht.stream_words(7, 0, ht.HAWKES_STREAM, 0, 5, 0, 2)
    assert not np.array_equal(plain[1], w[0])


def test_a_step_constant_off_by_1e_13_breaks_the_bound(fx):
    m = fx.meta
    case = fx.by_id["hawkes_mc-o0-e4"]                       # the expiry that ends the 64-step slice: 77 steps
    assert case["steps"] == 64
    n = case["n"]
    hi, _, fragile = fx.truth(case)
    scale = np.maximum(np.abs(hi), np.asarray(case["scales"])[:, None])[:, ~fragile]
    steps, dts = m["steps"][:5], m["dts"][:5]

    def state(scaled=None):
        return np.stack(hc.np_chain(case["params"], case["seed"], n, steps, dts, 0, scaled=scaled)[4])

    base = state()
    lim = mw.bound(case["oracle_err_n"][str(n)], "hawkes")
    assert np.all(error_n(fx, case, base, n) <= lim)          # the unmutated twin is inside the bound

    def move(st):
        return float(np.max(np.abs(st - base)[:, ~fragile] / scale))

    for name in hc.STEP_CONSTANTS:
        probe = 1e-9
        m0 = move(state((name, 1.0 + probe)))
        assert m0 > 0.0, name
        mutated = state((name, 1.0 + probe * MOVE / m0))
        assert 0.5 * MOVE <= move(mutated) <= 2.0 * MOVE, (name, move(mutated))
        err = error_n(fx, case, mutated, n)
        assert np.any(err > lim), (name, err.tolist(), lim.tolist())


def test_swapping_the_two_steps_word_pairs_breaks_the_bound(fx):
    m = fx.meta
    for cid in ("hawkes_mc-o0-e4", "hawkes_mc_excited-o1-e5"):
        case = fx.by_id[cid]
        i, n = case["expiry"], case["n"]
        good = hc.np_chain(case["params"], case["seed"], n, m["steps"][:i + 1], m["dts"][:i + 1], case["offset"])[i]
        swapped = hc.np_chain(case["params"], case["seed"], n, m["steps"][:i + 1], m["dts"][:i + 1], case["offset"], swap_halves=True)[i]
        lim = mw.bound(case["oracle_err_n"][str(n)], "hawkes")
        assert np.all(error_n(fx, case, np.stack(good), n) <= lim)
        assert np.all(error_n(fx, case, np.stack(swapped), n) > 1e6 * lim), cid        # other jumps altogether


def test_host_cv_formula():
    cv = hc.host_cv(0.45, [3, 7, 5], [0.02, 0.01, 0.02])
    want, acc = [], 0.0
    for nb, dt in ((3, 0.02), (7, 0.01), (5, 0.02)):
        acc = acc + nb * (0.45 * 0.45 * dt)
        want.append(acc)
    assert cv.tolist() == want
    assert hc.host_cv(0.45, [7, 5], [0.01, 0.02], cv_start=cv[0]).tolist() == want[1:]        # a continued chain: the same bits


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
def test_slicing_and_continuation_do_not_change_the_twins_bits(offset):
    p, n, seed, dt = hawkes_params("hawkes_mc_excited"), 257, 77, 0.01
    whole = hc.np_chain(p, seed, n, [3, 7, 5], [dt] * 3, offset, call_id=3)
    assert len(np.unique(whole[2][0])) > n // 2 and not np.array_equal(whole[0][0], whole[1][0])
    st, s = None, offset
    for i, nb in enumerate([3, 7, 5]):                        # three continued calls from the carried state
        st = hc.np_chain(p, seed, n, [nb], [dt], s, call_id=3, state=st)[0]
        assert all(np.array_equal(a, b) for a, b in zip(st, whole[i])), i
        s += nb
    tiny = hc.np_chain(p, seed, n, [1] * 17, [dt] * 17, offset, call_id=3)
    for i, end in enumerate((3, 10, 15)):                     # the one-step slices that end on the same global steps
        assert all(np.array_equal(a, b) for a, b in zip(tiny[end - 1], whole[i])), i
    # paths [0, 128) and [128, 257) by their global index concatenate to the whole job
    a = hc.np_chain(p, seed, 128, [3, 7, 5], [dt] * 3, offset, call_id=3)
    b = hc.np_chain(p, seed, 129, [3, 7, 5], [dt] * 3, offset, call_id=3, path0=128)
    for i in range(3):
        assert all(np.array_equal(np.concatenate([x, y]), w) for x, y, w in zip(a[i], b[i], whole[i]))
    assert not np.array_equal(whole[2][0], hc.np_chain(p, seed, n, [3, 7, 5], [dt] * 3, offset, call_id=4)[2][0])


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
QUOTE_K = np.concatenate([np.round(np.arange(0.8, 1.2001, 0.05), 2)] * 2)
QUOTE_T = np.array(["C"] * 9 + ["P"] * 9)


def black76(forward, strike, total_variance, put, discfactor):
    """the closed form on its own, from math.erfc: N(x) = erfc(-x / sqrt 2) / 2"""
    sd = math.sqrt(total_variance)
    d1 = math.log(forward / strike) / sd + 0.5 * sd
    d2 = d1 - sd

    def ncdf(x):
        return 0.5 * math.erfc(-x / math.sqrt(2.0))

    if put:
        return discfactor * (strike * ncdf(-d2) - forward * ncdf(-d1))
    return discfactor * (forward * ncdf(d1) - strike * ncdf(d2))


def test_no_jumps_is_black76_with_errors_exactly_zero():
    p = dict(hawkes_params(), sigma=0.45)
    for k in ("lambda_p", "lambda_m", "theta_p", "theta_m", "beta1_p", "beta2_p", "beta1_m", "beta2_m"):
        p[k] = 0.0
    n, ttms = 1000, (1.0 / 52.0, 1.0 / 12.0, 0.25)
    grids = ct.chain_grids(ttms, 480)
    nb, dts = [g[0] for g in grids], [g[1] for g in grids]
    states, cvs = hc.np_chain(p, 3, n, nb, dts), hc.host_cv(p["sigma"], nb, dts)
    for (mu, lp, lm), cv, ttm in zip(states, cvs, ttms):
        assert np.all(mu == mu[0]) and np.all(lp == 0.0) and np.all(lm == 0.0)
        for recenter in (True, False):
            prices, errs, stats = ct.estimator(mu, np.full(n, cv), 1.01, QUOTE_K, QUOTE_T, 0.99, recenter)
            want = np.array([black76(1.01, k, p["sigma"] ** 2 * ttm, t == "P", 0.99) for k, t in zip(QUOTE_K, QUOTE_T)])
            assert np.all(errs == 0.0) and stats["n_kept"] == n
            assert np.max(np.abs(prices - want) / np.maximum(1.01, QUOTE_K)) <= 8 * mw.ULP


def test_zero_sigma_is_the_plain_estimator_on_the_jump_path():
    p = dict(hawkes_params("hawkes_mc_excited"), sigma=0.0)
    n, ttms = 700, (1.0 / 52.0, 1.0 / 12.0, 0.25)
    grids = ct.chain_grids(ttms, 480)
    nb, dts = [g[0] for g in grids], [g[1] for g in grids]
    states, cvs = hc.np_chain(p, 12, n, nb, dts), hc.host_cv(0.0, nb, dts)
    assert np.all(cvs == 0.0)
    for (mu, _, _), df in zip(states, (0.999, 0.995, 0.99)):
        prices, errs, stats = ct.estimator(mu, np.zeros(n), 1.02, QUOTE_K, QUOTE_T, df)
        wp, we = ct.plain_estimator(mu, 1.02, QUOTE_K, QUOTE_T, df)
        assert stats["n_kept"] == n and np.all(errs > 0.0)
        assert np.max(np.abs(prices - wp) / np.maximum(1.02, QUOTE_K)) <= 1e-12
        assert np.max(np.abs(errs - we) / np.maximum(1.02, QUOTE_K)) <= 1e-12


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
def twin_conditional(p, chain, seed, n):
    grids = ct.chain_grids(hc.STAT_TTMS, hc.STAT_SPY)
    nb, dts = [g[0] for g in grids], [g[1] for g in grids]
    states = hc.np_chain(p, seed, n, nb, dts)
    cvs = hc.host_cv(p["sigma"], nb, dts)
    return [ct.estimator(st[0], np.full(n, cv), 1.0, k, t, df) for st, cv, k, t, df in
            zip(states, cvs, chain["strikes_ttms"], chain["optiontypes_ttms"], chain["discfactors"])]


def twin_plain(p, chain, seed, n):
    out, x, lp, lm, step0, t0 = [], np.zeros(n), np.full(n, p["lambda_p"]), np.full(n, p["lambda_m"]), 0, 0.0
    for ttm, k, t, df in zip(hc.STAT_TTMS, chain["strikes_ttms"], chain["optiontypes_ttms"], chain["discfactors"]):
        x, lp, lm, nb = ht.simulate_terminal(ttm - t0, x, lp, lm, p, seed, 0, 0, step0, hc.STAT_SPY)
        step0, t0 = step0 + nb, ttm
        out.append(ct.plain_estimator(x, 1.0, k, t, df))
    return out


def test_the_statistics_seed_keeps_both_twins_inside_the_bound():
    """the two estimators have one expectation for the same discretised model: the CPU twins of both on independent streams (9 / 10
    and 6 / 7) at hc.STAT_SEED.  A device test of the two pricers is to use this seed, at which both twins are shown here to stay
    inside the bound (it says nothing about other seeds)"""
    p = hawkes_params()
    chain, _ = hc.stat_chain(p)
    assert max(g[0] for g in ct.chain_grids(hc.STAT_TTMS, hc.STAT_SPY)) <= 120 and len(hc.STAT_TTMS) == 3
    cond, plain = twin_conditional(p, chain, hc.STAT_SEED, hc.STAT_N), twin_plain(p, chain, hc.STAT_SEED, hc.STAT_N)
    atm = hc.STAT_MONEYNESS.index(0.0)
    for i, ((cp, ce, _), (pp, pe)) in enumerate(zip(cond, plain)):
        z = (cp - pp) / np.hypot(ce, pe)
        print(f"hawkes cmc twins T={hc.STAT_TTMS[i]:.4f} max |z| {np.max(np.abs(z)):.2f} variance ratio at the forward "
              f"{(pe[atm] / ce[atm]) ** 2:.2f}")
        assert np.max(np.abs(z)) <= hc.Z_BOUND, (i, z)
        assert pe[atm] > ce[atm]


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------
def test_the_kernel_counts_of_the_earlier_rows_hold():
    from stochvolmodels_amd import build
    build.build()
    meta = json.load(open(build.ISA_JSON))["metadata"]
    assert len([k for k in meta if "cmc" in k]) == 8
    assert len([k for k in meta if "greeks" in k]) == 2
    assert len([k for k in meta if "cond_deriv" in k]) == 2
    hawkes = sorted(k for k in meta if "hawkesjd" in k)
    assert len(hawkes) == 3 and all("rng_kernel" in k or "rng_many_kernel" in k for k in hawkes), hawkes
    assert all(meta[k]["scratch_bytes"] == 0 for k in hawkes)
