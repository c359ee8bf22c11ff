"""
Conditional Monte Carlo for the Hawkes jump-diffusion on the device (include/svmc.h; csrc/svmc_hawkes.hip
hawkes_chain_cond_kernel), held to the CPU specification of tests/hawkes_cmc_twin.py and tests/test_hawkes_cmc_host.py.

  a. The 256-bit fixture tests/golden/hawkes_cmc_steps.npz: per (set, offset) run and path count 1, 63, 64, 65, 513, 700 ONE
     svmc_hawkesjd_chain_cond call of the fixture's six slices; row i of the mu snapshots and the intensities at expiry i (from six
     continued single-slice calls, which also exercise (step_offset, cv_start)) against the truth, fragile paths left out, within
     mc_steps_worker.bound(oracle_err_n, "hawkes") -- the bound tests/test_hawkes_cmc_host.py shows to see a step constant off by
     1e-13.  Every cv row is host_cv to the bit on every path.  SVMC_HAWKES_CMC_TOLERANCES=<file> keeps the observed err / oracle_err
     (profiles/hawkes_cmc_observed_tolerances.txt).
  b. Bits at n = 257, dt 0.01: slices [3, 7, 5] in one call = three continued calls = the matching ends of 17 one-step slices (two
     launches), step offsets 0 and 1; two shards by path_offset concatenate to the job; another call id gives other values; a replay
     the same bits.
  c. svmc_hawkesjd_chain_price_cmc = svmc_hawkesjd_chain_cond + svmc_cmc_payoff_chain on its rows, bit for bit, both recenter values,
     also on 17 expiries; the Python routes are the C ABI; the Greeks call's price / stderr are the price call's; price = F delta +
     K dual_delta and F^2 gamma = K^2 dual_gamma within tests/test_gpu_cmc_greeks.py's PARITY_BOUND; 17 slices = 16 + one continued.
  d. No jumps: Black-76 at sigma^2 T within 8 eps max(F, K), every error exactly 0, n_kept == n.  sigma = 0 (cv == 0): the plain
     estimator on the downloaded mu within 1e-12 max(F, K).
  e. Statistics at hawkes_cmc_twin.STAT_SEED, 2^16 paths: the conditional against the plain device pricer, |z| <= 4.5 on every quote,
     the plain error the larger at the forward.
  f. Every refusal of the three entries returns its status code and leaves the state as it was.
Each figure is printed before it is asserted (pytest -s).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import cmc_twin as ct
import hawkes_cmc_twin as hc
import hawkes_twin as ht
import mc_steps_worker as mw

pytestmark = pytest.mark.gpu

PARITY_BOUND = 1e-12           # tests/test_gpu_cmc_greeks.py's, for the same identities
QUOTE_K = np.concatenate([np.round(np.arange(0.8, 1.2001, 0.05), 2)] * 2)
QUOTE_T = np.array(["C"] * 9 + ["P"] * 9)
TTMS = (1.0 / 52.0, 1.0 / 12.0, 0.25)


def hawkes_params(name="hawkes_mc"):
    g = np.load(os.path.join(os.path.dirname(hc.FIXTURE), name + ".npz"))
    return dict(zip(ht.PARAM_NAMES, (float(v) for v in g["params"])))


def block_of(p):
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    return hp.params_block(**p)


def codes_of(types):
    return np.array([0 if t == "C" else 1 for t in types], dtype=np.int8)


def start_state(eng, p):
    n = eng.n_path
    eng.set_state(np.zeros(n), np.full(n, p["lambda_p"]), np.full(n, p["lambda_m"]))


def run_calls(p, n, seed, calls, call_id=0, path_offset=0):
    """calls: [(nb_steps list, dts list, step_offset)] continued from the origin (0, lambda_p, lambda_m), each with the cv the call
    before ended on; returns per call (mu rows [m][n], cv rows [m][n], host cvs [m], the state after it [3][n])"""
    from stochvolmodels_amd.engine import HipEngine
    eng = HipEngine(n, path_offset=path_offset)
    try:
        start_state(eng, p)
        out, cv = [], 0.0
        for nb, dts, off in calls:
            m = len(nb)
            cvs = eng.hawkesjd_chain_cond(nb, dts, block_of(p), seed, call_id, step_offset=off, cv_start=cv)
            rows = eng.download(eng.snapshot_ptr(0), 2 * m * n).reshape(2 * m, n)
            out.append((rows[:m].copy(), rows[m:].copy(), cvs.copy(), np.stack(eng.get_state())))
            cv = float(cvs[-1])
        return out
    finally:
        eng.close()


# ---- a ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import _lib
    f = mw.Fixture(hc.FIXTURE)
    assert f.meta["rng_stream_version"] == _lib.load().svmc_rng_stream_version() == sv.RNG_STREAM_VERSION
    return f


@pytest.mark.parametrize("sname", ["hawkes_mc", "hawkes_mc_excited"])
@pytest.mark.parametrize("offset", [0, 1])
def test_fixture_one_call_of_six_slices_per_path_count(fx, sname, offset):
    m = fx.meta
    steps, dts = m["steps"], m["dts"]
    cases = [fx.by_id[f"{sname}-o{offset}-e{i}"] for i in range(len(steps))]
    p, seed = cases[0]["params"], cases[0]["seed"]
    want_cv = hc.host_cv(p["sigma"], steps, dts)
    bad, lines = [], []
    for n in m["path_counts"]:
        (mu, cv, cvs, last), = run_calls(p, n, seed, [(steps, dts, offset)])
        assert np.array_equal(cvs, want_cv) and np.array_equal(cv, np.repeat(want_cv[:, None], n, axis=1)), (sname, offset, n)
        singles, s = [], offset                                  # six continued single-slice calls: the intermediate intensities
        for nb, dt in zip(steps, dts):
            singles.append(([nb], [dt], s))
            s += nb
        cont = run_calls(p, n, seed, singles)
        for i, (case, (mu1, cv1, cvs1, st)) in enumerate(zip(cases, cont)):
            assert np.array_equal(mu1[0], mu[i]) and np.array_equal(st[0], mu[i]), (case["id"], n, "a continued call moved mu")
            assert cvs1[0] == want_cv[i] and np.all(cv1[0] == want_cv[i]), (case["id"], n, "a continued call moved cv")
            hi, lo, fragile = fx.truth(case)
            err = np.array(mw.measure(np.stack([mu[i], st[1], st[2]]), hi[:, :n], lo[:, :n], fragile[:n], case["scales"]))
            oerr = np.array(case["oracle_err_n"][str(n)])
            lim = mw.bound(oerr, "hawkes")
            with np.errstate(all="ignore"):
                ratio = err / oerr
            line = (f"hawkes_cmc_steps {case['id']} n={n} oracle_err " + " ".join(f"{e:.2e}" for e in oerr) + " gpu_err "
                    + " ".join(f"{e:.2e}" for e in err) + " ratio " + " ".join(f"{r:.2f}" for r in ratio) + " ulps "
                    + " ".join(f"{e / mw.ULP:.2f}" for e in err))
            print(line)
            lines.append(line)
            if not np.all(err <= lim):
                bad.append((case["id"], n, err.tolist(), lim.tolist()))
        assert np.array_equal(cont[-1][3], last), (sname, offset, n, "the terminal state of the one call")
    if os.environ.get("SVMC_HAWKES_CMC_TOLERANCES"):
        with open(os.environ["SVMC_HAWKES_CMC_TOLERANCES"], "a") as fh:
            fh.write("\n".join(lines) + "\n")
    assert not bad, f"{len(bad)} figures past max(MARGIN x oracle_err, FLOOR_ULPS ulp) (mc_steps_worker.py): {bad[:6]}"


# ---- b ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
def test_slicing_continuation_and_sharding_keep_the_bits(offset):
    p, n, seed, dt = hawkes_params("hawkes_mc_excited"), 257, 77, 0.01
    (mu, cv, cvs, last), = run_calls(p, n, seed, [([3, 7, 5], [dt] * 3, offset)], call_id=3)
    assert len(np.unique(mu[2])) > n // 2 and not np.array_equal(mu[0], mu[1])
    assert np.array_equal(cvs, hc.host_cv(p["sigma"], [3, 7, 5], [dt] * 3))
    cont = run_calls(p, n, seed, [([3], [dt], offset), ([7], [dt], offset + 3), ([5], [dt], offset + 10)], call_id=3)
    for i, (mu1, cv1, cvs1, st) in enumerate(cont):               # three continued calls from the carried state
        assert np.array_equal(mu1[0], mu[i]) and np.array_equal(cv1[0], cv[i]) and cvs1[0] == cvs[i], i
    assert np.array_equal(cont[-1][3], last)
    (tmu, tcv, tcvs, tlast), = run_calls(p, n, seed, [([1] * 17, [dt] * 17, offset)], call_id=3)      # two launches: 16 + 1
    for i, end in enumerate((3, 10, 15)):                         # the one-step slices that end on the same global steps
        assert np.array_equal(tmu[end - 1], mu[i]), (i, "17 one-step slices")
    assert np.array_equal(cont[0][3], run_calls(p, n, seed, [([1] * 3, [dt] * 3, offset)], call_id=3)[0][3])     # intensities too
    # the twin on the same draws: the device's jumps are the twin's (no fragile path is pinned here: a loose bound)
    twin = hc.np_chain(p, seed, n, [3, 7, 5], [dt] * 3, offset, call_id=3)
    assert np.max(np.abs(mu[2] - twin[2][0])) <= 1e-9
    # paths [0, 128) and [128, 257) by their global index concatenate to the whole job
    (a, _, _, alast), = run_calls(p, 128, seed, [([3, 7, 5], [dt] * 3, offset)], call_id=3)
    (b, _, _, blast), = run_calls(p, 129, seed, [([3, 7, 5], [dt] * 3, offset)], call_id=3, path_offset=128)
    assert np.array_equal(np.concatenate([a, b], axis=1), mu) and np.array_equal(np.concatenate([alast, blast], axis=1), last)
    (other, _, _, _), = run_calls(p, n, seed, [([3, 7, 5], [dt] * 3, offset)], call_id=4)
    assert not np.array_equal(other[2], mu[2])
    (again, _, _, alast2), = run_calls(p, n, seed, [([3, 7, 5], [dt] * 3, offset)], call_id=3)
    assert np.array_equal(again, mu) and np.array_equal(alast2, last)


def test_seventeen_slices_equal_sixteen_plus_one_continued():
    p, n, seed = hawkes_params(), 130, 5
    nb, dts = [2] * 17, [0.004 + 0.0005 * i for i in range(17)]
    (mu, cv, cvs, last), = run_calls(p, n, seed, [(nb, dts, 1)])
    (mu16, cv16, cvs16, _), (mu1, cv1, cvs1, last1) = run_calls(p, n, seed, [(nb[:16], dts[:16], 1), (nb[16:], dts[16:], 33)])
    assert np.array_equal(mu[:16], mu16) and np.array_equal(mu[16], mu1[0]) and np.array_equal(last, last1)
    assert np.array_equal(cv[:16], cv16) and np.array_equal(cv[16], cv1[0]) and np.array_equal(cvs, np.concatenate([cvs16, cvs1]))
    assert np.array_equal(cvs, hc.host_cv(p["sigma"], nb, dts))


# ---- c ----------------------------------------------------------------------------------------------------------------------------
CHAIN = dict(ttms=np.array(TTMS), forwards=np.array([1.0, 1.01, 1.02]), discfactors=np.array([0.999, 0.995, 0.99]),
             strikes_ttms=[QUOTE_K] * 3, optiontypes_ttms=[QUOTE_T] * 3)
GREEKS_FIELDS = ("price", "stderr", "delta", "delta_stderr", "dual_delta", "dual_delta_stderr", "gamma", "gamma_stderr", "dual_gamma",
                 "dual_gamma_stderr")


def parts(p, chain, n, seed, spy, recenter, greeks=False):
    """the chain through svmc_hawkesjd_chain_cond and the tail entry on its rows, on an engine of its own"""
    from stochvolmodels_amd.engine import HipEngine
    grids = ct.chain_grids(chain["ttms"], spy)
    nb, dts = [g[0] for g in grids], [g[1] for g in grids]
    m = len(nb)
    eng = HipEngine(n)
    try:
        start_state(eng, p)
        eng.hawkesjd_chain_cond(nb, dts, block_of(p), seed, 0)
        codes = [codes_of(t) for t in chain["optiontypes_ttms"]]
        tail = eng.conditional_greeks if greeks else eng.conditional_payoffs
        return tail(chain["forwards"], chain["discfactors"], chain["strikes_ttms"], codes, recenter, mu_rows=list(range(m)),
                    cv_rows=list(range(m, 2 * m)))
    finally:
        eng.close()


@pytest.mark.parametrize("recenter", [True, False])
def test_the_fused_entries_are_their_parts_and_the_python_routes_are_the_c_abi(recenter):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.engine import get_engine, marshalled_chain
    p, n, seed, spy = hawkes_params("hawkes_mc_excited"), 5000, 5, 480
    wp, we, wst = parts(p, CHAIN, n, seed, spy, recenter)
    ch = marshalled_chain(CHAIN["ttms"], CHAIN["forwards"], CHAIN["discfactors"], CHAIN["strikes_ttms"],
                          [codes_of(t) for t in CHAIN["optiontypes_ttms"]])
    fp, fe, fst = get_engine(n).price_hawkesjd_chain_cmc_fused(ch, block_of(p), spy, recenter, seed, 0)
    pp, pe, pst = sv.hawkesjd_mc_chain_pricer_conditional(nb_path=n, seed=seed, nb_steps_per_year=spy, recenter=recenter,
                                                          return_stats=True, **CHAIN, **p)
    for i in range(3):
        assert np.array_equal(fp[i], wp[i]) and np.array_equal(fe[i], we[i]) and fst[i] == wst[i], (i, "fused against parts")
        assert np.array_equal(pp[i], wp[i]) and np.array_equal(pe[i], we[i]) and pst[i] == wst[i], (i, "function route")
        assert np.all(np.isfinite(wp[i])) and np.all(we[i] > 0.0) and wst[i]["n_kept"] == n
    chain = sv.OptionChain(ids=np.array(["a", "b", "c"]), **CHAIN)
    pricer, params = sv.HawkesJDPricer(), sv.HawkesJDParams(**p)
    cp, ce = pricer.model_mc_price_chain_conditional(chain, params, nb_path=n, seed=seed, nb_steps_per_year=spy, recenter=recenter)
    assert all(np.array_equal(a, b) for a, b in zip(cp + ce, wp + we))
    # the Greeks: the tail entry on the same rows, the fused entry, the function and the class route
    wg, wgst = parts(p, CHAIN, n, seed, spy, recenter, greeks=True)
    fg, fgst = get_engine(n).price_hawkesjd_chain_cmc_greeks_fused(ch, block_of(p), spy, recenter, seed, 0)
    g = sv.hawkesjd_mc_chain_greeks_conditional(nb_path=n, seed=seed, nb_steps_per_year=spy, recenter=recenter, return_stats=True,
                                                **CHAIN, **p)
    cg = pricer.model_mc_chain_greeks_conditional(chain, params, nb_path=n, seed=seed, nb_steps_per_year=spy, recenter=recenter)
    assert sorted(g) == sorted(GREEKS_FIELDS + ("stats",)) and sorted(cg) == sorted(GREEKS_FIELDS)
    for i in range(3):
        for f in GREEKS_FIELDS:
            assert np.array_equal(fg[f][i], wg[f][i]) and np.array_equal(g[f][i], wg[f][i]) and np.array_equal(cg[f][i], wg[f][i]), (i, f)
        assert fgst[i] == wgst[i] == g["stats"][i] and wgst[i]["n_zero_cv"] == 0
        assert np.array_equal(g["price"][i], wp[i]) and np.array_equal(g["stderr"][i], we[i])       # the price call's bits
        F, K = CHAIN["forwards"][i], QUOTE_K
        euler = np.abs(g["price"][i] - (F * g["delta"][i] + K * g["dual_delta"][i])) / F
        homog = np.abs(F * F * g["gamma"][i] - K * K * g["dual_gamma"][i]) / F
        print(f"hawkes cmc identities recenter={recenter} T={TTMS[i]:.4f} euler {euler.max():.2e} homogeneity {homog.max():.2e}")
        assert max(euler.max(), homog.max()) <= PARITY_BOUND
        assert np.all(g["gamma"][i] > 0.0) and np.all(g["dual_gamma_stderr"][i] > 0.0)


def test_a_fused_chain_of_seventeen_expiries_is_its_parts():
    from stochvolmodels_amd.engine import get_engine, marshalled_chain
    p, n, seed, spy = hawkes_params(), 700, 8, 365
    ttms = np.arange(1, 18) / 365.0 * 1.5                         # two steps per slice: two stepping launches, 16 + 1
    chain = dict(ttms=ttms, forwards=np.full(17, 1.0), discfactors=np.full(17, 0.99), strikes_ttms=[np.array([0.95, 1.05])] * 17,
                 optiontypes_ttms=[np.array(["P", "C"])] * 17)
    assert [g[0] for g in ct.chain_grids(ttms, spy)] == [2] * 17
    wp, we, wst = parts(p, chain, n, seed, spy, True)
    ch = marshalled_chain(chain["ttms"], chain["forwards"], chain["discfactors"], chain["strikes_ttms"],
                          [codes_of(t) for t in chain["optiontypes_ttms"]])
    fp, fe, fst = get_engine(n).price_hawkesjd_chain_cmc_fused(ch, block_of(p), spy, True, seed, 0)
    assert all(np.array_equal(a, b) for a, b in zip(fp + fe, wp + we)) and fst == wst


# ---- d ----------------------------------------------------------------------------------------------------------------------------
def black76(forward, strike, total_variance, put, discfactor):
    """the closed form on its own, from math.erfc (tests/test_hawkes_cmc_host.py's)"""
    sd = math.sqrt(total_variance)
    d1 = math.log(forward / strike) / sd + 0.5 * sd
    d2 = d1 - sd

    def ncdf(x):
        return 0.5 * math.erfc(-x / math.sqrt(2.0))

    if put:
        return discfactor * (strike * ncdf(-d2) - forward * ncdf(-d1))
    return discfactor * (forward * ncdf(d1) - strike * ncdf(d2))


@pytest.mark.parametrize("recenter", [True, False])
def test_no_jumps_is_black76_with_errors_exactly_zero(recenter):
    import stochvolmodels_amd as sv
    p = dict(hawkes_params(), sigma=0.45)
    for k in ("lambda_p", "lambda_m", "theta_p", "theta_m", "beta1_p", "beta2_p", "beta1_m", "beta2_m"):
        p[k] = 0.0
    n = 1000
    chain = dict(ttms=np.array(TTMS), forwards=np.full(3, 1.01), discfactors=np.full(3, 0.99), strikes_ttms=[QUOTE_K] * 3,
                 optiontypes_ttms=[QUOTE_T] * 3)
    prices, errs, stats = sv.hawkesjd_mc_chain_pricer_conditional(nb_path=n, seed=3, nb_steps_per_year=480, recenter=recenter,
                                                                  return_stats=True, **chain, **p)
    ok = True
    for i, ttm in enumerate(TTMS):
        want = np.array([black76(1.01, k, p["sigma"] ** 2 * ttm, t == "P", 0.99) for k, t in zip(QUOTE_K, QUOTE_T)])
        dev = np.max(np.abs(prices[i] - want) / np.maximum(1.01, QUOTE_K))
        print(f"hawkes cmc no jumps recenter={recenter} T={ttm:.4f} deviation {dev / mw.ULP:.2f} ulp of max(F, K)")
        assert np.all(errs[i] == 0.0) and stats[i]["n_kept"] == n and stats[i]["n_dropped"] == 0
        ok = ok and dev <= 8 * mw.ULP
    assert ok


def test_zero_sigma_is_the_plain_estimator_on_the_downloaded_jump_path():
    from stochvolmodels_amd.engine import HipEngine
    p = dict(hawkes_params("hawkes_mc_excited"), sigma=0.0)
    n = 700
    grids = ct.chain_grids(TTMS, 480)
    nb, dts = [g[0] for g in grids], [g[1] for g in grids]
    eng = HipEngine(n)
    try:
        start_state(eng, p)
        cvs = eng.hawkesjd_chain_cond(nb, dts, block_of(p), 12, 0)
        rows = eng.download(eng.snapshot_ptr(0), 6 * n).reshape(6, n)
        assert np.all(cvs == 0.0) and np.all(rows[3:] == 0.0)
        prices, errs, stats = eng.conditional_payoffs([1.02] * 3, [0.999, 0.995, 0.99], [QUOTE_K] * 3, [codes_of(QUOTE_T)] * 3, True,
                                                      mu_rows=[0, 1, 2], cv_rows=[3, 4, 5])
    finally:
        eng.close()
    for i, df in enumerate((0.999, 0.995, 0.99)):
        wp, we = ct.plain_estimator(rows[i], 1.02, QUOTE_K, QUOTE_T, df)
        dp = np.max(np.abs(prices[i] - wp) / np.maximum(1.02, QUOTE_K))
        de = np.max(np.abs(errs[i] - we) / np.maximum(1.02, QUOTE_K))
        print(f"hawkes cmc zero sigma T={TTMS[i]:.4f} price {dp:.2e} error {de:.2e}")
        assert stats[i]["n_kept"] == n and np.all(errs[i] > 0.0) and len(np.unique(rows[i])) > n // 2
        assert dp <= 1e-12 and de <= 1e-12


# ---- e ----------------------------------------------------------------------------------------------------------------------------
def test_statistics_against_the_plain_device_pricer():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    p = hawkes_params()
    chain, _ = hc.stat_chain(p)
    kw = dict(nb_path=hc.STAT_N, seed=hc.STAT_SEED, nb_steps_per_year=hc.STAT_SPY)
    cp, ce = sv.hawkesjd_mc_chain_pricer_conditional(**kw, **chain, **p)
    pp, pe = hp.hawkesjd_mc_chain_pricer(**kw, **chain, **p)
    atm, m = hc.STAT_MONEYNESS.index(0.0), len(hc.STAT_MONEYNESS)
    ok = True
    for i in range(3):
        z = (cp[i] - pp[i]) / np.hypot(ce[i], pe[i])
        ratio = (pe[i] / ce[i]) ** 2
        print(f"hawkes cmc statistics T={hc.STAT_TTMS[i]:.4f} max |z| {np.max(np.abs(z)):.2f} variance ratio at the forward "
              f"call {ratio[atm]:.2f} put {ratio[m + atm]:.2f} all " + " ".join(f"{r:.2f}" for r in ratio))
        ok = ok and bool(np.all(np.abs(z) <= hc.Z_BOUND)) and pe[i][atm] > ce[i][atm] and pe[i][m + atm] > ce[i][m + atm]
    assert ok


# ---- f ----------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_status_code_and_launches_nothing():
    from stochvolmodels_amd import _lib
    from stochvolmodels_amd.engine import HipEngine, marshalled_chain
    L = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    E, U = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNKNOWN_PAYOFF
    p, n = hawkes_params(), 130
    block = block_of(p)
    bp = block.ctypes.data_as(dp)
    nb, dts = np.array([3, 4], dtype=np.int32), np.array([0.01, 0.02])
    eng = HipEngine(n)
    try:
        eng.reserve_snapshots(4)
        sentinel = [np.full(n, v) for v in (0.125, 6.5, 8.5)]
        eng.set_state(*sentinel)
        eng.upload(eng.snapshot_ptr(0), np.full(4 * n, -7.0))
        x, lp, lm, s0, s1 = eng.x.ptr, eng.vol.ptr, eng.qvar.ptr, eng.snapshot_ptr(0), eng.snapshot_ptr(2)
        cvs = np.full(2, -1.0)

        def cond(x=x, lp=lp, lm=lm, n_path=n, m=2, nbs=nb, dt=dts, params=bp, cv0=0.0, call_id=0):
            return L.svmc_hawkesjd_chain_cond(x, lp, lm, n_path, m, None if nbs is None else nbs.ctypes.data_as(ip),
                                              None if dt is None else dt.ctypes.data_as(dp), params, cv0, 1, call_id, 0, 0, s0, s1,
                                              cvs.ctypes.data_as(dp), eng.stream)

        bad = block.copy()
        bad[3] = 1.5                                              # mean_p >= 1
        nan = block.copy()
        nan[1] = np.nan
        for what, rc in (("null mu", cond(x=None)), ("null lambda_p", cond(lp=None)), ("null lambda_m", cond(lm=None)),
                         ("no paths", cond(n_path=0)), ("no slices", cond(m=0)), ("null steps", cond(nbs=None)),
                         ("null dts", cond(dt=None)), ("negative steps", cond(nbs=np.array([3, -1], dtype=np.int32))),
                         ("zero dt", cond(dt=np.array([0.01, 0.0]))), ("infinite dt", cond(dt=np.array([np.inf, 0.01]))),
                         ("null params", cond(params=None)), ("mean_p", cond(params=bad.ctypes.data_as(dp))),
                         ("nan sigma", cond(params=nan.ctypes.data_as(dp))), ("call id", cond(call_id=1 << 24)),
                         ("negative cv_start", cond(cv0=-1e-300)), ("nan cv_start", cond(cv0=np.nan)),
                         ("infinite cv_start", cond(cv0=np.inf))):
            assert rc == E, (what, rc)
        # the fused entries on the engine's own session
        ch = marshalled_chain(np.array([0.05, 0.1]), np.ones(2), np.ones(2), [np.array([0.9, 1.1])] * 2, [np.array([0, 1], dtype=np.int8)] * 2)
        inverse = marshalled_chain(np.array([0.05, 0.1]), np.ones(2), np.ones(2), [np.array([0.9, 1.1])] * 2,
                                   [np.array([0, 2], dtype=np.int8), np.array([0, 1], dtype=np.int8)])
        junk = marshalled_chain(np.array([0.05, 0.1]), np.ones(2), np.ones(2), [np.array([0.9, 1.1])] * 2,
                                [np.array([0, 1], dtype=np.int8), np.array([9, 1], dtype=np.int8)])
        sess = eng.fused_chain_session(2, 4)
        res, stats = np.full((10, 4), -3.0), np.full((2, 6), -3.0)
        r0, r1, rs = res[0].ctypes.data_as(dp), res[1].ctypes.data_as(dp), stats.ctypes.data_as(dp)

        def price(c=ch, sess=sess, params=bp, spy=480, call_id=0, out=r0):
            return L.svmc_hawkesjd_chain_price_cmc(sess, c["ttms"], c["forwards"], c["discfactors"], c["m"], c["strikes"], c["codes"],
                                                   c["offsets"], params, spy, 1, 1, call_id, out, r1, rs)

        def greeks(c=ch, sess=sess, params=bp, spy=480, call_id=0, out=res.ctypes.data_as(dp)):
            return L.svmc_hawkesjd_chain_price_cmc_greeks(sess, c["ttms"], c["forwards"], c["discfactors"], c["m"], c["strikes"],
                                                          c["codes"], c["offsets"], params, spy, 1, 1, call_id, out, rs)

        for name, fn in (("price", price), ("greeks", greeks)):
            for what, rc, want in (("null session", fn(sess=None), E), ("null params", fn(params=None), E),
                                   ("mean_p", fn(params=bad.ctypes.data_as(dp)), E), ("no steps per year", fn(spy=0), E),
                                   ("call id", fn(call_id=1 << 24), E), ("null output", fn(out=None), E),
                                   ("an inverse payoff", fn(c=inverse), U), ("an unknown payoff", fn(c=junk), U)):
                assert rc == want, (name, what, rc)
        # nothing ran: the state, the snapshot rows and the outputs are as they were
        assert all(np.array_equal(a, b) for a, b in zip(eng.get_state(), sentinel))
        assert np.all(eng.download(s0, 4 * n) == -7.0) and np.all(cvs == -1.0) and np.all(res == -3.0) and np.all(stats == -3.0)
        # ... and the same calls unrefused run
        assert cond() == _lib.OK and price() == _lib.OK and greeks() == _lib.OK
        assert np.array_equal(cvs, hc.host_cv(p["sigma"], nb, dts)) and np.all(np.isfinite(res)) and stats[0, 3] == n
    finally:
        eng.close()
