"""
The conditional Monte Carlo chain pricers (include/svmc.h), checked without a device on the CPU twin
tests/cmc_twin.py and the fixture tests/golden/cmc_steps.npz (tests/golden/make_golden_cmc.py):

  1. the NumPy restatement of the two recursions against the 256-bit truth: it reproduces the errors the fixture stores for it (the
     yardstick of tests/test_gpu_cmc.py's bound) on inputs whose checksums the fixture recorded;
  2. statistics on the twin at 2^17 paths, LogSV "test" and Heston "base", maturities 1/12, 1/4, 1/2, strikes 0.8 (0.05) 1.2, calls
     and puts: (a) |mean F_c - F| <= 4 standard errors with recenter=False; (b) |conditional - plain| <= 4 hypot(se_cond, se_plain)
     per quote, plain the twin's own two-Brownian run on independent draws and se_plain the larger of the call's and the put's
     error at that strike (the two differences are equal by parity, and the recentring's noise sits on the call side); (c)
     se_cond <= se_plain on every quote priced above 1e-3 F;
  3. mutations, each breaking a named assertion: dropping -rho^2 V / 2 from mu + cv / 2 breaks (a) and NOT the recentred prices of
     (b) -- the recentring absorbs a factor common to all paths' forwards only approximately, and here within the noise; the sign
     of rho breaks (b); cv without its (1 - rho^2) breaks (a) and (b); a step constant off by 1e-13 breaks the fixture's bound;
  4. beta = volvol = 0 and no mean reversion: every path's price is Black-76 at sigma0 and the error is exactly 0;
  5. the build's metadata (libsvmc.isa.json): no new kernel uses scratch, the stepping pair reaches eight waves per SIMD.
"""
import json
import os

import numpy as np
import pytest

import cmc_twin as ct
import mc_steps_worker as mw

MOVE = 1e-13
REPRO_FACTOR, REPRO_ULPS = 2.0, 2.0            # as tests/test_mc_steps_host.py: libm's exp / log may round differently
N_STAT = 1 << 17
TTMS = (1.0 / 12.0, 0.25, 0.5)
STRIKES = np.round(np.arange(0.8, 1.2001, 0.05), 2)
F = 1.0
SETS = {"logsv": dict(sigma0=0.2, theta=0.22, kappa1=3.0, kappa2=12.0, beta=-0.3, volvol=0.4),
        "heston": dict(v0=0.04, theta=0.04, kappa=4.0, rho=-0.5, volvol=0.4)}
QUOTE_K = np.concatenate([STRIKES, STRIKES])
QUOTE_T = np.array(["C"] * STRIKES.size + ["P"] * STRIKES.size)


@pytest.fixture(scope="module")
def fx():
    return mw.Fixture(ct.FIXTURE)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
def reproduced(got, stored):
    got, stored = np.asarray(got), np.asarray(stored)
    slack = REPRO_ULPS * mw.ULP
    return bool(np.all(got <= REPRO_FACTOR * stored + slack) and np.all(got >= stored / REPRO_FACTOR - slack))


@pytest.mark.parametrize("gen", ["logsv", "heston"])
def test_numpy_restatement_reproduces_the_stored_errors(fx, gen):
    cases = [c for c in fx.cases if c["gen"] == gen]
    assert cases
    for case in cases:
        B = ct.case_normals(case)
        assert mw.checksum(B) == case["checksum"], (case["id"], "the random inputs moved: regenerate tests/golden/cmc_steps.npz")
        err = fx.error(case, ct.restate(case, B))
        assert reproduced(err, case["oracle_err"]), (case["id"], err, case["oracle_err"])
        assert np.all(np.isfinite(case["oracle_err"]))


def test_every_case_of_the_table_is_there(fx):
    ids = set(fx.by_id)
    for gen, sets in (("logsv", ("btc", "test", "zero")), ("heston", ("base", "btc", "rho_m1"))):
        for s in sets:
            for st in (1, 2, 3, 4, 5, 7, 8, 9, 64):
                for off in (0, 1, 2, 3):
                    assert f"{gen}-{s}-s{st}-o{off}" in ids
    assert {"logsv-btc-s1024-o0", "heston-btc-s1024-o0"} <= ids
    assert all(c["n"] == (64 if c["steps"] == 1024 else 130) and c["nq"] == 4 for c in fx.cases)
    assert fx.by_id["logsv-zero-s64-o0"]["params"]["beta"] == fx.by_id["logsv-zero-s64-o0"]["params"]["volvol"] == 0.0
    assert fx.by_id["heston-rho_m1-s64-o0"]["params"]["rho"] == -1.0
    assert fx.meta["stream_tag"] == ct.TAG == 8
    for case in fx.cases:
        fragile = fx.truth(case)[2]
        assert int(fragile.sum()) == case["fragile_paths"] and fragile.mean() <= fx.meta["max_fragile_share"] == 0.01, case["id"]
    assert os.path.getsize(ct.FIXTURE) < max(os.path.getsize(os.path.join(os.path.dirname(ct.FIXTURE), f))
                                             for f in os.listdir(os.path.dirname(ct.FIXTURE)) if f != "cmc_steps.npz" and f.endswith(".npz"))


def test_a_slice_may_start_anywhere_inside_a_call():
    """the stream's layout: the normals of steps [offset, offset + steps) are a window of the run from step 0"""
    full = ct.normals(7, 5, 21, 0)
    for off in (1, 2, 3, 4, 6):
        assert np.array_equal(ct.normals(7, 5, 9, off), full[off:off + 9])
    w = np.stack(ct.ht.stream_words(7, 0, ct.TAG, 0, 5, 0, 2))
    assert np.array_equal(ct.step_words(7, 5, 8, 0), np.concatenate([w[:, 0, :], w[:, 1, :]]))


# ---- 3 (the fixture's bound) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", ["logsv", "heston"])
def test_a_step_constant_off_by_1e_13_breaks_the_device_bound(fx, gen):
    case = fx.by_id[{"logsv": "logsv-btc-s64-o0", "heston": "heston-base-s64-o0"}[gen]]
    B = ct.case_normals(case)
    hi, _, fragile = fx.truth(case)
    scale = np.maximum(np.abs(hi), np.asarray(case["scales"])[:, None])[:, ~fragile]
    base = ct.restate(case, B)
    lim = mw.bound(case["oracle_err"], gen)
    assert np.all(np.array(fx.error(case, base)) <= lim)

    def move(state):
        return float(np.max(np.abs(state - base)[:, ~fragile] / scale))

    for name in ct.STEP_CONSTANTS[gen]:
        probe = 1e-9
        m0 = move(ct.restate(case, B, scaled=(name, 1.0 + probe)))
        assert m0 > 0.0, name
        mutated = ct.restate(case, B, scaled=(name, 1.0 + probe * MOVE / m0))
        assert 0.5 * MOVE <= move(mutated) <= 2.0 * MOVE, (name, move(mutated))
        err = np.array(fx.error(case, mutated))
        assert np.any(err > lim), (name, err.tolist(), lim.tolist())


# ---- 2 and 3: statistics ------------------------------------------------------------------------------------------------------------
def twin_chain(model, mutate=None, seed=11):
    """[(mu, cv)] per expiry of the twin's conditional chain at N_STAT paths"""
    p, out, off = SETS[model], [], 0
    vol0 = p["sigma0"] if model == "logsv" else p["v0"]
    st = [np.zeros(N_STAT), np.zeros(N_STAT), np.full(N_STAT, vol0), np.zeros(N_STAT)]
    for nb, dt in ct.chain_grids(TTMS, 360):
        B = ct.normals(seed, N_STAT, nb, off, exact=False)
        st = ct.np_logsv(st, dt, p, 1.0, True, B, mutate) if model == "logsv" else ct.np_heston(st, dt, p, B, mutate)
        out.append((st[0].copy(), st[1].copy()))
        off += nb
    return out


def twin_plain_chain(model, seed=12):
    """[x] per expiry of the twin's two-Brownian chain on independent draws"""
    p, out = SETS[model], []
    rng = np.random.default_rng(seed)
    x, v = np.zeros(N_STAT), np.full(N_STAT, p["sigma0"] if model == "logsv" else p["v0"])
    for nb, dt in ct.chain_grids(TTMS, 360):
        W0, W1 = rng.standard_normal((nb, N_STAT)), rng.standard_normal((nb, N_STAT))
        x, v = ct.np_logsv_plain(x, v, dt, p, 1.0, W0, W1) if model == "logsv" else ct.np_heston_plain(x, v, dt, p, W0, W1)
        out.append(x.copy())
    return out


@pytest.fixture(scope="module")
def stat_runs():
    return {m: dict(cond=twin_chain(m), plain=[ct.plain_estimator(x, F, QUOTE_K, QUOTE_T) for x in twin_plain_chain(m)])
            for m in ("logsv", "heston")}


def forward_z(chain):
    """(a): (mean F_c - F) / its standard error per expiry, recenter=False"""
    z = []
    for mu, cv in chain:
        st = ct.estimator(mu, cv, F, [], [], recenter=False)[2]
        z.append((st["forward_mc"] - F) / st["forward_mc_stderr"])
    return np.array(z)


def quote_figures(chain, plain):
    """(b), (c): per expiry (z per quote, se_cond, se_plain, prices)"""
    out = []
    for (mu, cv), (pp, pe) in zip(chain, plain):
        cp, ce, _ = ct.estimator(mu, cv, F, QUOTE_K, QUOTE_T)
        se_plain = np.tile(np.maximum(pe[:STRIKES.size], pe[STRIKES.size:]), 2)
        out.append(((cp - pp) / np.hypot(ce, se_plain), ce, se_plain, cp))
    return out


@pytest.mark.parametrize("model", ["logsv", "heston"])
def test_statistics_on_the_twin(stat_runs, model):
    r = stat_runs[model]
    z = forward_z(r["cond"])
    print("cmc twin", model, "forward z", np.round(z, 2))
    assert np.all(np.abs(z) <= 4.0), z                                   # (a)
    for i, (zq, ce, se_plain, cp) in enumerate(quote_figures(r["cond"], r["plain"])):
        print("cmc twin", model, f"T={TTMS[i]:.3f} max |z| {np.max(np.abs(zq)):.2f} variance ratio min "
              f"{np.min((se_plain / ce) ** 2):.1f} max {np.max((se_plain / ce) ** 2):.1f}")
        assert np.all(np.abs(zq) <= 4.0), (i, zq)                        # (b)
        priced = cp > 1e-3 * F
        assert np.all(ce[priced] <= se_plain[priced]), (i, ce, se_plain)  # (c)


@pytest.mark.parametrize("model", ["logsv", "heston"])
def test_mutation_dropping_half_rho2_v_breaks_the_forward_check_only(stat_runs, model):
    """F_c = F exp(mu + cv / 2) with cv / 2 taken WITHOUT its (1 - rho^2): the forward's mean leaves 1 by many standard errors (a);
    the recentred prices stay inside (b) -- the recentring takes the common factor out again, so (b) alone would not catch it"""
    p = SETS[model]
    rho2 = ct.logsv_rho_factor(p["beta"], p["volvol"])[1] ** 2 if model == "logsv" else p["rho"] ** 2
    mutated = [(mu + 0.5 * cv * rho2 / (1.0 - rho2), cv) for mu, cv in stat_runs[model]["cond"]]
    assert np.all(np.abs(forward_z(mutated)) > 4.0)
    for zq, _, _, _ in quote_figures(mutated, stat_runs[model]["plain"]):
        assert np.all(np.abs(zq) <= 4.0)


def test_mutation_the_sign_of_rho_breaks_the_price_check(stat_runs):
    for model in ("logsv", "heston"):
        figs = quote_figures(twin_chain(model, mutate="rho_sign"), stat_runs[model]["plain"])
        assert max(np.max(np.abs(zq)) for zq, _, _, _ in figs) > 4.0, model


def test_mutation_cv_without_its_factor_breaks_both_checks(stat_runs):
    for model in ("logsv", "heston"):
        chain = twin_chain(model, mutate="cv_no_factor")
        assert np.all(np.abs(forward_z(chain)) > 4.0), model
        assert max(np.max(np.abs(zq)) for zq, _, _, _ in quote_figures(chain, stat_runs[model]["plain"])) > 4.0, model


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
def test_zero_volvol_beta_and_mean_reversion_is_black76():
    from scipy.special import ndtr
    p = dict(sigma0=0.3, theta=0.3, kappa1=0.0, kappa2=0.0, beta=0.0, volvol=0.0)
    n, nb, dt = 1024, 90, 0.25 / 90
    st = [np.zeros(n), np.zeros(n), np.full(n, p["sigma0"]), np.zeros(n)]
    mu, cv, s, q = ct.np_logsv(st, dt, p, 1.0, True, ct.normals(3, n, nb, 0))
    assert np.all(s == s[0]) and np.all(mu == mu[0]) and np.all(cv == cv[0])
    prices, errs, stats = ct.estimator(mu, cv, F, QUOTE_K, QUOTE_T, discfactor=0.97)
    cv1 = np.full(2, p["sigma0"] ** 2 * 0.25)
    want = ct.estimator(-0.5 * cv1, cv1, F, QUOTE_K, QUOTE_T, 0.97, recenter=False)[0]      # Black-76 at sigma0, long double
    sd = p["sigma0"] * np.sqrt(0.25)
    d1 = np.log(F / QUOTE_K) / sd + 0.5 * sd
    assert np.allclose(want, 0.97 * np.where(QUOTE_T == "C", F * ndtr(d1) - QUOTE_K * ndtr(d1 - sd), QUOTE_K * ndtr(sd - d1) - F * ndtr(-d1)),
                       rtol=1e-9, atol=1e-15)
    assert np.max(np.abs(prices - want) / np.maximum(np.abs(want), 1e-4 * F)) < 1e-12
    assert np.all(errs == 0.0) and stats["n_kept"] == n and abs(stats["corr"]) < 1e-15


# ---- the refusals (raised before any device work: this machine needs no device for them) -------------------------------------------
def test_unsupported_requests_are_refused_before_any_device_work():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import VariableType
    chain = dict(ttms=np.array([0.25]), forwards=np.array([1.0]), discfactors=np.array([1.0]), strikes_ttms=[np.array([1.0])],
                 optiontypes_ttms=[np.array(["C"])], nb_path=64, seed=1)
    lkw = dict(v0=0.2, theta=0.2, kappa1=1.0, kappa2=1.0, beta=-0.3, volvol=0.4, vol_backbone_etas=np.ones(1))
    hkw = dict(v0=0.04, theta=0.04, kappa=4.0, rho=-0.5, volvol=0.4)

    class Two:
        world, rank = 2, 0

    for fn, kw in ((sv.logsv_mc_chain_pricer_conditional, lkw), (sv.heston_mc_chain_pricer_conditional, hkw)):
        for bad in ("IC", "IP"):
            with pytest.raises(ValueError, match="not implemented"):
                fn(**dict(chain, optiontypes_ttms=[np.array([bad])]), **kw)
        with pytest.raises(NotImplementedError):
            fn(variable_type=VariableType.Q_VAR, **chain, **kw)
        with pytest.raises(NotImplementedError):
            fn(devices=2, **chain, **kw)
        with pytest.raises(NotImplementedError):
            fn(comm=Two(), **chain, **kw)
    with pytest.raises(NotImplementedError):
        sv.logsv_mc_chain_pricer_conditional(is_spot_measure=False, **chain, **lkw)
    with pytest.raises(NotImplementedError):
        sv.heston_mc_chain_pricer_conditional(scheme="qe", **chain, **hkw)
    with pytest.raises(ValueError, match="not implemented"):
        sv.compute_mc_vars_payoff_conditional(np.zeros(4), np.ones(4), 1.0, 1.0, np.array([1.0]), np.array(["IC"]))


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch_and_the_stepping_pair_reaches_eight_waves():
    from stochvolmodels_amd import build
    build.build()
    meta = json.load(open(build.ISA_JSON))["metadata"]
    cmc = {k: v for k, v in meta.items() if "cmc" in k}
    for stem in ("logsv_chain_cmc_kernel", "logsv_chain_cmc_lat_kernel", "heston_chain_cmc_kernel", "heston_chain_cmc_lat_kernel",
                 "cmc_forward_kernel", "cmc_forward_finish_kernel", "cmc_payoff_kernel", "cmc_finish_kernel"):
        hit = [k for k in cmc if stem + "E" in k]
        assert len(hit) == 1, (stem, sorted(cmc))
        assert cmc[hit[0]]["scratch_bytes"] == 0, (stem, cmc[hit[0]])
    assert len(cmc) == 8 and not any("rng_kernel" in k for k in cmc)
    # gfx950: 512 vector registers per lane of a SIMD in granules of 8, 160 KB of LDS per CU, 4 SIMDs; waves of a block / 64 lanes
    for stem, block in (("logsv_chain_cmc_kernelE", 1024), ("heston_chain_cmc_kernelE", 512)):
        m = [v for k, v in cmc.items() if stem in k][0]
        by_regs = 512 // (-(-m["vgpr"] // 8) * 8)
        by_lds = (160 * 1024 // m["lds_bytes"]) * (block // 64) // 4
        assert min(by_regs, by_lds, 8) == 8, (stem, m, by_regs, by_lds)
