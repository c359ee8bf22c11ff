"""
The conditional Monte Carlo Greeks (include/svmc.h), checked without a device on the long-double twin
tests/cmc_greeks_twin.py:

  1. the twin's delta, dual delta, gamma and dual gamma equal central differences (h = 1e-4) of tests/cmc_twin.py's estimator in F
     and in K, calls and puts, a strike with K' <= 0, both recentring settings, planted dropped and cv == 0 paths.  Measured: 1e-8
     for the first derivatives and 3e-7 for the second (the differences' truncation); asserted at 1e-7 / 3e-6;
  2. a twin with one wrong term -- c B_k dropped from delta, or K' for K in gamma's factor -- fails 1 by orders of magnitude;
  3. price = F delta + K dual_delta and F^2 gamma = K^2 dual_gamma to 1e-14 relative;
  4. the host refusals are check_conditional_request's, raised before any device work;
  5. the density composition on planted (mu, cv) integrates to the kept, non-degenerate share within 1e-6 on x in [-1.5, 1], 501
     points;
  6. the build's metadata (libsvmc.isa.json): the two new kernels use no scratch.
"""
import json

import numpy as np
import pytest

import cmc_greeks_twin as gt
import cmc_twin as ct

H = 1e-4
FIRST_BOUND, SECOND_BOUND = 1e-7, 3e-6
F0, D0 = 1.0, 0.97
N = 4096
STRIKES = np.array([-0.05, 0.7, 0.85, 0.95, 1.0, 1.03, 1.15, 1.3, 0.9, 1.1])
TYPES = np.array(["C", "C", "P", "C", "P", "C", "P", "C", "C", "P"])


def synthetic(n, seed, plant=(), drop_first=False):
    """tests/test_gpu_cmc.py's inputs, restated"""
    rng = np.random.default_rng(seed)
    cv = rng.uniform(0.004, 0.06, n)
    mu = -0.5 * cv + 0.1 * rng.standard_normal(n)
    bad = 0
    if "bad" in plant and n >= 64:
        mu[5], mu[17], mu[40] = np.nan, np.inf, -np.inf
        cv[9], cv[23], cv[33] = -1e-3, np.inf, np.nan
        mu[50] = 800.0
        bad = 7
    if "zero_cv" in plant and n >= 64:
        cv[3] = 0.0
    if drop_first:
        mu[0] = np.nan
        bad += 1
    return mu, cv, bad


def central_differences(mu, cv, recenter):
    """(dP/dF, dP/dK, d2P/dF2, d2P/dK2) of cmc_twin.estimator's prices, [K] each"""
    def price(f=F0, dk=0.0):
        return ct.estimator(mu, cv, f, STRIKES + dk, TYPES, D0, recenter)[0]
    p0 = price()
    fu, fd, ku, kd = price(f=F0 + H), price(f=F0 - H), price(dk=H), price(dk=-H)
    return (fu - fd) / (2 * H), (ku - kd) / (2 * H), (fu - 2 * p0 + fd) / (H * H), (ku - 2 * p0 + kd) / (H * H)


def difference_figures(mu, cv, recenter, mutate=None):
    g, _ = gt.estimator(mu, cv, F0, STRIKES, TYPES, D0, recenter, mutate)
    dF, dK, d2F, d2K = central_differences(mu, cv, recenter)
    return dict(delta=np.max(np.abs(g["delta"] - dF)), dual_delta=np.max(np.abs(g["dual_delta"] - dK)),
                gamma=np.max(np.abs(g["gamma"] - d2F)), dual_gamma=np.max(np.abs(g["dual_gamma"] - d2K)))


@pytest.mark.parametrize("recenter", [True, False])
@pytest.mark.parametrize("plant,drop_first", [((), False), (("bad", "zero_cv"), False), (("bad",), True)])
def test_twin_equals_central_differences_of_the_price_estimator(recenter, plant, drop_first):
    mu, cv, _ = synthetic(N, 41, plant, drop_first)
    figs = difference_figures(mu, cv, recenter)
    print(f"cmc greeks twin vs central differences recenter={recenter} plant={plant} drop_first={drop_first} "
          + " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    corr = ct.estimator(mu, cv, F0, STRIKES, TYPES, D0, recenter)[2]["corr"]
    assert STRIKES[0] + corr <= 0.0                                    # the K' <= 0 strike is among them
    assert figs["delta"] <= FIRST_BOUND and figs["dual_delta"] <= FIRST_BOUND, figs
    assert figs["gamma"] <= SECOND_BOUND and figs["dual_gamma"] <= SECOND_BOUND, figs


def test_a_twin_with_one_wrong_term_fails_by_orders_of_magnitude():
    mu, cv, _ = synthetic(N, 41, ("bad", "zero_cv"))
    mu = mu + 0.02                                                     # a recentring that is not small: c = 0.02
    good = difference_figures(mu, cv, True)
    assert good["delta"] <= FIRST_BOUND and good["gamma"] <= SECOND_BOUND
    no_c = difference_figures(mu, cv, True, "no_c_bk")
    kp = difference_figures(mu, cv, True, "kp_in_gamma_factor")
    print(f"cmc greeks mutations: delta without c B_k {no_c['delta']:.2e} (bound {FIRST_BOUND:.0e}), gamma with K' in its factor "
          f"{kp['gamma']:.2e} (bound {SECOND_BOUND:.0e})")
    assert no_c["delta"] > 1e3 * FIRST_BOUND and no_c["gamma"] <= SECOND_BOUND
    assert kp["gamma"] > 1e3 * SECOND_BOUND and kp["delta"] <= FIRST_BOUND


@pytest.mark.parametrize("recenter", [True, False])
def test_both_identities_hold_on_the_twin(recenter):
    mu, cv, _ = synthetic(N, 43, ("bad", "zero_cv"))
    g, stats = gt.estimator(mu, cv, 1.3, STRIKES, TYPES, D0, recenter)
    euler = np.abs(g["price"] - (1.3 * g["delta"] + STRIKES * g["dual_delta"])) / 1.3
    homog = np.abs(1.3 ** 2 * g["gamma"] - STRIKES ** 2 * g["dual_gamma"]) / np.maximum(np.abs(STRIKES ** 2 * g["dual_gamma"]), 1e-300)
    print(f"cmc greeks twin identities recenter={recenter} euler {euler.max():.2e} homogeneity {homog.max():.2e}")
    assert euler.max() <= 1e-14 and homog.max() <= 1e-14
    assert stats["n_zero_cv"] == 1 and g["gamma"][0] == 0.0


def test_unsupported_requests_are_refused_before_any_device_work():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import VariableType
    chain = dict(ttms=np.array([0.25]), forwards=np.array([1.0]), discfactors=np.array([1.0]), strikes_ttms=[np.array([1.0])],
                 optiontypes_ttms=[np.array(["C"])], nb_path=64, seed=1)
    lkw = dict(v0=0.2, theta=0.2, kappa1=1.0, kappa2=1.0, beta=-0.3, volvol=0.4, vol_backbone_etas=np.ones(1))
    hkw = dict(v0=0.04, theta=0.04, kappa=4.0, rho=-0.5, volvol=0.4)

    class Two:
        world, rank = 2, 0

    for fn, kw in ((sv.logsv_mc_chain_greeks_conditional, lkw), (sv.heston_mc_chain_greeks_conditional, hkw)):
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
        sv.logsv_mc_chain_greeks_conditional(is_spot_measure=False, **chain, **lkw)
    with pytest.raises(NotImplementedError):
        sv.heston_mc_chain_greeks_conditional(scheme="qe", **chain, **hkw)
    with pytest.raises(ValueError, match="not implemented"):
        sv.compute_mc_vars_greeks_conditional(np.zeros(4), np.ones(4), 1.0, 1.0, np.array([1.0]), np.array(["IC"]))
    option_chain = sv.OptionChain(ttms=chain["ttms"], forwards=chain["forwards"], discfactors=chain["discfactors"],
                                  strikes_ttms=chain["strikes_ttms"], optiontypes_ttms=[np.array(["IC"])], ids=np.array(["a"]))
    with pytest.raises(ValueError, match="not implemented"):
        sv.LogSVPricer().model_mc_chain_greeks_conditional(option_chain, sv.LOGSV_BTC_PARAMS, nb_path=64, seed=1)
    with pytest.raises(ValueError, match="not implemented"):
        sv.HestonPricer().model_mc_chain_greeks_conditional(option_chain, sv.BTC_HESTON_PARAMS, nb_path=64, seed=1)


@pytest.mark.parametrize("recenter", [False, True])
def test_density_composition_integrates_to_the_kept_non_degenerate_share(recenter):
    # total deviation of x at most sqrt(0.02 + 0.08^2) = 0.163: the grid's nearer end is 6.1 deviations out (4e-10 of the mass)
    # and the narrowest path (sd 0.063) spans 12 grid steps, so the trapezoid sum is exact far below the bound
    rng = np.random.default_rng(47)
    cv = rng.uniform(0.004, 0.02, N)
    mu = -0.5 * cv + 0.08 * rng.standard_normal(N)
    mu[5], mu[17], cv[9], cv[23], mu[50], bad = np.nan, np.inf, -1e-3, np.nan, 800.0, 5
    cv[3], cv[100], cv[200] = 0.0, 0.0, 0.0                            # three point masses
    x = np.linspace(-1.5, 1.0, 501)
    pdf, err, stats = gt.log_return_pdf(mu, cv, x, recenter)
    dx = x[1] - x[0]
    integral = dx * (pdf.sum() - 0.5 * (pdf[0] + pdf[-1]))
    share = (stats["n_kept"] - stats["n_zero_cv"]) / stats["n_kept"]
    print(f"cmc greeks density recenter={recenter} integral {integral:.12f} share {share:.12f} difference {integral - share:.2e}")
    assert stats["n_kept"] == N - bad and stats["n_zero_cv"] == 3
    assert abs(integral - share) <= 1e-6
    assert np.all(pdf >= 0.0) and np.all(err >= 0.0)


def test_the_two_new_kernels_use_no_scratch():
    from stochvolmodels_amd import build
    build.build()
    meta = json.load(open(build.ISA_JSON))["metadata"]
    for stem in ("cond_deriv_kernelILi4EE", "cond_deriv_finish_kernelE"):
        hit = [k for k in meta if stem in k]
        assert len(hit) == 1, (stem, sorted(k for k in meta if "cond_deriv" in k))
        assert meta[hit[0]]["scratch_bytes"] == 0, (stem, meta[hit[0]])
    assert len([k for k in meta if "cond_deriv" in k]) == 2
