"""
The Hawkes risk-premia kernel on the GPU against the unmodified reference (tests/golden/hawkes_risk_premia.npz,
make_golden_hawkes_risk_premia.py): the normalizers and gamma forwards (hawkes_risk_forwards_kernel), chain prices and one
slice (mgf_gamma_slice_kernel, both payoff-weight branches), put-call parity, the gamma = 0 limit against the plain Fourier
pricer, the batch against single calls bit for bit, the calibration objective, capped and full calibrations, the batched
against the plain gradient, and the entry points' error codes.
"""
import ctypes as C

import numpy as np
import pytest

import hawkes_twin as twin

pytestmark = pytest.mark.gpu


def _hp():
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    return hp


def _params(vec, gamma=None):
    p = _hp().HawkesJDParams(**dict(zip(twin.PARAM_NAMES, (float(v) for v in vec))))
    p.risk_premia_gamma = gamma
    return p


def _chain(f, first_only=False):
    from stochvolmodels_amd.data.option_chain import OptionChain
    m = 1 if first_only else f["ttms"].size
    return OptionChain(ttms=f["ttms"][:m], forwards=f["forwards"][:m], discfactors=f["discfactors"][:m],
                       strikes_ttms=[f[f"strikes_{i}"] for i in range(m)], optiontypes_ttms=[f[f"types_{i}"] for i in range(m)],
                       bid_ivs=[f[f"bid_{i}"] for i in range(m)], ask_ivs=[f[f"ask_{i}"] for i in range(m)], ids=None)


def _kw(chain):
    return dict(ttms=chain.ttms, forwards=chain.forwards, discfactors=chain.discfactors, strikes_ttms=chain.strikes_ttms,
                optiontypes_ttms=chain.optiontypes_ttms)


def _rel_floor(a, b, scale):
    """the metric of test_gpu_hawkes.py's test_analytic_matches_the_reference: relative, floored at 1e-4 x forward"""
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-4 * scale))


def test_forwards_match_the_reference(golden):
    hp = _hp()
    f = golden("hawkes_risk_premia")
    cases = dict(chain=(f["ttms"], f["forwards0"]), grid=(f["grid_ttms"], f["grid_forwards"]),
                 paper=(f["grid_ttms"], np.array([1.0])))
    for s, vec in enumerate(f["param_sets"]):
        for case, (ttms, fwds) in cases.items():
            for g, gamma in enumerate(f["gammas"]):
                norm, gfwd = hp.hawkesjd_forwards_under_risk_kernel(model_params=_params(vec), risk_premia_gamma=gamma,
                                                                    ttms=ttms, forwards=fwds)
                assert norm.shape == gfwd.shape == ttms.shape
                msg = f"set {s} {case} gamma {gamma}"
                # where the solution blows up before ttm (gamma = 4.8 at the longest ttms), SciPy fails and the reference
                # keeps the last state it reached; our integrator gives up there: NaN, and only there
                failed = f[f"fwd_tight_{s}_{case}_failed"][g]
                np.testing.assert_array_equal(np.isnan(gfwd), failed, err_msg=msg)
                ok = ~failed
                np.testing.assert_allclose(norm[ok], f[f"fwd_tight_{s}_{case}_norm"][g][ok], rtol=1e-9, err_msg=msg)
                np.testing.assert_allclose(gfwd[ok], f[f"fwd_tight_{s}_{case}_gfwd"][g][ok], rtol=1e-9, err_msg=msg)
                np.testing.assert_allclose(gfwd[ok], f[f"fwd_default_{s}_{case}_gfwd"][g][ok], rtol=1e-3, err_msg=msg)
                if case == "paper":                                      # zip truncation: only the first entry
                    assert np.all(norm[1:] == 1.0) and np.all(gfwd[1:] == 1.0)
                if gamma == 0.0:                                         # log E(0) = 0 exactly
                    assert np.all(norm == 1.0)


# gamma = 4.8: the normalizer (0.04-0.7) and K^5.8 amplify the last expiry's ODE error; observed on an MI355X: 4.1e-8
TIGHT_PRICE_TOL = {4.8: 1e-7}


def test_chain_prices_match_the_reference(golden):
    """tight: 1e-8 in the metric of the plain pricer's test (TIGHT_PRICE_TOL where the kernel amplifies the ODE error).
    Default: 2e-3, or the reference's own default-to-tight spread where that is larger (its RK45 at rtol 1e-3 drifts by up to
    0.12 at gamma = 4.8 and 0.055 at gamma = -2 on this chain)"""
    hp = _hp()
    f = golden("hawkes_risk_premia")
    chain = _chain(f)
    scale = np.repeat(chain.forwards, [k.size for k in chain.strikes_ttms])
    bad = []
    for s, vec in enumerate(f["param_sets"]):
        for g, gamma in enumerate(f["gammas"]):
            pr = hp.hawkesjd_chain_pricer_with_risk_premia(model_params=_params(vec, gamma), **_kw(chain))
            assert [p.shape for p in pr] == [k.shape for k in chain.strikes_ttms]
            pr = np.concatenate(pr)
            tight = np.concatenate([f[f"prices_tight_{s}_{g}_{i}"] for i in range(4)])
            default = np.concatenate([f[f"prices_default_{s}_{g}_{i}"] for i in range(4)])
            spread = _rel_floor(tight, default, scale)
            e_tight, e_default = _rel_floor(pr, tight, scale), _rel_floor(pr, default, scale)
            print(f"set {s} gamma {gamma}: vs tight {e_tight:.3g}, vs default {e_default:.3g} (reference spread {spread:.3g})")
            if e_tight > TIGHT_PRICE_TOL.get(float(gamma), 1e-8) or e_default > max(2e-3, 1.05 * spread):
                bad.append((s, float(gamma), e_tight, e_default))
    assert not bad, bad


def test_slice_pricer_both_branches(golden):
    """the reference's slice pricer on one tight log-MGF: the complex weight at gamma = 1, and the real shortcut on the grid of
    real part 0 at gamma = -0.5, where the complex weight would be the same number but not the same bits"""
    from stochvolmodels_amd.utils import mgf_pricer as mgfp
    f = golden("hawkes_risk_premia")
    kw = dict(log_mgf_grid=f["slice_log_mgf"], ttm=float(f["slice_ttm"]), forward=float(f["slice_forward"]),
              normalizer=float(f["slice_normalizer"]), gamma_forward=float(f["slice_gamma_forward"]),
              strikes=f["slice_strikes"], optiontypes=f["slice_types"])
    pr = mgfp.slice_pricer_with_mgf_grid_with_gamma(phi_grid=f["slice_phi"], risk_premia_gamma=float(f["slice_gamma"]), **kw)
    np.testing.assert_allclose(pr, f["slice_prices"], rtol=1e-12, atol=1e-14)
    phi0 = 1j * f["slice_phi"].imag
    assert mgfp.gamma_shortcut(phi0, -0.5)
    short = mgfp.slice_pricer_with_mgf_grid_with_gamma(phi_grid=phi0, risk_premia_gamma=-0.5, **kw)
    np.testing.assert_allclose(short, f["slice_prices_shortcut"], rtol=1e-12, atol=1e-14)


def test_put_call_parity_and_gamma_shortcut_chain(golden):
    hp = _hp()
    f = golden("hawkes_risk_premia")
    chain = _chain(f)
    for gamma in (-0.5, 1.0, 4.8):
        p = _params(f["param_sets"][1], gamma)
        kw = _kw(chain)
        calls = hp.hawkesjd_chain_pricer_with_risk_premia(model_params=p, **{**kw, "optiontypes_ttms": [
            np.full(k.shape, "C") for k in chain.strikes_ttms]}, return_forwards=True)
        puts = hp.hawkesjd_chain_pricer_with_risk_premia(model_params=p, **{**kw, "optiontypes_ttms": [
            np.full(k.shape, "P") for k in chain.strikes_ttms]})
        _, gfwd = calls[1]
        for i, (c, q, k) in enumerate(zip(calls[0], puts, chain.strikes_ttms)):
            np.testing.assert_allclose(c - q, gfwd[i] - k, rtol=0, atol=1e-12 * gfwd[i], err_msg=f"gamma {gamma} expiry {i}")


def test_gamma_zero_is_the_plain_pricer(golden):
    """at gamma = 0 the risk grid is the plain one, the normalizer is 1 and the gamma forward is F exp(Re log E(-1)) = F to
    the ODE tolerance: on a unit-discount chain the two pricers agree to that tolerance"""
    hp = _hp()
    f = golden("hawkes_risk_premia")
    chain = _chain(f)
    assert np.all(chain.discfactors == 1.0)
    for vec in f["param_sets"]:
        risk, (norm, gfwd) = hp.hawkesjd_chain_pricer_with_risk_premia(model_params=_params(vec, 0.0), **_kw(chain),
                                                                       return_forwards=True)
        plain = hp.hawkesjd_chain_pricer(model_params=_params(vec), **_kw(chain))
        assert np.all(norm == 1.0)
        np.testing.assert_allclose(gfwd, chain.forwards, rtol=1e-9)
        np.testing.assert_allclose(np.concatenate(risk), np.concatenate(plain), rtol=0, atol=2e-9)


def _batch_sets(f):
    """(sigma, gamma) sets on different grids, the shortcut set, and one whose kappa_p = 1e9 makes the ODEs so stiff that DOP853
    gives up on every point (test_gpu_hawkes_calibration.py's stiff set)"""
    base = f["param_sets"][1]
    sets = [_params(base, 0.0), _params(base, 2.0), _params(base, -0.5), _params(f["param_sets"][0], 4.8)]
    sets.append(_params(np.where(np.arange(16) == 1, 0.15, base), -2.0))
    sets.append(_params(np.where(np.arange(16) == 1, 1.2, base), 1e-4))
    sets.append(_params(np.where(np.arange(16) == 8, 1e9, base), 1.0))
    return sets


def test_batch_is_bit_identical_to_single_calls(golden):
    hp = _hp()
    f = golden("hawkes_risk_premia")
    chain = _chain(f)
    sets = _batch_sets(f)
    batch, fwds = hp.hawkesjd_chain_pricer_with_risk_premia_batch(params_list=sets, **_kw(chain), return_forwards=True)
    assert len(batch) == len(fwds) == len(sets)
    for s, p in enumerate(sets):
        single, (norm, gfwd) = hp.hawkesjd_chain_pricer_with_risk_premia(model_params=p, **_kw(chain), return_forwards=True)
        np.testing.assert_array_equal(fwds[s][0], norm, err_msg=f"set {s}")
        np.testing.assert_array_equal(fwds[s][1], gfwd, err_msg=f"set {s}")
        for b, a in zip(batch[s], single):
            np.testing.assert_array_equal(b, a, err_msg=f"set {s}")
    # the stiff set gave up: NaN there only
    assert np.isnan(np.concatenate(batch[-1])).all() and np.isnan(fwds[-1][1]).all()
    for s in range(len(sets) - 1):
        assert np.isfinite(np.concatenate(batch[s])).all() and np.isfinite(fwds[s][1]).all()


def test_more_than_16_sets_are_chunked(golden):
    """20 sets: the C ABI chunks them into launches of 16, bit-identical to one set per call"""
    hp = _hp()
    f = golden("hawkes_risk_premia")
    chain = _chain(f)
    sets = [_params(np.where(np.arange(16) == 1, sig, f["param_sets"][1]), gm)
            for sig, gm in zip(np.linspace(0.2, 0.9, 20), np.linspace(-1.5, 3.0, 20))]
    batch, fwds = hp.hawkesjd_chain_pricer_with_risk_premia_batch(params_list=sets, **_kw(chain), return_forwards=True)
    for s in (0, 15, 16, 19):
        single, (norm, gfwd) = hp.hawkesjd_chain_pricer_with_risk_premia(model_params=sets[s], **_kw(chain),
                                                                         return_forwards=True)
        np.testing.assert_array_equal(fwds[s][1], gfwd, err_msg=f"set {s}")
        for b, a in zip(batch[s], single):
            np.testing.assert_array_equal(b, a, err_msg=f"set {s}")


def _objective(f, vega: bool, first_only: bool = False, **kw):
    hp = _hp()
    p0 = _params(f["calib_params0"], 0.0)
    return hp.HawkesJDPricer().risk_premia_calibration_objective(_chain(f, first_only), p0, is_vega_weighted=vega,
                                                                 print_iter=False, **kw), p0


def test_objective_matches_the_reference(golden):
    f = golden("hawkes_risk_premia")
    for vega in (False, True):
        obj, p0 = _objective(f, vega)
        tag = "vega" if vega else "flat"
        np.testing.assert_allclose(obj.weights, f[f"obj_{tag}_weights"], rtol=1e-13)
        got = np.array([obj(x) for x in f["obj_samples"]])
        np.testing.assert_allclose(got, f[f"obj_{tag}_tight"], rtol=1e-8, err_msg=tag)
        # the last sample's unpack is left in params0, as in the reference
        assert p0.sigma == f["obj_samples"][-1][0] and p0.risk_premia_gamma == 8.0 * f["obj_samples"][-1][1]


def _calibrate(f, tag, **kw):
    hp = _hp()
    first = tag.endswith("slice")
    p0 = _params(f["calib_params0"], 0.0)
    pricer = hp.HawkesJDPricer()
    fit = pricer.calibrate_risk_premia_gamma_to_chain(option_chain=_chain(f, first), params0=p0, is_vega_weighted=first,
                                                      maxiter=int(f[f"cal_{tag}_maxiter"]), print_iter=False, disp=False, **kw)
    assert fit is p0
    return fit, pricer.last_calibration


# observed on an MI355X: |x - x_ref| of the capped tight run 1.2e-9.  The fixture has no 4-expiry tight run: the reference's
# tightened solver does not finish its first line search in reasonable time (make_golden_hawkes_risk_premia.py)
TIGHT_X_TOL = 1e-8


def test_capped_tight_calibration_matches_the_reference(golden):
    tag = "tight_slice"
    f = golden("hawkes_risk_premia")
    fit, last = _calibrate(f, tag)
    x_ref = f[f"cal_{tag}_x"]
    print(tag, "x", last["x"].tolist(), "ref", x_ref.tolist(), "diff", np.abs(last["x"] - x_ref).max(),
          "fun", last["objective"], f[f"cal_{tag}_fun"], "status", last["status"], int(f[f"cal_{tag}_status"]))
    np.testing.assert_allclose(last["x"], x_ref, rtol=0, atol=TIGHT_X_TOL)
    assert last["status"] == int(f[f"cal_{tag}_status"]) and last["nit"] == int(f[f"cal_{tag}_nit"])
    assert fit.sigma == last["x"][0] and fit.risk_premia_gamma == 8.0 * last["x"][1]


# observed on an MI355X: our objective at our fit minus our objective at the reference's fit.  default_chain: both runs stop
# at SLSQP's iteration limit (exit mode 9), ours at 1701.81 where the reference's fit, re-priced by us, gives 1694.71: +7.09,
# 0.4 % of the objective.  default_slice: SLSQP stops (exit mode 0) at 5.52121 against 5.51977: +1.43e-3
DEFAULT_MARGIN = {"default_chain": 10.0, "default_slice": 2e-3}


@pytest.mark.parametrize("tag", ["default_chain", "default_slice"])
def test_full_default_calibration_is_no_worse_than_the_reference(golden, tag):
    """our objective at our fit no worse than at the reference's fit plus a recorded margin.  On the 4-expiry chain the
    reference does not converge at ftol 1e-16 (SLSQP's iteration limit, exit mode 9) and neither do we.  On the one-slice run
    the reference's objective, priced by its default-tolerance solver, is noisy enough to keep SLSQP busy for 100 iterations;
    ours is smooth and SLSQP stops earlier, so the exit mode is not compared there"""
    f = golden("hawkes_risk_premia")
    fit, last = _calibrate(f, tag)
    obj, _ = _objective(f, tag.endswith("slice"), tag.endswith("slice"))
    at_ref = obj(f[f"cal_{tag}_x"])
    at_ours = obj(last["x"])
    print(tag, "x", last["x"].tolist(), "ref", f[f"cal_{tag}_x"].tolist(), "obj ours", at_ours, "at ref x", at_ref,
          "diff", at_ours - at_ref,
          "ref fun (its solver)", float(f[f"cal_{tag}_fun"]), "status", last["status"], "n_eval", last["n_eval"],
          "batches", last["n_gradient_batches"])
    if tag == "default_chain":
        assert last["status"] == int(f[f"cal_{tag}_status"]) == 9
    assert at_ours <= at_ref + DEFAULT_MARGIN[tag]


def test_batched_and_plain_gradients_give_the_same_fit(golden):
    f = golden("hawkes_risk_premia")
    _, batched = _calibrate(f, "default_slice")
    _, plain = _calibrate(f, "default_slice", batched_gradient=False)
    assert batched["n_gradient_batches"] > 0 and plain["n_gradient_batches"] == 0
    np.testing.assert_allclose(batched["x"], plain["x"], rtol=0, atol=1e-12)
    assert batched["status"] == plain["status"] and batched["nit"] == plain["nit"]


def test_error_codes():
    from stochvolmodels_amd import _lib
    from stochvolmodels_amd.engine import DeviceBuffer
    hp = _hp()
    L = _lib.load()
    pf, pi = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rows = np.ascontiguousarray(np.stack([hp.params_block(**hp.HawkesJDParams().to_dict())] * 2))
    gam = np.array([0.5, 1.0])
    ttms, fwds = np.array([0.1, 0.2]), np.array([1.0, 1.0])
    buf = DeviceBuffer(64)
    rt, at = hp.ODE_RTOL, hp.ODE_ATOL

    def fw(rows_p=rows.ctypes.data_as(pf), n_sets=2, t=ttms, out=buf.ptr):
        return L.svmc_hawkesjd_risk_forwards_batch(rows_p, gam.ctypes.data_as(pf), n_sets, t.ctypes.data_as(pf),
                                                   fwds.ctypes.data_as(pf), t.size, out, buf.offset(8), rt, at, None)
    try:
        assert fw() == 0 and L.svmc_stream_synchronize(None) == 0
        assert fw(rows_p=None) == 1
        assert fw(out=None) == 1
        assert fw(n_sets=0) == 1
        assert fw(t=np.array([0.1, 0.0])) == 1
        assert fw(t=np.array([-0.1, 0.2])) == 1
        bad = rows.copy()
        bad[1, 3] = 1.5                                                    # mean_p >= 1 in the second set
        assert fw(rows_p=bad.ctypes.data_as(pf)) == 1
        phi = DeviceBuffer(2 * 2 * 501)
        ks, codes, short = np.array([0.9, 1.1]), np.array([0, 1], dtype=np.int32), np.array([0, 0], dtype=np.int32)

        def sl(phi_p=phi.ptr, n_sets=2, c=codes, k=ks):
            return L.svmc_mgf_gamma_slice_batch(phi_p, phi_p, 501, n_sets, gam.ctypes.data_as(pf), short.ctypes.data_as(pi),
                                                buf.ptr, buf.offset(8), 0, 1.0, k.ctypes.data_as(pf), c.ctypes.data_as(pi),
                                                k.size, buf.offset(16), None)
        assert sl(phi_p=None) == 1
        assert sl(n_sets=0) == 1
        assert sl(c=np.array([0, 2], dtype=np.int32)) == 3                # 'IC': SVMC_ERR_UNKNOWN_PAYOFF
        assert sl(k=np.array([0.9, -1.0])) == 1
        phi.free()
    finally:
        buf.free()


def test_strikes_and_expiries_beyond_one_launch_are_chunked(golden):
    """70 strikes (launches of 32) and 40 expiries (launches of 32 lane pairs) equal smaller calls bit for bit"""
    from stochvolmodels_amd.utils import mgf_pricer as mgfp
    hp = _hp()
    f = golden("hawkes_risk_premia")
    kw = dict(log_mgf_grid=f["slice_log_mgf"], phi_grid=f["slice_phi"], risk_premia_gamma=float(f["slice_gamma"]),
              ttm=float(f["slice_ttm"]), forward=float(f["slice_forward"]), normalizer=float(f["slice_normalizer"]),
              gamma_forward=float(f["slice_gamma_forward"]))
    ks = np.linspace(0.5, 1.6, 70)
    types = np.where(np.arange(70) % 3 == 0, "P", "C")
    whole = mgfp.slice_pricer_with_mgf_grid_with_gamma(strikes=ks, optiontypes=types, **kw)
    parts = np.concatenate([mgfp.slice_pricer_with_mgf_grid_with_gamma(strikes=ks[i:i + 7], optiontypes=types[i:i + 7], **kw)
                            for i in range(0, 70, 7)])
    np.testing.assert_array_equal(whole, parts)
    ttms = np.linspace(0.01, 0.4, 40)
    fwds = np.linspace(0.9, 1.2, 40)
    p = _params(f["param_sets"][1])
    norm, gfwd = hp.hawkesjd_forwards_under_risk_kernel(p, 1.5, ttms, fwds)
    for e in (0, 31, 32, 39):
        n1, g1 = hp.hawkesjd_forwards_under_risk_kernel(p, 1.5, ttms[e:e + 1], fwds[e:e + 1])
        assert n1[0] == norm[e] and g1[0] == gfwd[e]
