"""
The Hawkes calibration's host side against the unmodified reference (tests/golden/hawkes_calibration.npz,
make_golden_hawkes_calibration.py): the codec helpers of stochvolmodels_amd.pricers.hawkes_jd_pricer (start vector, bounds,
unpacked parameter sets, constraint) and the objective's vega weights.  No GPU.
"""
import numpy as np

import hawkes_twin as twin


def _chain(f):
    from stochvolmodels_amd.data.option_chain import OptionChain
    m = f["ttms"].size
    return OptionChain(ttms=f["ttms"], forwards=f["forwards"], discfactors=f["discfactors"],
                       strikes_ttms=[f[f"strikes_{i}"] for i in range(m)], optiontypes_ttms=[f[f"types_{i}"] for i in range(m)],
                       bid_ivs=[f[f"bid_{i}"] for i in range(m)], ask_ivs=[f[f"ask_{i}"] for i in range(m)], ids=None)


def _params0(f):
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    return hp.HawkesJDParams(**dict(zip(twin.PARAM_NAMES, (float(v) for v in f["params0"]))))


def _vec(p):
    return np.array([getattr(p, k) for k in twin.PARAM_NAMES])


def test_codec_reproduces_the_reference(golden):
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    f = golden("hawkes_calibration")
    params0 = _params0(f)
    np.testing.assert_array_equal(_vec(hp.HawkesJDParams()), f["params0"])      # the paper script's params0
    np.testing.assert_array_equal(hp.calibration_start_vector(params0), f["x0"])
    np.testing.assert_array_equal(np.asarray(hp.CALIBRATION_BOUNDS), f["bounds"])
    np.testing.assert_array_equal(f["samples"][0], f["x0"])
    for pars, ref, cond in zip(f["samples"], f["sample_params"], f["sample_conds"]):
        fit = hp.unpack_calibration_vector(pars, params0)
        assert isinstance(fit, hp.HawkesJDParams) and fit.risk_premia_gamma is None
        np.testing.assert_array_equal(_vec(fit), ref)
        assert hp.calibration_constraint(pars, params0) == cond
    # the fitted vectors of both reference runs unpack to the reference's fits
    for tag in ("default", "tight"):
        np.testing.assert_array_equal(_vec(hp.unpack_calibration_vector(f[f"{tag}_x"], params0)), f[f"{tag}_params"])


def test_vega_weights_match_the_reference(golden):
    from stochvolmodels_amd.utils.calibration import chain_calibration_weights
    from stochvolmodels_amd.utils.funcs import to_flat_np_array
    f = golden("hawkes_calibration")
    chain = _chain(f)
    market_vols = to_flat_np_array(chain.get_chain_data_as_xy()[1])
    np.testing.assert_array_equal(market_vols, f["market_vols"])
    weights = chain_calibration_weights(chain, market_vols, True, False)
    assert weights.shape == f["weights"].shape == (49,)
    np.testing.assert_allclose(weights, f["weights"], rtol=0, atol=1e-14)
