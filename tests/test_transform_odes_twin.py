"""
The CPU twin's LogSV coefficient ODE (oracle.logsv_mgf_grid: Dormand-Prince 5(4) at rtol 1e-10 / atol 1e-12, the
pricers' tolerance) against the high-precision solutions of tests/golden/transform_odes.npz -- no GPU.  It anchors the
fixture and the twin on machines without one: the GPU tests hold the device kernels to the same fixture.
"""
import numpy as np

# measured worst 2.4e-10 of max(1, |mp|) (kappa2_zero, order 1, spot, 1 year), x 4 headroom; under the GPU tests' ceiling of
# 1e-8, so that a wrong term of relative weight 1e-7 fails
TWIN_BOUND = 1e-9


def test_fixture_agreement(golden):
    fx = golden("transform_odes")
    assert np.all(np.isfinite(fx["logsv_agree"])) and np.max(fx["logsv_agree"]) <= 1e-18
    assert np.all(np.isfinite(fx["chain_agree"])) and np.max(fx["chain_agree"]) <= 1e-18
    assert np.all(np.isfinite(fx["logsv_A"])) and np.all(np.isfinite(fx["logsv_log_mgf"]))
    # at first order components 3 and 4 are not part of the system
    assert np.all(fx["logsv_A"][:, :, 0, ..., 3:] == 0)


def _err(a, lm, A_mp, lm_mp):
    nc = a.shape[-1]
    e = np.abs(a - A_mp[:, :nc]) / np.maximum(1.0, np.abs(A_mp[:, :nc]))
    return max(float(e.max()), float((np.abs(lm - lm_mp) / np.maximum(1.0, np.abs(lm_mp))).max()))


def test_twin_logsv_mgf_grid_vs_fixture(golden, oracle):
    fx = golden("transform_odes")
    worst = 0.0
    for s, params in enumerate(fx["logsv_params"]):
        for m in range(2):
            phi, psi = fx["logsv_phi"][s, m], fx["logsv_psi"][s, m]
            for o in range(2):
                for t, ttm in enumerate(fx["logsv_ttms"]):
                    a, lm = oracle.logsv_mgf_grid(phi, psi, float(ttm), *params, is_spot_measure=(m == 0), expansion_order=o + 1)
                    worst = max(worst, _err(a, lm, fx["logsv_A"][s, m, o, t], fx["logsv_log_mgf"][s, m, o, t]))
    # the chained pair: the second slice starts from the first's A at its own vol_backbone_eta
    s = int(fx["chain_set"])
    (t0, t1), (e0, e1) = fx["chain_ttms"], fx["chain_etas"]
    for m in range(2):
        phi, psi = fx["logsv_phi"][s, m], fx["logsv_psi"][s, m]
        a0, _ = oracle.logsv_mgf_grid(phi, psi, float(t0), *fx["logsv_params"][s], is_spot_measure=(m == 0), vol_backbone_eta=e0)
        a1, lm1 = oracle.logsv_mgf_grid(phi, psi, float(t1 - t0), *fx["logsv_params"][s], a_t0=a0, is_spot_measure=(m == 0),
                                        vol_backbone_eta=e1)
        worst = max(worst, _err(a0, np.zeros(phi.size), fx["chain_A_first"][m], np.zeros(phi.size)),
                    _err(a1, lm1, fx["chain_A"][m], fx["chain_log_mgf"][m]))
    print(f"CPU twin vs mp: {worst:.4g} (bound {TWIN_BOUND:.4g})")
    assert worst <= TWIN_BOUND, worst
