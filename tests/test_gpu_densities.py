"""
Densities, digital options and histograms on the device against the reference's outputs of
tests/golden/densities.npz (tests/golden/make_golden_densities.py) and against identities that need no reference.

Slice kernels on a GIVEN transform: both sides get the same closed-form log-MGF, so only the inversion is under test.  The two
differ by the rounding of exp / sincos at arguments up to max_j |Im arg_j| and by summation order; the bound of a sum is
    SLICE_C eps (2 + max_j |Im arg_j|) sum_j |term_j|
computed in NumPy from the fixture's inputs (test_densities_host.pdf_terms / digital_terms).  SLICE_C = 4 x the larger of (a) a
NumPy restatement summed in reversed order against the reference, on the CPU, and (b) the device against the fixture; both
observations are in profiles/densities_observed_tolerances.txt and every test prints its own ratio.

logsv_pdfs end to end: the fixture was made with the reference's solve_ivp tightened to rtol 1e-11 / atol 1e-13; the error is
max |device - reference| over the space grid in units of the peak mass, bounded by PDF_TIGHT_BOUND (4 x the largest observed).
"""
import os

import numpy as np
import pytest

from test_densities_host import EPS, SLICE_C, digital_terms, params, pdf_terms

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TTM = 0.25
PDF_TIGHT_BOUND = 1.5e-12     # of the peak mass: 4 x the largest observed (3.72e-13, BTC set, SIGMA, first order)
QVAR_DEFAULT_BOUND = 5e-6      # of the peak mass, for a fixture whose Q_VAR case was solved at the reference's default tolerance
                               # (qvar_is_tight False; the committed fixture's is tight)


def report(name, value, bound):
    print(f"DEVICE-MAX {name}: {value:.4g} (bound {bound:.4g})")
    assert value <= bound, (name, value, bound)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "densities.npz"))


@pytest.fixture(scope="module")
def sv():
    import stochvolmodels_amd
    return stochvolmodels_amd


# ---- 1. slice kernels on a given transform ---------------------------------------------------------------------------------
PDF_CASES = [("pdf", "slice_phi", "slice_log_mgf", dict(), "slice_pdf"),
             ("pdf_trapz", "slice_phi", "slice_log_mgf", dict(is_simpson=False), "slice_pdf_trapz"),
             ("pdf_shift_scale", "slice_phi", "slice_log_mgf", dict(shift=0.03, scale=1.25), "slice_pdf_shift_scale"),
             ("pdf_even", "slice_even_phi", "slice_even_log_mgf", dict(), "slice_even_pdf")]


@pytest.mark.parametrize("name,var_key,lm_key,kw,want_key", PDF_CASES, ids=[c[0] for c in PDF_CASES])
def test_pdf_slice_against_the_reference(sv, fx, name, var_key, lm_key, kw, want_key):
    var, lm, space = fx[var_key], fx[lm_key], fx["slice_space"]
    got = sv.pdf_with_mgf_grid(lm, var, space, **kw)
    _, _, scale = pdf_terms(var, lm, space, **kw)
    report(f"slice ratio {name}", float(np.max(np.abs(got - fx[want_key]) / scale)), SLICE_C)


def test_pdf_slice_drops_nan_terms(sv, fx):
    lm = fx["slice_log_mgf"].copy()
    lm[fx["slice_nan_idx"]] = np.nan + 1j * np.nan
    got = sv.pdf_with_mgf_grid(lm, fx["slice_phi"], fx["slice_space"])
    assert np.all(np.isfinite(got))
    _, _, scale = pdf_terms(fx["slice_phi"], lm, fx["slice_space"])
    report("slice ratio pdf_nan", float(np.max(np.abs(got - fx["slice_nan_pdf"]) / scale)), SLICE_C)
    prices = sv.digital_slice_pricer_with_mgf_grid(lm, fx["slice_phi"], float(fx["slice_forward"]), fx["slice_dig_strikes"],
                                                   np.full(4, "C"), float(fx["slice_discfactor"]))
    _, dscale, _ = digital_terms(fx["slice_phi"], lm, float(fx["slice_forward"]), fx["slice_dig_strikes"])
    report("slice ratio dig_nan", float(np.max(np.abs(prices - fx["slice_nan_dig_calls"]) / (float(fx["slice_discfactor"]) * dscale))),
           SLICE_C)


def test_pdf_identities_need_no_reference(sv, fx):
    """the reference's own bounds (tests/test_mgf_pricer_identities.py:168-181)"""
    space = fx["slice_space"]
    m = sv.pdf_with_mgf_grid(fx["slice_log_mgf"], fx["slice_phi"], space)
    variance = 0.3 * 0.3 * 0.5
    assert np.min(m) >= -1e-10
    report("mass", abs(float(np.sum(m)) - 1.0), 2e-8)
    report("mean", abs(float(np.sum(space * m)) + 0.5 * variance), 2e-8)
    report("martingale", abs(float(np.sum(np.exp(space) * m)) - 1.0), 3e-8)


def test_digitals_against_the_reference_both_contours(sv, fx):
    f, df, k4 = float(fx["slice_forward"]), float(fx["slice_discfactor"]), fx["slice_dig_strikes"]
    phi, lm = fx["slice_phi"], fx["slice_log_mgf"]
    _, scale, calls = digital_terms(phi, lm, f, k4)
    assert calls
    for name, types, want, kw in (("calls", np.full(4, "C"), fx["slice_dig_calls"], {}),
                                  ("puts", np.full(4, "P"), fx["slice_dig_puts"], {}),
                                  ("calls_trapz", np.full(4, "C"), fx["slice_dig_calls_trapz"], dict(is_simpson=False))):
        sc = digital_terms(phi, lm, f, k4, **kw)[1] if kw else scale
        got = sv.digital_slice_pricer_with_mgf_grid(lm, phi, f, k4, types, df, **kw)
        report(f"slice ratio dig_{name}", float(np.max(np.abs(got - want) / (df * sc))), SLICE_C)
    _, escale, _ = digital_terms(fx["slice_even_phi"], fx["slice_even_log_mgf"], f, k4)
    got = sv.digital_slice_pricer_with_mgf_grid(fx["slice_even_log_mgf"], fx["slice_even_phi"], f, k4, np.full(4, "C"), df)
    report("slice ratio dig_even", float(np.max(np.abs(got - fx["slice_even_dig_calls"]) / (df * escale))), SLICE_C)
    # positive contour: the sums are digital puts, calls are the complement
    php, lmp, k3, t3 = fx["slice_pos_phi"], fx["slice_pos_log_mgf"], fx["slice_pos_strikes"], fx["slice_pos_types"]
    _, pscale, pcalls = digital_terms(php, lmp, f, k3)
    assert not pcalls
    got = sv.digital_slice_pricer_with_mgf_grid(lmp, php, f, k3, t3, df)
    report("slice ratio dig_pos", float(np.max(np.abs(got - fx["slice_pos_digitals"]) / (df * pscale))), SLICE_C)


def test_digital_identities_need_no_reference(sv, fx):
    f, df, k4 = float(fx["slice_forward"]), float(fx["slice_discfactor"]), fx["slice_dig_strikes"]
    phi, lm = fx["slice_phi"], fx["slice_log_mgf"]
    calls = sv.digital_slice_pricer_with_mgf_grid(lm, phi, f, k4, np.full(4, "C"), df)
    puts = sv.digital_slice_pricer_with_mgf_grid(lm, phi, f, k4, np.full(4, "P"), df)
    report("call + put digital - discount factor", float(np.max(np.abs(calls + puts - df))), 4 * EPS)
    from stochvolmodels_amd.utils.mgf_pricer import vanilla_slice_pricer_with_mgf_grid
    bump = 1.0e-5
    up = vanilla_slice_pricer_with_mgf_grid(lm, phi, f, k4 + bump, np.full(4, "C"), df)
    dn = vanilla_slice_pricer_with_mgf_grid(lm, phi, f, k4 - bump, np.full(4, "C"), df)
    report("digital call + dC/dK", float(np.max(np.abs(calls + (up - dn) / (2.0 * bump)))), 2e-7)


def test_digital_pricer_refuses_strikes_and_forwards_without_a_logarithm(sv, fx):
    phi, lm = fx["slice_phi"], fx["slice_log_mgf"]
    for forward, strikes in ((1.2, [1.0, 0.0]), (1.2, [-1.0]), (0.0, [1.0]), (1.2, [np.nan]), (np.inf, [1.0])):
        with pytest.raises(ValueError):
            sv.digital_slice_pricer_with_mgf_grid(lm, phi, forward, np.array(strikes), np.full(len(strikes), "C"))


def test_batch_of_three_sets_is_bit_equal_to_three_single_calls(sv, fx):
    from stochvolmodels_amd.analytic import digital_slice_sums, pdf_slices
    phi, space, vols = fx["slice_phi"], fx["slice_space"], fx["slice_batch_vols"]
    lms = np.stack([0.5 * (v * v * 0.5) * (phi + phi * phi) for v in vols])
    spaces = np.stack([space, space + 0.01, 1.1 * space])
    shifts, scales = [0.0, 0.02, -0.01], [1.0, 1.25, 0.9]
    batch = pdf_slices(np.stack([phi] * 3), lms, spaces, shifts, scales)
    for s in range(3):
        single = sv.pdf_with_mgf_grid(lms[s], phi, spaces[s], shift=shifts[s], scale=scales[s])
        assert np.array_equal(batch[s], single)
    _, _, scale = pdf_terms(phi, lms[0], space)
    report("slice ratio pdf_batch", float(np.max(np.abs(batch[0] - fx["slice_batch_pdf"][0]) / scale)), SLICE_C)
    k = np.linspace(0.7, 1.6, 37)                             # two launches of 32 strikes
    dbatch = digital_slice_sums(np.stack([phi] * 3), lms, 1.2, k, True)
    for s in range(3):
        assert np.array_equal(dbatch[s], digital_slice_sums(phi[None, :], lms[s][None, :], 1.2, k, True)[0])


def test_heston_log_mgf_density_and_digitals(sv, fx):
    """any model's log-MGF: the reference's closed-form Heston transform, and the device's own"""
    hphi, hlm, space = fx["heston_phi"], fx["heston_log_mgf"], fx["heston_space"]
    _, _, scale = pdf_terms(hphi, hlm, space)
    got = sv.pdf_with_mgf_grid(hlm, hphi, space)
    report("slice ratio heston_pdf", float(np.max(np.abs(got - fx["heston_pdf"]) / scale)), SLICE_C)
    _, dscale, _ = digital_terms(hphi, hlm, 1.0, fx["heston_dig_strikes"])
    dig = sv.digital_slice_pricer_with_mgf_grid(hlm, hphi, 1.0, fx["heston_dig_strikes"], np.full(3, "C"))
    report("slice ratio heston_dig", float(np.max(np.abs(dig - fx["heston_dig_calls"]) / dscale)), SLICE_C)
    v0, theta, kappa, rho, volvol = (float(v) for v in fx["heston_params"])
    dlm = sv.compute_heston_mgf_grid(v0=v0, theta=theta, kappa=kappa, volvol=volvol, rho=rho, ttm=float(fx["heston_ttm"]),
                                     phi_grid=hphi, psi_grid=np.zeros_like(hphi))[0]
    # the device's closed form differs from the reference's by rounding of csqrt / clog / cexp (each <= 5e-16 relative,
    # tests/test_gpu_device_math.py) on a log-MGF of modulus up to ~1e2: ~1e-13 of a term, two orders under this bound
    own = sv.pdf_with_mgf_grid(dlm, hphi, space)
    report("heston density, device transform", float(np.max(np.abs(own - fx["heston_pdf"])) / fx["heston_pdf"].max()), 1e-11)


# ---- 2. logsv_pdfs end to end ----------------------------------------------------------------------------------------------
def _pdf_cases():
    out = []
    for tag in ("test", "btc"):
        for order in (1, 2):
            out.append((tag, "sigma", order, True))
            for spot in (True, False):
                out.append((tag, "x", order, spot))
    return out


def _vt(sv, name):
    return {"x": sv.VariableType.LOG_RETURN, "qvar": sv.VariableType.Q_VAR, "sigma": sv.VariableType.SIGMA}[name]


def _order(sv, order):
    return sv.ExpansionOrder.FIRST if order == 1 else sv.ExpansionOrder.SECOND


@pytest.mark.parametrize("tag,vname,order,spot", _pdf_cases(), ids=lambda v: str(v))
def test_logsv_pdfs_against_the_tightened_reference(sv, fx, tag, vname, order, spot):
    p = params(fx, tag)
    space = p.get_variable_space_grid(variable_type=_vt(sv, vname), ttm=TTM, n=200, n_stdevs=4.5)
    assert np.array_equal(space, fx[f"space_{tag}_{vname}"])
    got = sv.LogSVPricer().logsv_pdfs(params=p, ttm=TTM, space_grid=space, is_spot_measure=spot, expansion_order=_order(sv, order),
                                      variable_type=_vt(sv, vname))
    want = fx[f"pdf_{tag}_{vname}_{order}_{'spot' if spot else 'inv'}"]
    from stochvolmodels_amd.pricers import logsv_pricer
    assert logsv_pricer.LAST_ANALYTIC_GIVEN_UP == 0
    report(f"logsv_pdfs {tag} {vname} order {order} {'spot' if spot else 'inv'} / peak", float(np.max(np.abs(got - want)) / want.max()),
           PDF_TIGHT_BOUND)


def test_logsv_pdfs_qvar(sv, fx):
    """the 40 000-point psi grid: the inversion alone on the reference's own log-MGF, then end to end"""
    p = params(fx, "test")
    space = fx["space_test_qvar"]
    want = fx["pdf_test_qvar_2_spot"]
    from stochvolmodels_amd.utils.mgf_pricer import get_psi_grid
    psi = get_psi_grid()
    inv = sv.pdf_with_mgf_grid(fx["qvar_log_mgf"], psi, space, shift=0.0, scale=1.0 / TTM) / (1.0 / TTM)
    _, _, scale = pdf_terms(psi, fx["qvar_log_mgf"], space, scale=1.0 / TTM)
    report("slice ratio qvar 40000", float(np.max(np.abs(inv - want) / (scale * TTM))), SLICE_C)
    got = sv.logsv_pdfs(params=p, ttm=TTM, space_grid=space, variable_type=sv.VariableType.Q_VAR)
    tight = bool(fx["qvar_is_tight"])
    report(f"logsv_pdfs test qvar order 2 / peak (reference {'tight' if tight else 'default tolerance'})",
           float(np.max(np.abs(got - want)) / want.max()), PDF_TIGHT_BOUND if tight else QVAR_DEFAULT_BOUND)


def test_logsv_pdfs_batch_is_bit_equal_to_single_calls(sv, fx):
    pt, pb = params(fx, "test"), params(fx, "btc")
    for vname in ("x", "sigma"):
        vt = _vt(sv, vname)
        plist = [pt, pb, pt, pb]
        orders = [sv.ExpansionOrder.FIRST, sv.ExpansionOrder.FIRST, sv.ExpansionOrder.SECOND, sv.ExpansionOrder.SECOND]
        spaces = [fx[f"space_{t}_{vname}"] for t in ("test", "btc", "test", "btc")]
        batch = sv.logsv_pdfs_batch(plist, TTM, spaces, expansion_orders=orders, variable_type=vt)
        for p, o, s, b in zip(plist, orders, spaces, batch):
            assert np.array_equal(b, sv.logsv_pdfs(params=p, ttm=TTM, space_grid=s, expansion_order=o, variable_type=vt))


def test_integrator_flags_are_accepted(sv, fx):
    p = params(fx, "test")
    space = fx["space_test_x"]
    base = sv.logsv_pdfs(params=p, ttm=TTM, space_grid=space)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert np.array_equal(base, sv.logsv_pdfs(params=p, ttm=TTM, space_grid=space, is_stiff_solver=True, is_analytic=True))


# ---- 3. histogram ----------------------------------------------------------------------------------------------------------
def test_histogram_equals_numpy_on_simulated_states(sv, fx):
    from stochvolmodels_amd.analytic import device_histograms, histogram_edges
    from stochvolmodels_amd.engine import get_engine
    p = params(fx, "test")
    n = 100_000
    x, vol, q = sv.LogSVPricer().simulate_terminal_values(params=p, ttm=TTM, nb_path=n, seed=77)
    eng = get_engine(n)
    grids = [fx["space_test_x"], fx["space_test_sigma"], fx["space_test_qvar"]]
    edges = [histogram_edges(g[0], g[-1], g.size - 1) for g in grids]
    counts = device_histograms([eng.x.ptr, eng.vol.ptr, eng.qvar.ptr], n, edges, [1.0, 1.0, TTM])
    for name, data, g, c in zip(("x", "sigma", "qvar / ttm"), (x, vol, q / TTM), grids, counts):
        want = np.histogram(data, bins=g.size - 1, range=(g[0], g[-1]))[0]
        assert c.dtype == np.int64 and np.array_equal(c, want), name
        print(f"DEVICE histogram {name}: {int(c.sum())} of {n} inside the grid, equal to np.histogram")
    # a narrow range: most values fall outside and are dropped
    e = histogram_edges(-0.05, 0.02, 13)
    c = device_histograms([eng.x.ptr], n, [e], [1.0])[0]
    assert np.array_equal(c, np.histogram(x, bins=13, range=(-0.05, 0.02))[0])


def test_histogram_edge_cases_equal_numpy(sv):
    from stochvolmodels_amd.analytic import device_histograms, histogram_edges
    from stochvolmodels_amd.engine import DeviceBuffer
    from stochvolmodels_amd import _lib
    L = _lib.load()
    for lo, hi, n_bins in ((-0.3, 0.9, 199), (0.0, 0.37, 7), (0.1, 1.3, 8192), (1e-3, 1e-3 + 1e-9, 50)):
        e = histogram_edges(lo, hi, n_bins)
        sub = e if e.size <= 400 else e[:: e.size // 397]
        v = np.concatenate([sub, np.nextafter(sub, -np.inf), np.nextafter(sub, np.inf), [lo, hi, np.nextafter(lo, -np.inf),
                            np.nextafter(hi, np.inf), np.nan, np.inf, -np.inf, 0.5 * (lo + hi)],
                            np.random.default_rng(3).uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), 5000)])
        for div in (1.0, 0.3):
            data = np.ascontiguousarray(v * div)              # the kernel divides by `div` again: the test data is (v div) / div
            buf = DeviceBuffer(data.size)
            try:
                _lib.check(L.svmc_memcpy_h2d(buf.ptr, data.ctypes.data, data.nbytes, None))
                _lib.check(L.svmc_stream_synchronize(None))
                c = device_histograms([buf.ptr], data.size, [e], [div])[0]
            finally:
                buf.free()
            with np.errstate(invalid="ignore"):
                want = np.histogram(data / div, bins=n_bins, range=(lo, hi))[0]
            assert np.array_equal(c, want), (lo, hi, n_bins, div)
    with pytest.raises(ValueError):
        device_histograms([0], 0, [histogram_edges(0.0, 1.0, 8193)], [1.0])


def test_terminal_value_histograms_equal_compute_histogram_data(sv, fx):
    p = params(fx, "test")
    pricer = sv.LogSVPricer()
    hists = pricer.terminal_value_histograms(params=p, ttm=TTM, nb_path=100_000, seed=77, n=200, n_stdevs=4.5)
    x, vol, q = pricer.simulate_terminal_values(params=p, ttm=TTM, nb_path=100_000, seed=77)
    for vt, data in ((sv.VariableType.LOG_RETURN, x), (sv.VariableType.Q_VAR, q / TTM), (sv.VariableType.SIGMA, vol)):
        grid = p.get_variable_space_grid(variable_type=vt, ttm=TTM, n=200, n_stdevs=4.5)
        want = sv.compute_histogram_data(data=data, x_grid=grid)
        got = hists[vt]
        assert np.array_equal(got.index.to_numpy(), want.index.to_numpy()) and np.array_equal(got.to_numpy(), want.to_numpy())
        assert got.iloc[0] == grid[0] / 100_000               # the reference's quirk, kept
    h = sv.HestonParams(v0=0.04, theta=0.05, kappa=3.0, rho=-0.6, volvol=0.5)
    grids = {sv.VariableType.LOG_RETURN: np.linspace(-0.6, 0.4, 101), sv.VariableType.Q_VAR: np.linspace(0.0, 0.2, 81),
             sv.VariableType.SIGMA: np.linspace(0.0, 0.25, 61)}
    hp = sv.HestonPricer()
    hh = hp.terminal_value_histograms(params=h, space_grids=grids, ttm=0.5, nb_path=50_000, seed=5)
    x, var, q = hp.simulate_terminal_values(params=h, ttm=0.5, nb_path=50_000, seed=5)
    for vt, data in ((sv.VariableType.LOG_RETURN, x), (sv.VariableType.Q_VAR, q / 0.5), (sv.VariableType.SIGMA, var)):
        want = sv.compute_histogram_data(data=data, x_grid=grids[vt])
        assert np.array_equal(hh[vt].to_numpy(), want.to_numpy())


# ---- 4. the figure's claim -------------------------------------------------------------------------------------------------
def test_second_order_density_against_400000_paths(sv, fx):
    """|z_gpu - z_ref| <= 0.05 per bin: z the second-order mass of a bin minus the Monte Carlo frequency in units of the binomial
    standard error sqrt(p (1 - p) / n), p the reference's mass; z_ref from the reference's masses and the CPU twin's histogram
    on the same random stream.  The mass of the bin [x_(i-1), x_i] is the mean of the masses at its edges.  Bins expected to
    hold fewer than 5 paths under the reference's masses are left out -- at most 5 % of them, a condition the fixture's
    generator holds its grids to: the figure's grids narrowed to the span of the bins that are expected to hold 5 paths, 200
    points again (the figure's own leave 27 % of the log-return's bins and 67 % of the volatility's short of that)."""
    p = params(fx, "test")
    n = int(fx["fig_paths"])
    assert n == 400_000
    pricer = sv.LogSVPricer()
    names = ("x", "sigma", "qvar")
    hists = pricer.terminal_value_histograms(params=p, ttm=TTM, nb_path=n, seed=int(fx["fig_seed"]),
                                             space_grids={_vt(sv, v): fx[f"fig_{v}_space"] for v in names})
    for vname in names:
        vt = _vt(sv, vname)
        space = fx[f"fig_{vname}_space"]
        assert space.size == 200
        keep, z_ref = fx[f"fig_{vname}_keep"], fx[f"fig_{vname}_z_ref"]
        assert np.count_nonzero(~keep) <= 0.05 * keep.size
        ref = fx[f"fig_{vname}_mass"]
        pb_ref = 0.5 * (ref[:-1] + ref[1:])
        assert np.array_equal(keep, n * pb_ref >= 5.0)
        m = pricer.logsv_pdfs(params=p, ttm=TTM, space_grid=space, variable_type=vt)
        pb = 0.5 * (m[:-1] + m[1:])
        freq = hists[vt].to_numpy()[1:]
        se = np.sqrt(pb_ref[keep] * (1.0 - pb_ref[keep]) / n)
        z = (pb[keep] - freq[keep]) / se
        print(f"DEVICE figure {vname}: max |z| {np.abs(z).max():.2f}, L1(mass, frequency) {np.abs(pb - freq).sum():.4f}, "
              f"{int(np.count_nonzero(freq * n != fx[f'fig_{vname}_hist'][1:] * n))} bins differ from the CPU twin's histogram")
        report(f"figure {vname} max |z_gpu - z_ref|", float(np.max(np.abs(z - z_ref[keep]))), 0.05)
