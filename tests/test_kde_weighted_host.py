"""
Host side of the weighted kernel density estimates, no GPU: what device_kdes_weighted sends to the library --
the nullable weights and tilt pointers among it -- and how it reads the answer, against test_kde_host's stand-in for libsvmc;
the gamma axis of engine_state_kdes and of the pricers' methods; the two exceptions from a fabricated stats block; the routing
of risk_premia_gamma=None to the unweighted function; the refusal of sharded requests; the header's declarations.
"""
import os
import re
import types

import numpy as np
import pytest

from stochvolmodels_amd import _lib, analytic
from stochvolmodels_amd.pricers import logsv_pricer as lp
from test_kde_host import StubLib, fake_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# n_kept, n_nan, n_low, n_high, n_bad_weight, sum_w, neff, mean, var, h, factor, sum_w2
GOOD = [100.0, 0.0, 0.0, 0.0, 3.0, 55.5, 80.25, -0.05, 0.09, 0.12, 0.4, 38.4]


class WeightedStubLib(StubLib):
    def __getattr__(self, name):
        call = super().__getattr__(name)
        if name != "svmc_kde_weighted_workspace_bytes":
            return call

        def sized(*args):
            call(*args)
            args[1]._obj.value, args[2]._obj.value = 8192, 2048
            return 0
        return sized


@pytest.fixture
def stub():
    lib = WeightedStubLib()
    with pytest.MonkeyPatch.context() as m:
        m.setattr(_lib, "load", lambda: lib)
        yield lib


def header():
    return open(os.path.join(ROOT, "include", "svmc.h")).read()


def test_stats_fields_are_the_headers():
    text = header()
    assert int(re.search(r"#define SVMC_KDE_WEIGHTED_STATS_DOUBLES (\d+)", text).group(1)) == analytic.KDE_WEIGHTED_STATS_DOUBLES
    assert len(analytic.KDE_WEIGHTED_STATS_FIELDS) == analytic.KDE_WEIGHTED_STATS_DOUBLES
    listed = re.search(r"\[SVMC_KDE_WEIGHTED_STATS_DOUBLES\] =\s*\*?\s*\{([^}]*)\}", text).group(1)
    assert tuple(f.strip(" *\n") for f in listed.split(",")) == analytic.KDE_WEIGHTED_STATS_FIELDS
    assert analytic.KDE_WEIGHTED_STATS_FIELDS[:4] == analytic.KDE_STATS_FIELDS[:4]


def test_header_declares_the_new_symbols_and_the_binding_covers_them():
    text = header()
    for name in ("svmc_kde_weighted_workspace_bytes", "svmc_kde_gaussian_weighted"):
        assert re.search(r"SVMC_API\s+int\s+" + name + r"\s*\(", text), name
    assert re.search(r"svmc_kde_gaussian_weighted\(const double \*values, const double \*weights, const double \*tilt, double gamma,\s*"
                     r"size_t n,\s*double divisor, double limit, const double \*points, int n_points,\s*double bandwidth_factor, "
                     r"double \*density, double \*stats, void \*workspace,\s*size_t workspace_bytes, svmc_stream_t stream\)", text)
    assert "gamma must be finite" in open(os.path.join(ROOT, "stochvolmodels_amd", "csrc", "svmc_density.hip")).read()
    source = open(os.path.join(ROOT, "stochvolmodels_amd", "_lib.py")).read()
    assert '"svmc_kde_weighted_workspace_bytes"' in source and '"svmc_kde_gaussian_weighted"' in source


def test_device_kdes_weighted_marshals_nullable_pointers(stub):
    grids = [np.linspace(0.0, 1.0, 5), np.linspace(-1.0, 1.0, 201), np.array([0.25, 0.5, 0.75]), np.array([1.0, 2.0])]
    densities = [np.arange(5) + 0.5, np.arange(201) * 2.0, np.array([7.0, 8.0, 9.0]), np.array([1.5, 2.5])]
    blocks = [GOOD, [50.0, 1.0, 2.0, 3.0, 4.0, 20.0, 30.0, 0.1, 0.2, 0.3, 0.5, 13.0], GOOD, GOOD]
    stub.answer = np.concatenate(densities + blocks)
    out = analytic.device_kdes_weighted([111, 222, 333, 444], 1000, grids, [1.0, 0.25, 1.0, 1.0], weight_ptrs=[None, 555, 666, None],
                                        tilt_ptrs=[777, None, 888, None], gammas=[-1.0, 0.0, 4.45, 2.0], stream=77)
    names = stub.names()
    assert names.count("svmc_memcpy_h2d") == 1 and names.count("svmc_memcpy_d2h") == 1 and names.count("svmc_stream_synchronize") == 1
    assert names.count("svmc_kde_gaussian_weighted") == 4 and names.count("svmc_kde_gaussian") == 0
    assert names.count("svmc_kde_weighted_workspace_bytes") == 1 and names.count("svmc_kde_workspace_bytes") == 0
    assert names.count("svmc_malloc") == names.count("svmc_free") == 3
    up = next(c for c in stub.calls if c[0] == "svmc_memcpy_h2d")
    grid_buf = up[1]
    assert up[3] == 8 * 211 and up[4] == 77
    down = next(c for c in stub.calls if c[0] == "svmc_memcpy_d2h")
    res_buf = down[2]
    assert down[3] == 8 * (211 + 4 * 12) and down[4] == 77
    launches = [c for c in stub.calls if c[0] == "svmc_kde_gaussian_weighted"]
    assert max(i for i, c in enumerate(names) if c == "svmc_kde_gaussian_weighted") < names.index("svmc_memcpy_d2h")
    offs = [0, 5, 206, 209]
    for i, c in enumerate(launches):
        _, ptr, w, t, gamma, n, div, limit, points, m, factor, density, stats, ws, ws_bytes, stream = c
        assert (ptr, n, div, limit, m, factor, stream) == ((111, 222, 333, 444)[i], 1000, (1.0, 0.25, 1.0, 1.0)[i], 1e16,
                                                           (5, 201, 3, 2)[i], 0.0, 77)
        assert w == (None, 555, 666, None)[i] and t == (777, None, 888, None)[i]        # None reaches ctypes as a NULL pointer
        assert gamma == (-1.0, 0.0, 4.45, 2.0)[i] and isinstance(gamma, float)
        assert points == grid_buf + 8 * offs[i] and density == res_buf + 8 * offs[i]
        assert stats == res_buf + 8 * (211 + 12 * i)
        assert ws == launches[0][13] and ws_bytes == 8192
    for (d, s), want, block in zip(out, densities, blocks):
        assert np.array_equal(d, want)
        assert [s[k] for k in analytic.KDE_WEIGHTED_STATS_FIELDS] == block
        assert all(isinstance(s[k], int) for k in ("n_kept", "n_nan", "n_low", "n_high", "n_bad_weight"))
        assert isinstance(s["neff"], float) and isinstance(s["sum_w"], float)
    # the defaults: no weights, no tilt, gamma 0, the default stream; a given limit and factor
    stub.calls.clear()
    stub.answer = np.concatenate([np.zeros(5), GOOD])
    analytic.device_kdes_weighted([111], 10, [grids[0]], [1.0], limit=5.0, bandwidth_factor=0.3)
    c = next(c for c in stub.calls if c[0] == "svmc_kde_gaussian_weighted")
    assert c[2] is None and c[3] is None and c[4] == 0.0 and c[7] == 5.0 and c[10] == 0.3 and c[15] is None
    with pytest.raises(ValueError, match="per vector"):
        analytic.device_kdes_weighted([111], 10, [grids[0]], [1.0], tilt_ptrs=[1, 2], gammas=[1.0])


@pytest.mark.parametrize("n_kept", [0.0, 1.0])
def test_too_few_kept_samples_raise_value_error(stub, n_kept):
    stub.answer = np.concatenate([np.full(4, np.nan), [n_kept, 3.0, 0.0, 0.0, 0.0, n_kept, n_kept, np.nan, np.nan, np.nan, 1.0, n_kept]])
    with pytest.raises(ValueError):
        analytic.device_kdes_weighted([111], 4, [np.zeros(4)], [1.0], tilt_ptrs=[222], gammas=[1.0])
    assert stub.names().count("svmc_free") == 3                      # the buffers are released on the way out


@pytest.mark.parametrize("var", [0.0, np.nan, np.inf, -1.0])
def test_a_variance_that_is_not_positive_and_finite_raises_linalg_error(stub, var):
    """a single non-zero weight among them: sw - sw2 / sw = 0, so the device's var is inf or NaN"""
    stub.answer = np.concatenate([np.full(4, np.nan), [10.0, 0.0, 0.0, 0.0, 0.0, 2.0, 1.0, 0.5, var, 0.0, 1.0, 4.0]])
    with pytest.raises(np.linalg.LinAlgError):
        analytic.device_kdes_weighted([111], 10, [np.zeros(4)], [1.0], weight_ptrs=[222])


def recording_fakes(monkeypatch):
    """stand-ins for both device functions in logsv_pricer: (calls of the plain one, calls of the weighted one)"""
    plain, weighted = [], []

    def fake_plain(ptrs, n, grids, divisors, limit=1e16, bandwidth_factor=None, stream=None):
        plain.append(dict(ptrs=list(ptrs), n=n, divisors=list(divisors), limit=limit, factor=bandwidth_factor, stream=stream))
        return [(np.full(len(g), i + 1.0), {"n_kept": n, "n_low": 2, "n_high": 1, "n_nan": 7}) for i, g in enumerate(grids)]

    def fake_weighted(ptrs, n, grids, divisors, weight_ptrs=None, tilt_ptrs=None, gammas=None, limit=1e16, bandwidth_factor=None,
                      stream=None):
        weighted.append(dict(ptrs=list(ptrs), n=n, grids=[np.asarray(g) for g in grids], divisors=list(divisors), weights=weight_ptrs,
                             tilts=list(tilt_ptrs), gammas=list(gammas), limit=limit, factor=bandwidth_factor, stream=stream))
        return [(np.arange(len(g)) + 100.0 * i + 1.0, {"n_kept": n, "n_low": 2, "n_high": 1, "n_nan": 7, "neff": 10.0 + i})
                for i, g in enumerate(grids)]

    monkeypatch.setattr(lp, "device_kdes", fake_plain)
    monkeypatch.setattr(lp, "device_kdes_weighted", fake_weighted)
    return plain, weighted


def test_engine_state_kdes_gamma_axis_and_sources(monkeypatch):
    from stochvolmodels_amd import VariableType
    plain, weighted = recording_fakes(monkeypatch)
    grids = {VariableType.SIGMA: np.linspace(0, 1, 4), VariableType.LOG_RETURN: np.linspace(-1, 1, 6), VariableType.Q_VAR: np.linspace(0, 2, 5)}
    out = lp.engine_state_kdes(fake_engine(), grids, 0.25, bandwidth_factor=0.2, risk_premia_gamma=[-1.0, 1.0])
    assert not plain and len(weighted) == 1
    seen = weighted[0]
    assert seen["ptrs"] == [2000, 1000, 3000] * 2 and seen["divisors"] == [1.0, 1.0, 0.25] * 2      # gamma-major; qvar / ttm
    assert seen["tilts"] == [1000] * 6 and seen["weights"] is None                                  # the tilt is the UNdivided x
    assert seen["gammas"] == [-1.0] * 3 + [1.0] * 3
    assert seen["n"] == 64 and seen["stream"] == 5 and seen["limit"] == 1e16 and seen["factor"] == 0.2
    assert list(out) == list(grids)
    for i, k in enumerate(grids):
        density, stats = out[k]
        assert density.shape == (2, len(grids[k])) and len(stats) == 2
        assert density[0][0] == 100.0 * i + 1.0 and density[1][0] == 100.0 * (3 + i) + 1.0
        assert [s["neff"] for s in stats] == [10.0 + i, 13.0 + i]
    # a float is a sequence of one: the axis is there
    density, stats = lp.engine_state_kdes(fake_engine(), {1: np.zeros(3)}, 0.5, risk_premia_gamma=0.5)[1]
    assert density.shape == (1, 3) and len(stats) == 1 and weighted[-1]["gammas"] == [0.5] and weighted[-1]["ptrs"] == [1000]
    assert lp.engine_state_kdes(fake_engine(), {2: np.zeros(3)}, 0.5, risk_premia_gamma=np.linspace(-1, 1, 16))[2][0].shape == (16, 3)
    for bad in ([], np.linspace(-1, 1, 17)):
        with pytest.raises(ValueError):
            lp.engine_state_kdes(fake_engine(), {1: np.zeros(3)}, 0.5, risk_premia_gamma=bad)
    with pytest.raises(NotImplementedError):
        lp.engine_state_kdes(fake_engine(), {4: np.zeros(3)}, 0.25, risk_premia_gamma=1.0)


def test_no_gamma_routes_to_the_unweighted_function_and_never_to_the_weighted_one(monkeypatch, capsys):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    plain, weighted = recording_fakes(monkeypatch)
    eng = fake_engine()
    monkeypatch.setattr(sv.LogSVPricer, "_simulate_on_engine", staticmethod(lambda *a: eng))
    monkeypatch.setattr(sv.HestonPricer, "_simulate_on_engine", staticmethod(lambda *a: eng))
    monkeypatch.setattr(hp, "hawkesjd_terminal_on_engine", lambda **kw: eng)
    grid = np.linspace(-1.0, 1.0, 4)
    grids = {sv.VariableType.LOG_RETURN: grid, sv.VariableType.Q_VAR: grid}
    lp.engine_state_kdes(eng, grids, 0.25)
    lp.engine_state_kdes(eng, grids, 0.25, risk_premia_gamma=None)
    for pricer in (sv.LogSVPricer(), sv.HestonPricer()):
        kdes = pricer.terminal_value_kdes(params=None, space_grids=grids, ttm=0.25, nb_path=64, seed=1)
        assert kdes[sv.VariableType.Q_VAR].shape == (4,)
        kdes, stats = pricer.terminal_value_kdes(params=None, space_grids=grids, ttm=0.25, nb_path=64, seed=1, return_stats=True,
                                                 risk_premia_gamma=None)
        assert stats[sv.VariableType.LOG_RETURN]["n_kept"] == 64
    # HawkesJDPricer ignores params.risk_premia_gamma here, as it always did: only the explicit keyword tilts
    tilted_params = hp.HawkesJDParams(risk_premia_gamma=1.0)
    for pricer, params in ((sv.LogSVPricer(), None), (sv.HestonPricer(), None), (sv.HawkesJDPricer(), tilted_params)):
        got = pricer.get_log_return_mc_pdf_device(ttm=0.25, params=params, x_grid=grid, nb_path=64, seed=1)
        assert got.shape == (4,)
    assert not weighted and len(plain) == 2 + 4 + 3
    capsys.readouterr()
    # ... and with the keyword, the weighted one and never the plain one
    plain.clear()
    for pricer in (sv.LogSVPricer(), sv.HestonPricer()):
        kdes, stats = pricer.terminal_value_kdes(params=None, space_grids=grids, ttm=0.25, nb_path=64, seed=1, return_stats=True,
                                                 risk_premia_gamma=[-1.0, 1.0], bandwidth_factor=0.3)
        assert kdes[sv.VariableType.Q_VAR].shape == (2, 4) and len(stats[sv.VariableType.Q_VAR]) == 2
        assert weighted[-1]["gammas"] == [-1.0, -1.0, 1.0, 1.0] and weighted[-1]["divisors"] == [1.0, 0.25] * 2
        assert weighted[-1]["factor"] == 0.3 and weighted[-1]["tilts"] == [1000] * 4
    for pricer, params in ((sv.LogSVPricer(), None), (sv.HestonPricer(), None), (sv.HawkesJDPricer(), tilted_params)):
        got, stats = pricer.get_log_return_mc_pdf_device(ttm=0.25, params=params, x_grid=grid, nb_path=64, seed=1,
                                                         risk_premia_gamma=[-1.0, 1.0], return_stats=True)
        assert capsys.readouterr().out == "in mc: num -inf = 2, num +inf = 1, num nans = 7\n"        # once, not once per gamma
        assert got.shape == (2, 4) and len(stats) == 2
        np.testing.assert_array_equal(got[0], np.array([1.0, 2.0, 3.0, 4.0]) / 10.0)                 # each gamma normalised alone
        np.testing.assert_array_equal(got[1], np.array([101.0, 102.0, 103.0, 104.0]) / 410.0)
        assert weighted[-1]["gammas"] == [-1.0, 1.0] and weighted[-1]["ptrs"] == [1000, 1000] and weighted[-1]["tilts"] == [1000, 1000]
        assert pricer.get_log_return_mc_pdf_device(ttm=0.25, params=params, x_grid=grid, nb_path=64, risk_premia_gamma=0.5).shape == (1, 4)
        capsys.readouterr()
    assert not plain


def test_sharded_requests_are_refused_with_the_keyword_too():
    import stochvolmodels_amd as sv
    world2 = types.SimpleNamespace(world=2, rank=0)
    for kw in (dict(comm=world2), dict(devices=[0, 1])):
        with pytest.raises(NotImplementedError):
            sv.LogSVPricer().terminal_value_kdes(params=None, ttm=0.25, nb_path=8, risk_premia_gamma=1.0, **kw)
        with pytest.raises(NotImplementedError):
            sv.HestonPricer().terminal_value_kdes(params=None, space_grids={}, ttm=0.25, nb_path=8, risk_premia_gamma=[1.0], **kw)
        for pricer in (sv.LogSVPricer(), sv.HestonPricer(), sv.HawkesJDPricer()):
            with pytest.raises(NotImplementedError):
                pricer.get_log_return_mc_pdf_device(ttm=0.25, params=None, x_grid=np.zeros(3), nb_path=8, risk_premia_gamma=-1.0, **kw)


def test_pdf_under_risk_kernel_is_the_tilted_and_normalised_fourier_density(monkeypatch):
    """host composition only: exp(gamma x) p(x) normalizer from the two existing routes"""
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    x = np.linspace(-0.5, 0.5, 5)
    p = np.array([0.1, 0.2, 0.4, 0.2, 0.1])
    seen = {}

    def fake_mgf(ttm, phi_grid, model_params, **kw):
        seen.update(ttm=ttm, n_phi=len(phi_grid), re_phi=float(np.real(phi_grid[0])))
        return np.zeros((len(phi_grid), 3), dtype=complex), np.full(len(phi_grid), 0.25 + 0j)

    def fake_pdf(log_mgf_grid, transform_var_grid, space_grid, **kw):
        assert np.all(log_mgf_grid == 0.25) and len(transform_var_grid) == seen["n_phi"]
        return p.copy()

    def fake_forwards(model_params, gamma, ttms, forwards, **kw):
        seen.update(gamma=gamma, ttms=np.asarray(ttms).tolist(), forwards=np.asarray(forwards).tolist())
        return np.array([0.8]), np.array([1.1])

    monkeypatch.setattr(hp, "compute_hawkes_a_mgf_grid", fake_mgf)
    monkeypatch.setattr(hp.mgfp, "pdf_with_mgf_grid", fake_pdf)
    monkeypatch.setattr(hp, "hawkesjd_forwards_under_risk_kernel", fake_forwards)
    got = sv.hawkesjd_pdf_under_risk_kernel(hp.HawkesJDParams(), -1.0, 0.25, x)
    np.testing.assert_array_equal(got, np.exp(-1.0 * x) * p * 0.8)
    assert seen == dict(ttm=0.25, n_phi=hp.MAX_PHI, re_phi=-0.5, gamma=-1.0, ttms=[0.25], forwards=[1.0])
