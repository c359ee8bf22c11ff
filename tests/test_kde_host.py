"""
Host side of the kernel density estimates, no GPU: what device_kdes sends to the library and how it reads the
answer, against a stand-in for libsvmc that records every call and fills the download with a prepared answer; the pointer and
divisor map of engine_state_kdes; the reference's report line and normalisation of get_log_return_mc_pdf_device.
"""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from stochvolmodels_amd import _lib, analytic
from stochvolmodels_amd.pricers import logsv_pricer as lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = [100.0, 0.0, 0.0, 0.0, -0.05, 0.09, 0.12, 0.4]       # n_kept, n_nan, n_low, n_high, mean, var, h, factor


class StubLib:
    """libsvmc stand-in: every call succeeds and is recorded with its arguments; svmc_malloc hands out distinct addresses nothing
    dereferences; svmc_memcpy_d2h fills the destination with `answer` (doubles), where one is set"""

    def __init__(self):
        self.calls, self.next_ptr, self.answer = [], 1 << 20, None

    def names(self):
        return [c[0] for c in self.calls]

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name,) + args)
            if name == "svmc_malloc":
                args[0]._obj.value, self.next_ptr = self.next_ptr, self.next_ptr + (1 << 30)
            elif name == "svmc_kde_workspace_bytes":
                args[1]._obj.value, args[2]._obj.value = 4096, 2048
            elif name == "svmc_memcpy_d2h" and self.answer is not None:
                a = np.ascontiguousarray(self.answer, dtype=np.float64)
                assert a.nbytes == args[2]
                C.memmove(args[0], a.ctypes.data, a.nbytes)
            return 0
        return call


@pytest.fixture
def stub():
    lib = StubLib()
    with pytest.MonkeyPatch.context() as m:
        m.setattr(_lib, "load", lambda: lib)
        yield lib


def test_python_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "svmc.h")).read()
    for name, value in (("TILE", analytic.KDE_TILE), ("MAX_POINTS", analytic.KDE_MAX_POINTS), ("STATS_DOUBLES", analytic.KDE_STATS_DOUBLES)):
        assert int(re.search(r"#define SVMC_KDE_" + name + r" (\d+)", text).group(1)) == value
    assert len(analytic.KDE_STATS_FIELDS) == analytic.KDE_STATS_DOUBLES


def test_device_kdes_one_upload_one_launch_per_vector_one_download(stub):
    grids = [np.linspace(0.0, 1.0, 5), np.linspace(-1.0, 1.0, 201), np.array([0.25, 0.5, 0.75])]
    densities = [np.arange(5) + 0.5, np.arange(201) * 2.0, np.array([7.0, 8.0, 9.0])]
    blocks = [GOOD, [50.0, 1.0, 2.0, 3.0, 0.1, 0.2, 0.3, 0.5], [2.0, 0.0, 0.0, 0.0, 1.0, 1e-300, 1e-150, 0.87]]
    stub.answer = np.concatenate(densities + blocks)
    out = analytic.device_kdes([111, 222, 333], 1000, grids, [1.0, 0.25, 1.0], bandwidth_factor=None, stream=77)
    names = stub.names()
    assert names.count("svmc_memcpy_h2d") == 1 and names.count("svmc_memcpy_d2h") == 1 and names.count("svmc_stream_synchronize") == 1
    assert names.count("svmc_kde_gaussian") == 3 and names.count("svmc_malloc") == names.count("svmc_free") == 3
    assert names.index("svmc_memcpy_h2d") < names.index("svmc_kde_gaussian")
    assert max(i for i, c in enumerate(names) if c == "svmc_kde_gaussian") < names.index("svmc_memcpy_d2h") < names.index("svmc_stream_synchronize")
    up = next(c for c in stub.calls if c[0] == "svmc_memcpy_h2d")
    grid_buf, n_up = up[1], up[3]
    assert n_up == 8 * (5 + 201 + 3) and up[4] == 77
    launches = [c for c in stub.calls if c[0] == "svmc_kde_gaussian"]
    down = next(c for c in stub.calls if c[0] == "svmc_memcpy_d2h")
    res_buf = down[2]
    assert down[3] == 8 * (209 + 3 * 8) and down[4] == 77
    offs = [0, 5, 206]
    for i, c in enumerate(launches):
        _, ptr, n, div, limit, points, m, factor, density, stats, ws, ws_bytes, stream = c
        assert (ptr, n, div, limit, m, factor, stream) == ((111, 222, 333)[i], 1000, (1.0, 0.25, 1.0)[i], 1e16, (5, 201, 3)[i], 0.0, 77)
        assert points == grid_buf + 8 * offs[i]                      # the grids lie back to back in one upload
        assert density == res_buf + 8 * offs[i]                      # ... and so do the densities, the stats blocks behind them
        assert stats == res_buf + 8 * (209 + 8 * i)
        assert ws == launches[0][10] and ws_bytes == 4096            # one workspace: the launches share a stream
    for (d, s), want, block in zip(out, densities, blocks):
        assert np.array_equal(d, want)
        assert [s[k] for k in analytic.KDE_STATS_FIELDS] == block
        assert all(isinstance(s[k], int) for k in ("n_kept", "n_nan", "n_low", "n_high"))
    stub.calls.clear()
    stub.answer = np.concatenate([np.zeros(5), GOOD])
    analytic.device_kdes([111], 10, [grids[0]], [1.0], limit=5.0, bandwidth_factor=0.3)
    c = next(c for c in stub.calls if c[0] == "svmc_kde_gaussian")
    assert c[4] == 5.0 and c[7] == 0.3 and c[12] is None


@pytest.mark.parametrize("n_kept", [0.0, 1.0])
def test_too_few_kept_samples_raise_value_error(stub, n_kept):
    stub.answer = np.concatenate([np.full(4, np.nan), [n_kept, 3.0, 0.0, 0.0, np.nan, np.nan, np.nan, 1.0]])
    with pytest.raises(ValueError):
        analytic.device_kdes([111], 4, [np.zeros(4)], [1.0])
    assert stub.names().count("svmc_free") == 3                      # the buffers are released on the way out


@pytest.mark.parametrize("var", [0.0, np.nan, np.inf, -1.0])
def test_a_variance_that_is_not_positive_and_finite_raises_linalg_error(stub, var):
    stub.answer = np.concatenate([np.full(4, np.nan), [10.0, 0.0, 0.0, 0.0, 0.5, var, 0.0, 0.63]])
    with pytest.raises(np.linalg.LinAlgError):
        analytic.device_kdes([111], 10, [np.zeros(4)], [1.0])


def fake_engine():
    ns = types.SimpleNamespace
    return ns(x=ns(ptr=1000), vol=ns(ptr=2000), qvar=ns(ptr=3000), n_path=64, stream=5)


def test_engine_state_kdes_sources(monkeypatch):
    from stochvolmodels_amd import VariableType
    seen = {}

    def fake(ptrs, n, grids, divisors, limit=1e16, bandwidth_factor=None, stream=None):
        seen.update(ptrs=list(ptrs), n=n, grids=[np.asarray(g) for g in grids], divisors=list(divisors), limit=limit,
                    factor=bandwidth_factor, stream=stream)
        return [(np.full(len(g), float(i)), {"n_kept": n}) for i, g in enumerate(grids)]

    monkeypatch.setattr(lp, "device_kdes", fake)
    grids = {VariableType.SIGMA: np.linspace(0, 1, 4), VariableType.LOG_RETURN: np.linspace(-1, 1, 6), VariableType.Q_VAR: np.linspace(0, 2, 5)}
    out = lp.engine_state_kdes(fake_engine(), grids, 0.25, bandwidth_factor=0.2)
    assert seen["ptrs"] == [2000, 1000, 3000] and seen["divisors"] == [1.0, 1.0, 0.25]           # qvar / ttm; the others untouched
    assert seen["n"] == 64 and seen["stream"] == 5 and seen["limit"] == 1e16 and seen["factor"] == 0.2
    assert list(out) == list(grids) and [out[k][0][0] for k in grids] == [0.0, 1.0, 2.0]
    for g, k in zip(seen["grids"], grids):
        assert np.array_equal(g, grids[k])
    assert list(lp.engine_state_kdes(fake_engine(), {2: np.zeros(3)}, 0.5)) == [2] and seen["ptrs"] == [3000]      # plain codes too
    with pytest.raises(NotImplementedError):
        lp.engine_state_kdes(fake_engine(), {VariableType.LOG_RETURN: np.zeros(3), 4: np.zeros(3)}, 0.25)


def test_log_return_mc_pdf_device_prints_the_references_line_and_normalises(monkeypatch, capsys):
    import stochvolmodels_amd as sv
    density = np.array([0.5, np.nan, 1.5, 2.0])
    stats = dict(n_kept=90, n_nan=7, n_low=2, n_high=1, mean=0.0, var=1.0, h=0.4, factor=0.4)
    calls = []

    def fake(ptrs, n, grids, divisors, **kw):
        calls.append((list(ptrs), n, list(divisors)))
        return [(density.copy(), dict(stats))]

    monkeypatch.setattr(lp, "device_kdes", fake)
    eng = fake_engine()
    monkeypatch.setattr(sv.LogSVPricer, "_simulate_on_engine", staticmethod(lambda *a: eng))
    monkeypatch.setattr(sv.HestonPricer, "_simulate_on_engine", staticmethod(lambda *a: eng))
    grid = np.linspace(-1.0, 1.0, 4)
    for pricer in (sv.LogSVPricer(), sv.HestonPricer()):
        got = pricer.get_log_return_mc_pdf_device(ttm=0.25, params=None, x_grid=grid, nb_path=64, seed=1)
        assert capsys.readouterr().out == "in mc: num -inf = 2, num +inf = 1, num nans = 7\n"
        np.testing.assert_array_equal(got, density / 4.0)           # nansum: the NaN stays and does not poison the rest
        assert calls[-1] == ([1000], 64, [1.0])
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    monkeypatch.setattr(hp, "hawkesjd_terminal_on_engine", lambda **kw: eng)
    got = hp.HawkesJDPricer().get_log_return_mc_pdf_device(ttm=0.25, params=hp.HawkesJDParams(), x_grid=grid, nb_path=64, seed=1)
    assert capsys.readouterr().out == "in mc: num -inf = 2, num +inf = 1, num nans = 7\n"
    np.testing.assert_array_equal(got, density / 4.0)
    assert calls[-1] == ([1000], 64, [1.0])


def test_sharded_requests_are_refused_before_any_device_work(monkeypatch):
    import stochvolmodels_amd as sv
    world2 = types.SimpleNamespace(world=2, rank=0)
    for kw in (dict(comm=world2), dict(devices=[0, 1])):
        with pytest.raises(NotImplementedError):
            sv.LogSVPricer().terminal_value_kdes(params=None, ttm=0.25, nb_path=8, **kw)
        with pytest.raises(NotImplementedError):
            sv.HestonPricer().terminal_value_kdes(params=None, space_grids={}, ttm=0.25, nb_path=8, **kw)
        for pricer in (sv.LogSVPricer(), sv.HestonPricer(), sv.HawkesJDPricer()):
            with pytest.raises(NotImplementedError):
                pricer.get_log_return_mc_pdf_device(ttm=0.25, params=None, x_grid=np.zeros(3), nb_path=8, **kw)
