"""
Gaussian kernel density estimates of the simulated terminal state on the device (svmc_kde_gaussian).

The truth is a np.longdouble brute force of the four steps of include/svmc.h -- filter, two-pass moments, Scott's bandwidth, the
sum of exponentials -- on the downloaded samples (brute_force below); scipy.stats.gaussian_kde is the second witness.  Deviations
are max |a - b| / max(truth) over the grid, "of the peak".

Tolerances (profiles/kde_observed_tolerances.txt is the printout of one run of this file with -s):
  DEVICE_TOL   device against the long-double truth: ten times the largest observed deviation, rounded up to one digit;
  SCIPY_TOL    device against SciPy: ten times the sum of the two largest observed deviations from the truth (the device's and SciPy's);
  CEILING      a condition, not a measurement: n terms of [0, 1] summed in fp64 in any order err by at most n 2^-53 of the sum --
               1.1e-11 at n = 10^5; every observed deviation must lie below it.
"""
import os

import numpy as np
import pytest

from test_densities_host import params

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TTM = 0.25
DEVICE_TOL = 5e-15          # 10 x 4.77e-16 (n = 524 588, m = 9)
SCIPY_TOL = 2e-12           # 10 x (4.77e-16 + 1.08e-13: SciPy at n = 524 588, m = 9)
CEILING = 1.1e-11
LIMIT = 1e16


def brute_force(samples, grid, factor=None):
    """(density, stats) of the four semantic steps in np.longdouble"""
    v = np.asarray(samples, dtype=np.float64)
    is_nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        high, low = ~is_nan & (v > LIMIT), ~is_nan & (v < -LIMIT)
    kept = v[~(is_nan | high | low)].astype(np.longdouble)
    n = kept.size
    mean = kept.sum() / n
    var = ((kept - mean) ** 2).sum() / (n - 1)
    h = np.sqrt(var) * (np.longdouble(n) ** (np.longdouble(-1) / 5) if factor is None else np.longdouble(factor))
    g = np.asarray(grid, dtype=np.longdouble)
    density = np.empty(g.size, dtype=np.longdouble)
    for j0 in range(0, g.size, 16):                                  # 16 points at a time: 16 x n long doubles of memory
        d = (g[j0:j0 + 16, None] - kept[None, :]) / h
        density[j0:j0 + 16] = np.exp(-0.5 * d * d).sum(axis=1)
    density /= n * h * np.sqrt(2 * np.pi * np.longdouble(1))
    return density, dict(n_kept=n, n_nan=int(is_nan.sum()), n_low=int(low.sum()), n_high=int(high.sum()), mean=mean, var=var, h=h)


def deviation(a, truth):
    return float(np.max(np.abs(np.asarray(a, dtype=np.longdouble) - truth)) / np.max(truth))


def report(name, value, bound):
    print(f"KDE-MAX {name}: {value:.3e} (bound {bound:.3e})")
    assert value <= bound, (name, value, bound)


@pytest.fixture(scope="module")
def sv():
    import stochvolmodels_amd
    return stochvolmodels_amd


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "densities.npz"))


class Resident:
    """a host vector uploaded for the life of a `with` block"""

    def __init__(self, data):
        from stochvolmodels_amd import _lib
        from stochvolmodels_amd.engine import DeviceBuffer
        self.data = np.ascontiguousarray(data, dtype=np.float64)
        self.buf = DeviceBuffer(self.data.size)
        L = _lib.load()
        _lib.check(L.svmc_memcpy_h2d(self.buf.ptr, self.data.ctypes.data, self.data.nbytes, None))
        _lib.check(L.svmc_stream_synchronize(None))
        self.ptr, self.n = self.buf.ptr, self.data.size

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.buf.free()


def normal_samples(n, seed=11):
    return -0.05 + 0.3 * np.random.default_rng(seed).standard_normal(n)


def wide_grid(m):
    """m points reaching 8 standard deviations out: the far tail's exponentials underflow"""
    return np.linspace(-0.05 - 8 * 0.3, -0.05 + 8 * 0.3, m) if m > 1 else np.array([-0.05])


def check_against_truth(name, got, stats, data, grid, factor=None):
    from scipy.stats import gaussian_kde
    truth, want = brute_force(data, grid, factor)
    for k in ("n_kept", "n_nan", "n_low", "n_high"):
        assert stats[k] == want[k], (name, k)
    for k in ("mean", "var", "h"):                                   # a few dozen roundings each, of values no larger than these
        assert abs(stats[k] - want[k]) <= 64 * np.finfo(np.float64).eps * max(abs(want[k]), np.sqrt(want["var"])), (name, k)
    kept = data[~np.isnan(data) & (np.abs(data) <= LIMIT)]
    sci = gaussian_kde(kept, bw_method=factor)(grid)
    dev, sci_dev = deviation(got, truth), deviation(sci, truth)
    print(f"KDE-OBSERVED {name}: device {dev:.3e}, scipy {sci_dev:.3e} of the peak against the long-double truth")
    assert dev <= CEILING and dev <= DEVICE_TOL, (name, dev)
    report(f"{name} device - scipy", deviation(got, sci.astype(np.longdouble)), SCIPY_TOL)
    return dev


def shapes():
    from stochvolmodels_amd import analytic
    chunk = analytic.kde_workspace(1000)[1]
    tile = analytic.KDE_TILE
    return chunk, tile, [2, 63, 64, 65, 1000, chunk - 1, chunk, chunk + 1, 3 * chunk + 7], [1, tile - 1, tile, tile + 1, 200, 201]


# ---- 1. small shapes where the kernel can go wrong --------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(9))
def test_small_shapes_against_long_double_and_scipy(sv, which):
    from stochvolmodels_amd import analytic
    chunk, tile, ns, ms = shapes()
    assert analytic.kde_workspace(3 * chunk + 7)[1] == chunk        # all of these sizes are cut into chunks of one length
    n = ns[which]
    data = normal_samples(n)
    with Resident(data) as r:
        grids = [wide_grid(m) for m in ms]
        out = analytic.device_kdes([r.ptr] * len(ms), n, grids, [1.0] * len(ms))
    for m, g, (got, stats) in zip(ms, grids, out):
        assert got.shape == (m,)
        check_against_truth(f"shape n={n} m={m}", got, stats, data, g)
        if m >= 200 and n >= 1000:
            assert got[0] == 0.0 or got[0] < 1e-12 * got.max()          # 8 standard deviations out


def test_longer_chunks_beyond_2_to_19_samples(sv):
    """above 256 chunks of the shortest length the chunk grows with n and a moment thread takes more than 8 samples"""
    from stochvolmodels_amd import analytic
    chunk, tile = analytic.kde_workspace(1000)[1], analytic.KDE_TILE
    n = 256 * chunk + 300
    assert analytic.kde_workspace(n)[1] > chunk
    data = normal_samples(n, seed=12)
    g = wide_grid(tile + 1)
    with Resident(data) as r:
        got, stats = analytic.device_kdes([r.ptr], n, [g], [1.0])[0]
    check_against_truth(f"shape n={n} m={g.size}", got, stats, data, g)


def test_given_bandwidth_factor(sv):
    from stochvolmodels_amd import analytic
    data, g = normal_samples(1000), wide_grid(201)
    with Resident(data) as r:
        got, stats = analytic.device_kdes([r.ptr], 1000, [g], [1.0], bandwidth_factor=0.37)[0]
    assert stats["factor"] == 0.37
    check_against_truth("factor 0.37 n=1000 m=201", got, stats, data, g, factor=0.37)


# ---- 2. filtering -----------------------------------------------------------------------------------------------------------
def test_filtering_counts_and_density(sv):
    from stochvolmodels_amd import analytic
    data = normal_samples(1000, seed=13)
    for i, bad in zip((0, 17, 63, 64, 500, 999, 998), (np.nan, np.inf, -np.inf, 2e16, -2e16, 1e16, np.nan)):
        data[i] = bad
    g = wide_grid(200)
    with Resident(data) as r:
        got, stats = analytic.device_kdes([r.ptr], 1000, [g], [1.0])[0]
    is_nan = np.isnan(data)
    assert stats["n_nan"] == int(is_nan.sum()) == 2
    assert stats["n_high"] == int((~is_nan & (data > LIMIT)).sum()) == 2
    assert stats["n_low"] == int((~is_nan & (data < -LIMIT)).sum()) == 2
    assert stats["n_kept"] == 994                                    # 1e16 itself is kept: the comparisons are strict
    truth, want = brute_force(data, g)
    dev = deviation(got, truth)
    print(f"KDE-OBSERVED filtering n=1000 m=200: device {dev:.3e} of the peak against the long-double truth")
    assert dev <= CEILING and dev <= DEVICE_TOL
    # ... and with the 1e16 out of the way the estimate is test 1's: the kept samples alone give the same density
    data[999] = np.nan
    kept = data[~np.isnan(data) & (np.abs(data) <= LIMIT)]
    with Resident(data) as r, Resident(kept) as k:
        (got, stats), = analytic.device_kdes([r.ptr], 1000, [g], [1.0])
        (alone, _), = analytic.device_kdes([k.ptr], kept.size, [g], [1.0])
    assert stats["n_kept"] == kept.size == 993
    check_against_truth("filtering, kept alone n=993 m=200", got, stats, data, g)
    report("filtered - kept alone", deviation(got, alone.astype(np.longdouble)), DEVICE_TOL)


# ---- 3. divisor -------------------------------------------------------------------------------------------------------------
def test_divisor_is_a_division(sv, fx):
    from stochvolmodels_amd.engine import get_engine
    from stochvolmodels_amd.pricers.logsv_pricer import engine_state_kdes
    p = params(fx, "test")
    n = 1000
    x, vol, q = sv.LogSVPricer().simulate_terminal_values(params=p, ttm=TTM, nb_path=n, seed=3)
    data = q / TTM
    g = np.linspace(data.min() - 3 * data.std(), data.max() + 3 * data.std(), 201)
    got, stats = engine_state_kdes(get_engine(n), {sv.VariableType.Q_VAR: g}, TTM)[sv.VariableType.Q_VAR]
    check_against_truth("divisor qvar / 0.25 n=1000 m=201", got, stats, data, g)


# ---- 4. refusals (SVMC_ERR_INVALID_ARGUMENT reaches Python as ValueError with the library's message) -----------------------
def test_refusals(sv):
    from stochvolmodels_amd import analytic
    g = wide_grid(9)
    with Resident(np.full(1000, 0.5)) as r:                          # sums of 0.5 are exact: the variance is exactly zero
        with pytest.raises(np.linalg.LinAlgError):
            analytic.device_kdes([r.ptr], r.n, [g], [1.0])
    with Resident(np.array([np.nan, 0.25, np.inf])) as r:            # one kept sample
        with pytest.raises(ValueError):
            analytic.device_kdes([r.ptr], r.n, [g], [1.0])
    with Resident(normal_samples(100)) as r:
        with pytest.raises(ValueError, match="svmc_kde_gaussian"):
            analytic.device_kdes([r.ptr], r.n, [np.empty(0)], [1.0])                 # n_points = 0
        with pytest.raises(ValueError, match="svmc_kde_gaussian"):
            analytic.device_kdes([r.ptr], r.n, [g], [0.0])                           # a zero divisor
        with pytest.raises(ValueError, match="svmc_kde_gaussian"):
            analytic.device_kdes([r.ptr], r.n, [g], [1.0], limit=np.inf)
        with pytest.raises(ValueError, match="svmc_kde_gaussian"):
            analytic.device_kdes([r.ptr], r.n, [np.zeros(analytic.KDE_MAX_POINTS + 1)], [1.0])
        got, _ = analytic.device_kdes([r.ptr], r.n, [g], [1.0])[0]                   # the library still answers
        assert np.all(np.isfinite(got))


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_company(sv):
    from stochvolmodels_amd import analytic
    chunk = analytic.kde_workspace(1000)[1]
    n = 3 * chunk + 7
    a, b, c = normal_samples(n, 21), normal_samples(n, 22) * 2.0, normal_samples(n, 23) + 0.4
    g200, g57 = wide_grid(200), np.linspace(-3.0, 3.0, 57)
    with Resident(a) as ra, Resident(b) as rb, Resident(c) as rc:
        first, _ = analytic.device_kdes([ra.ptr], n, [g200], [1.0])[0]
        again, _ = analytic.device_kdes([ra.ptr], n, [g200], [1.0])[0]
        assert np.array_equal(first, again)                          # the same call twice
        three = analytic.device_kdes([rb.ptr, ra.ptr, rc.ptr], n, [g57, g200, g57[:11]], [1.0, 1.0, 0.5])
        assert np.array_equal(three[1][0], first)                    # alone, or one of three
        seven, _ = analytic.device_kdes([ra.ptr], n, [g200[:7]], [1.0])[0]
        assert np.array_equal(seven, first[:7])                      # 200 points, or the first 7 of them
        shifted, _ = analytic.device_kdes([ra.ptr], n, [g200[3:100]], [1.0])[0]
        assert np.array_equal(shifted, first[3:100])                 # a point's sum does not depend on its place in a tile
    assert first.max() > 0.0


# ---- 6. pricers -------------------------------------------------------------------------------------------------------------
def check_against_scipy(name, got, data, grid):
    """full grid against SciPy; every 10th point against the long-double truth (2 x 10^6 long-double exponentials at 10^5 paths)"""
    from scipy.stats import gaussian_kde
    sci = gaussian_kde(data)(grid)
    sub = slice(0, None, 10)
    truth, _ = brute_force(data, grid[sub])
    peak = np.longdouble(max(sci.max(), float(truth.max())))
    dev = float(np.max(np.abs(got[sub].astype(np.longdouble) - truth)) / peak)
    sci_dev = float(np.max(np.abs(sci[sub].astype(np.longdouble) - truth)) / peak)
    print(f"KDE-OBSERVED {name}: device {dev:.3e}, scipy {sci_dev:.3e} of the peak against the long-double truth (every 10th point)")
    assert dev <= CEILING and dev <= DEVICE_TOL, (name, dev)
    report(f"{name} device - scipy", float(np.max(np.abs(got - sci)) / sci.max()), SCIPY_TOL)
    return sci


def normalised_pdf_arithmetic(sample, grid):
    """ModelPricer.get_log_return_mc_pdf's arithmetic on a given sample"""
    from scipy.stats import gaussian_kde
    ok = ~np.isnan(sample) & ~(sample > LIMIT) & ~(sample < -LIMIT)
    density = gaussian_kde(sample[ok])(grid)
    return density / np.nansum(density)


def test_logsv_pricer_kdes_equal_scipy_on_the_same_sample(sv, fx, capsys):
    p = params(fx, "test")
    pricer, n = sv.LogSVPricer(), 100_000
    kdes, stats = pricer.terminal_value_kdes(params=p, ttm=TTM, nb_path=n, seed=77, n=200, n_stdevs=4.5, return_stats=True)
    x, vol, q = pricer.simulate_terminal_values(params=p, ttm=TTM, nb_path=n, seed=77)
    for vt, data in ((sv.VariableType.LOG_RETURN, x), (sv.VariableType.Q_VAR, q / TTM), (sv.VariableType.SIGMA, vol)):
        grid = p.get_variable_space_grid(variable_type=vt, ttm=TTM, n=200, n_stdevs=4.5)
        assert stats[vt]["n_kept"] == n and kdes[vt].shape == grid.shape
        check_against_scipy(f"LogSV {vt.name} n=100000 m=200", kdes[vt], data, grid)
    grid = p.get_variable_space_grid(variable_type=sv.VariableType.LOG_RETURN, ttm=TTM, n=200, n_stdevs=4.5)
    got = pricer.get_log_return_mc_pdf_device(ttm=TTM, params=p, x_grid=grid, nb_path=n, seed=77)
    out = capsys.readouterr().out
    print(out, end="")                                               # what the checks above printed stays in the printout
    assert "in mc: num -inf = 0, num +inf = 0, num nans = 0\n" in out
    want = normalised_pdf_arithmetic(x, grid)
    report("LogSV get_log_return_mc_pdf_device", float(np.max(np.abs(got - want)) / want.max()), SCIPY_TOL)
    assert abs(got.sum() - 1.0) < 1e-12


def test_heston_pricer_kdes_equal_scipy_on_the_same_sample(sv, capsys):
    h = sv.HestonParams(v0=0.04, theta=0.05, kappa=3.0, rho=-0.6, volvol=0.5)
    grids = {sv.VariableType.LOG_RETURN: np.linspace(-0.6, 0.4, 200), sv.VariableType.Q_VAR: np.linspace(0.0, 0.2, 200),
             sv.VariableType.SIGMA: np.linspace(0.0, 0.25, 200)}
    hp, n = sv.HestonPricer(), 100_000
    kdes = hp.terminal_value_kdes(params=h, space_grids=grids, ttm=TTM, nb_path=n, seed=5, scheme="euler")
    x, var, q = hp.simulate_terminal_values(params=h, ttm=TTM, nb_path=n, seed=5, scheme="euler")
    for vt, data in ((sv.VariableType.LOG_RETURN, x), (sv.VariableType.Q_VAR, q / TTM), (sv.VariableType.SIGMA, var)):
        check_against_scipy(f"Heston {vt.name} n=100000 m=200", kdes[vt], data, grids[vt])
    grid = grids[sv.VariableType.LOG_RETURN]
    got = hp.get_log_return_mc_pdf_device(ttm=TTM, params=h, x_grid=grid, nb_path=n, seed=5, scheme="euler")
    out = capsys.readouterr().out
    print(out, end="")                                               # what the checks above printed stays in the printout
    assert "in mc: num -inf = 0, num +inf = 0, num nans = 0\n" in out
    want = normalised_pdf_arithmetic(x, grid)
    report("Heston get_log_return_mc_pdf_device", float(np.max(np.abs(got - want)) / want.max()), SCIPY_TOL)


def test_hawkes_pricer_log_return_pdf_equals_scipy_on_the_same_sample(sv, capsys):
    from stochvolmodels_amd.engine import get_engine
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    from stochvolmodels_amd.pricers.logsv_pricer import engine_state_kdes
    p, n = hp.HawkesJDParams(), 100_000
    pricer = hp.HawkesJDPricer()
    x, _, _ = pricer.simulate_terminal_values(params=p, ttm=TTM, nb_path=n, seed=9)
    grid = np.linspace(x.mean() - 6 * x.std(), x.mean() + 6 * x.std(), 200)
    got = pricer.get_log_return_mc_pdf_device(ttm=TTM, params=p, x_grid=grid, nb_path=n, seed=9)
    out = capsys.readouterr().out
    print(out, end="")                                               # what the checks above printed stays in the printout
    assert "in mc: num -inf = 0, num +inf = 0, num nans = 0\n" in out
    want = normalised_pdf_arithmetic(x, grid)
    report("Hawkes get_log_return_mc_pdf_device", float(np.max(np.abs(got - want)) / want.max()), SCIPY_TOL)
    density, _ = engine_state_kdes(get_engine(n), {sv.VariableType.LOG_RETURN: grid}, TTM)[sv.VariableType.LOG_RETURN]
    check_against_scipy("Hawkes LOG_RETURN n=100000 m=200", density, x, grid)


# ---- 7. against the model: the device adds nothing to what the host route gives ---------------------------------------------
def test_device_kde_is_as_close_to_the_model_density_as_the_host_route(sv, fx):
    """a sanity check, not a parity check: a KDE is biased by its bandwidth, so the total-variation distance between the
    normalised KDE of x and the normalised second-order masses of logsv_pdfs is only required not to exceed what
    scipy.stats.gaussian_kde gives on the same 400 000 paths, plus test 6's tolerance -- on the grid and the set of
    test_gpu_densities.test_second_order_density_against_400000_paths"""
    p = params(fx, "test")
    n, seed, space = int(fx["fig_paths"]), int(fx["fig_seed"]), fx["fig_x_space"]
    assert n == 400_000 and space.size == 200
    pricer = sv.LogSVPricer()
    got = pricer.get_log_return_mc_pdf_device(ttm=TTM, params=p, x_grid=space, nb_path=n, seed=seed)
    x = pricer.simulate_terminal_values(params=p, ttm=TTM, nb_path=n, seed=seed)[0]
    host = normalised_pdf_arithmetic(x, space)
    m = pricer.logsv_pdfs(params=p, ttm=TTM, space_grid=space, variable_type=sv.VariableType.LOG_RETURN)
    model = m / np.nansum(m)
    tv_device, tv_host = 0.5 * np.abs(got - model).sum(), 0.5 * np.abs(host - model).sum()
    print(f"KDE-MODEL total variation to the second-order density: device {tv_device:.6e}, host SciPy route {tv_host:.6e}, "
          f"device - host {tv_device - tv_host:.3e}")
    assert tv_host < 0.05                                            # the two curves are the same density to begin with
    assert tv_device <= tv_host + SCIPY_TOL
