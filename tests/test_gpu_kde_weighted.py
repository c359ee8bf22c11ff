"""
Weighted Gaussian kernel density estimates on the device (svmc_kde_gaussian_weighted): densities under the
exponential risk-premia kernel exp(gamma x), and under any non-negative weights.

The truth is a np.longdouble brute force of the six steps of include/svmc.h -- sample, weight, keep rule, weighted moments, Scott's
bandwidth from the effective sample size, the weighted sum of exponentials (brute_force_weighted below; the keep rule alone is
taken in fp64, where the header defines it); scipy.stats.gaussian_kde(kept, weights=w_kept) is the second witness.  Deviations are
max |a - b| / max(truth) over the grid, "of the peak", as in test_gpu_kde.py, whose helpers and CEILING this file uses.

Tolerances (profiles/kde_weighted_observed_tolerances.txt is the printout of one run of this file with -s):
  DEVICE_TOL   device against the long-double truth: ten times the largest observed deviation, rounded up to one digit;
  SCIPY_TOL    device against SciPy: ten times the largest observed deviation between the two, rounded up to one digit;
  CEILING      test_gpu_kde.py's condition, 1.1e-11: every observed deviation must lie below it, whatever was recorded.
"""
import os

import numpy as np
import pytest

from test_densities_host import params
from test_gpu_kde import CEILING, LIMIT, Resident, deviation, normal_samples, report, wide_grid

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TTM = 0.25
DEVICE_TOL = 8e-15          # 10 x 7.51e-16 (n = 524 588, m = 9, tilt gamma = 1)
SCIPY_TOL = 2e-12           # 10 x 1.23e-13 (n = 524 588, m = 9, weights and tilt: SciPy's own 1.23e-13 from the truth, the device's 7.5e-16)
assert DEVICE_TOL <= CEILING and SCIPY_TOL <= CEILING     # no recording may raise the ceiling
EPS = np.finfo(np.float64).eps
GAMMAS = (-2.0, 1.0, 4.45)


def brute_force_weighted(values, grid, weights=None, tilt=None, gamma=0.0, factor=None):
    """(density, stats, kept mask, fp64 weights) of the six semantic steps in np.longdouble; `values` are the divided samples"""
    v = np.asarray(values, dtype=np.float64)
    w = np.ones(v.size, dtype=np.longdouble)
    if weights is not None:
        w = w * np.asarray(weights, dtype=np.longdouble)
    if tilt is not None:
        with np.errstate(over="ignore", invalid="ignore"):
            w = w * np.exp(np.longdouble(gamma) * np.asarray(tilt, dtype=np.longdouble))
    with np.errstate(over="ignore", invalid="ignore"):
        w64 = w.astype(np.float64)                                   # the keep rule is the header's: fp64 w >= 0, w and w^2 finite
        good_w = (w64 >= 0.0) & np.isfinite(w64) & np.isfinite(w64 * w64)
        is_nan = np.isnan(v)
        high, low = ~is_nan & (v > LIMIT), ~is_nan & (v < -LIMIT)
    passed = ~(is_nan | high | low)
    keep = passed & good_w
    kv, kw = v[keep].astype(np.longdouble), w[keep]
    sw, sw2 = kw.sum(), (kw * kw).sum()
    neff = sw * sw / sw2
    mean = (kw * kv).sum() / sw
    var = (kw * (kv - mean) ** 2).sum() / (sw - sw2 / sw)
    f = neff ** (np.longdouble(-1) / 5) if factor is None else np.longdouble(factor)
    h = np.sqrt(var) * f
    g = np.asarray(grid, dtype=np.longdouble)
    density = np.empty(g.size, dtype=np.longdouble)
    for j0 in range(0, g.size, 16):                                  # 16 points at a time: 16 x n long doubles of memory
        d = (g[j0:j0 + 16, None] - kv[None, :]) / h
        density[j0:j0 + 16] = (kw[None, :] * np.exp(-0.5 * d * d)).sum(axis=1)
    density /= sw * h * np.sqrt(2 * np.pi * np.longdouble(1))
    stats = dict(n_kept=int(keep.sum()), n_nan=int(is_nan.sum()), n_low=int(low.sum()), n_high=int(high.sum()),
                 n_bad_weight=int((passed & ~good_w).sum()), sum_w=sw, neff=neff, mean=mean, var=var, h=h, factor=f)
    return density, stats, keep, w64


def check_against_truth(name, got, stats, values, grid, weights=None, tilt=None, gamma=0.0, factor=None, scipy_too=True):
    from scipy.stats import gaussian_kde
    truth, want, keep, w64 = brute_force_weighted(values, grid, weights, tilt, gamma, factor)
    for k in ("n_kept", "n_nan", "n_low", "n_high", "n_bad_weight"):
        assert stats[k] == want[k], (name, k, stats[k], want[k])
    for k in ("sum_w", "neff", "mean", "var", "h"):                  # f7's scale: a few dozen roundings each, of values no larger than these
        err, scale = abs(stats[k] - want[k]), max(abs(want[k]), np.sqrt(want["var"]))
        print(f"KDE-STATS {name} {k}: {float(err / scale) / EPS:.2f} eps")
        assert err <= 64 * EPS * scale, (name, k, stats[k], want[k])
    dev = deviation(got, truth)
    if not scipy_too:
        print(f"KDE-OBSERVED {name}: device {dev:.3e} of the peak against the long-double truth")
        assert dev <= CEILING and dev <= DEVICE_TOL, (name, dev)
        return dev
    sci = gaussian_kde(np.asarray(values, dtype=np.float64)[keep], weights=w64[keep], bw_method=factor)(grid)
    sci_dev, both = deviation(sci, truth), deviation(got, sci.astype(np.longdouble))
    print(f"KDE-OBSERVED {name}: device {dev:.3e}, scipy {sci_dev:.3e} of the peak against the long-double truth, device - scipy {both:.3e}")
    assert dev <= CEILING and dev <= DEVICE_TOL, (name, dev)
    report(f"{name} device - scipy", both, SCIPY_TOL)
    return dev


@pytest.fixture(scope="module")
def sv():
    import stochvolmodels_amd
    return stochvolmodels_amd


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "densities.npz"))


def shapes():
    from stochvolmodels_amd import analytic
    chunk = analytic.kde_weighted_workspace(1000)[1]
    tile = analytic.KDE_TILE
    return chunk, tile, [2, 63, 64, 65, 1000, chunk - 1, chunk, chunk + 1, 3 * chunk + 7], [1, tile - 1, tile, tile + 1, 200, 201]


def modes(data, other, weights):
    """(label, weights, tilt, gamma) of a shape's five estimates: the log-return tilted by itself at three gammas, a weights
    vector, and weights with the tilt of ANOTHER vector"""
    return [(f"tilt gamma={g}", None, data, g) for g in GAMMAS] + [("weights", weights, None, 0.0), ("weights and tilt gamma=1.0", weights, other, 1.0)]


# ---- 1. small shapes where the kernel can go wrong --------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(9))
def test_small_shapes_against_long_double_and_scipy(sv, which):
    from stochvolmodels_amd import analytic
    chunk, tile, ns, ms = shapes()
    assert analytic.kde_weighted_workspace(3 * chunk + 7)[1] == chunk == analytic.kde_workspace(1000)[1]
    n = ns[which]
    data, other, weights = normal_samples(n), normal_samples(n, seed=31), np.random.default_rng(41).random(n)
    grids = [wide_grid(m) for m in ms]
    with Resident(data) as r, Resident(other) as ro, Resident(weights) as rw:
        ptr = {id(data): r.ptr, id(other): ro.ptr, id(weights): rw.ptr, id(None): None}
        for label, w, t, gamma in modes(data, other, weights):
            out = analytic.device_kdes_weighted([r.ptr] * len(ms), n, grids, [1.0] * len(ms), weight_ptrs=[ptr[id(w)]] * len(ms),
                                                tilt_ptrs=[ptr[id(t)]] * len(ms), gammas=[gamma] * len(ms))
            for m, g, (got, stats) in zip(ms, grids, out):
                assert got.shape == (m,)
                check_against_truth(f"shape n={n} m={m} {label}", got, stats, data, g, w, t, gamma)


# ---- 2. long chunks ---------------------------------------------------------------------------------------------------------
def test_longer_chunks_beyond_2_to_19_samples(sv):
    """above 256 chunks of the shortest length the chunk grows with n and a moment thread takes more than 8 samples"""
    from stochvolmodels_amd import analytic
    chunk, tile = analytic.kde_weighted_workspace(1000)[1], analytic.KDE_TILE
    n = 256 * chunk + 300
    assert n == 524_588 and analytic.kde_weighted_workspace(n)[1] > chunk
    data, other, weights = normal_samples(n, seed=12), normal_samples(n, seed=32), np.random.default_rng(42).random(n)
    g = wide_grid(tile + 1)
    with Resident(data) as r, Resident(other) as ro, Resident(weights) as rw:
        out = analytic.device_kdes_weighted([r.ptr] * 3, n, [g] * 3, [1.0] * 3, weight_ptrs=[None, rw.ptr, rw.ptr],
                                            tilt_ptrs=[r.ptr, None, ro.ptr], gammas=[1.0, 0.0, 1.0])
    for (got, stats), (label, w, t, gamma) in zip(out, [modes(data, other, weights)[i] for i in (1, 3, 4)]):
        check_against_truth(f"shape n={n} m={g.size} {label}", got, stats, data, g, w, t, gamma)


# ---- 3. filtering -----------------------------------------------------------------------------------------------------------
def test_filtering_counts_and_density(sv):
    from stochvolmodels_amd import analytic
    n, gamma = 3000, 1.0
    data, tilt, weights = normal_samples(n, seed=13), normal_samples(n, seed=33), np.random.default_rng(43).random(n) + 0.1
    for i, bad in zip((0, 17, 63, 64, 500, 2999, 2998), (np.nan, np.inf, -np.inf, 2e16, -2e16, 1e16, np.nan)):
        data[i] = bad                                                # 1e16 itself is kept: the comparisons are strict
    for i, bad in zip((1, 65, 255, 256, 1000, 17), (np.nan, np.inf, -0.25, 0.0, 0.0, np.nan)):
        weights[i] = bad                                             # 17: a bad weight on a bad value counts with the value
    for i, bad in zip((2, 66, 2047, 2048, 2049, 64), (np.nan, 711.0, 1000.0, 400.0, -800.0, np.nan)):
        tilt[i] = bad                                                # exp(711), exp(1000) overflow; exp(400)^2 overflows; exp(-800) = +0 is kept
    g = wide_grid(200)
    with Resident(data) as r, Resident(tilt) as rt, Resident(weights) as rw:
        (got, stats), = analytic.device_kdes_weighted([r.ptr], n, [g], [1.0], weight_ptrs=[rw.ptr], tilt_ptrs=[rt.ptr], gammas=[gamma])
    assert (stats["n_nan"], stats["n_high"], stats["n_low"]) == (2, 2, 2)
    assert stats["n_bad_weight"] == 3 + 4                            # weights NaN, inf, negative; tilts NaN, 711, 1000, 400
    assert stats["n_kept"] == n - 6 - 7                              # the two zero weights and the underflowed exponential are KEPT
    check_against_truth(f"filtering n={n} m=200 weights and tilt", got, stats, data, g, weights, tilt, gamma, scipy_too=False)
    # ... and with the 1e16 out of the way the estimate is the kept set's: the kept samples alone, with their weights, give the
    # same density
    data[2999] = np.nan
    with Resident(data) as r, Resident(tilt) as rt, Resident(weights) as rw:
        (got, stats), = analytic.device_kdes_weighted([r.ptr], n, [g], [1.0], weight_ptrs=[rw.ptr], tilt_ptrs=[rt.ptr], gammas=[gamma])
    assert stats["n_nan"] == 3 and stats["n_kept"] == n - 7 - 7
    check_against_truth(f"filtering n={n} m=200 weights and tilt, 1e16 out", got, stats, data, g, weights, tilt, gamma, scipy_too=False)
    _, _, keep, w64 = brute_force_weighted(data, g, weights, tilt, gamma)
    assert keep.sum() == stats["n_kept"] and (w64[keep] == 0.0).sum() == 3
    with Resident(data[keep]) as k, Resident(w64[keep]) as kw:
        (alone, alone_stats), = analytic.device_kdes_weighted([k.ptr], int(keep.sum()), [g], [1.0], weight_ptrs=[kw.ptr])
    assert alone_stats["n_kept"] == stats["n_kept"] and alone_stats["n_bad_weight"] == 0
    check_against_truth(f"filtering, kept alone n={int(keep.sum())} m=200 weights", alone, alone_stats, data[keep], g, w64[keep])
    report("filtered - kept alone", deviation(got, alone.astype(np.longdouble)), DEVICE_TOL)


# ---- 4. bit identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 3 * 2048 + 7, 524_588])
def test_without_weights_and_tilt_the_bits_are_the_unweighted_estimates(sv, n):
    from stochvolmodels_amd import analytic
    data = normal_samples(n, seed=14)
    data[[0, 5, n - 1]] = (np.nan, 2e16, -np.inf)
    grids, divisors = [wide_grid(201), wide_grid(9)], [1.0, 0.25]
    with Resident(data) as r:
        plain = analytic.device_kdes([r.ptr] * 2, n, grids, divisors)
        weighted = analytic.device_kdes_weighted([r.ptr] * 2, n, grids, divisors)
        given = analytic.device_kdes_weighted([r.ptr], n, grids[:1], [1.0], gammas=[3.0], bandwidth_factor=0.37)[0]
        given_plain = analytic.device_kdes([r.ptr], n, grids[:1], [1.0], bandwidth_factor=0.37)[0]
    for (d0, s0), (d1, s1) in list(zip(plain, weighted)) + [(given_plain, given)]:
        assert np.array_equal(d0, d1) and d0.max() > 0.0
        for k in ("n_kept", "n_nan", "n_low", "n_high", "mean", "var", "h", "factor"):
            assert s0[k] == s1[k], k
        assert s1["n_bad_weight"] == 0 and s1["sum_w"] == s1["sum_w2"] == s1["neff"] == s1["n_kept"] == n - 3


def test_bits_do_not_depend_on_the_company(sv):
    from stochvolmodels_amd import analytic
    chunk = analytic.kde_weighted_workspace(1000)[1]
    n = 3 * chunk + 7
    a, b, c = normal_samples(n, 21), normal_samples(n, 22) * 2.0, normal_samples(n, 23) + 0.4
    w = np.random.default_rng(44).random(n)
    g200, g57 = wide_grid(200), np.linspace(-3.0, 3.0, 57)
    with Resident(a) as ra, Resident(b) as rb, Resident(c) as rc, Resident(w) as rw:
        def kde(ptrs, grids, divisors, weights, tilts, gammas):
            return analytic.device_kdes_weighted(ptrs, n, grids, divisors, weight_ptrs=weights, tilt_ptrs=tilts, gammas=gammas)
        first, _ = kde([ra.ptr], [g200], [1.0], [None], [ra.ptr], [1.0])[0]
        again, _ = kde([ra.ptr], [g200], [1.0], [None], [ra.ptr], [1.0])[0]
        assert np.array_equal(first, again)                          # the same call twice
        five = kde([rb.ptr, ra.ptr, ra.ptr, rc.ptr, ra.ptr], [g57, g200, g200, g57[:11], g200], [1.0, 1.0, 1.0, 0.5, 1.0],
                   [rw.ptr, None, None, None, rw.ptr], [ra.ptr, ra.ptr, ra.ptr, rb.ptr, ra.ptr], [-2.0, -1.0, 1.0, 4.45, 1.0])
        assert np.array_equal(five[2][0], first)                     # alone, or among other vectors and gammas
        assert not np.array_equal(five[1][0], first) and not np.array_equal(five[4][0], first)
        minus, _ = kde([ra.ptr], [g200], [1.0], [None], [ra.ptr], [-1.0])[0]
        assert np.array_equal(five[1][0], minus)
        both, _ = kde([ra.ptr], [g200], [1.0], [rw.ptr], [ra.ptr], [1.0])[0]
        assert np.array_equal(five[4][0], both)
        seven, _ = kde([ra.ptr], [g200[:7]], [1.0], [None], [ra.ptr], [1.0])[0]
        assert np.array_equal(seven, first[:7])                      # 200 points, or the first 7 of them
        shifted, _ = kde([ra.ptr], [g200[3:100]], [1.0], [None], [ra.ptr], [1.0])[0]
        assert np.array_equal(shifted, first[3:100])                 # a point's sum does not depend on its place in a tile
    assert first.max() > 0.0


# ---- 5. given bandwidth factor; divisor -------------------------------------------------------------------------------------
def test_given_bandwidth_factor(sv):
    from stochvolmodels_amd import analytic
    data, g = normal_samples(1000), wide_grid(201)
    with Resident(data) as r:
        got, stats = analytic.device_kdes_weighted([r.ptr], 1000, [g], [1.0], tilt_ptrs=[r.ptr], gammas=[-2.0], bandwidth_factor=0.37)[0]
    assert stats["factor"] == 0.37
    check_against_truth("factor 0.37 n=1000 m=201 tilt gamma=-2.0", got, stats, data, g, None, data, -2.0, factor=0.37)


def test_divisor_is_a_division_and_the_tilt_is_not_divided(sv, fx):
    from stochvolmodels_amd.engine import get_engine
    from stochvolmodels_amd.pricers.logsv_pricer import engine_state_kdes
    p = params(fx, "test")
    n = 1000
    x, vol, q = sv.LogSVPricer().simulate_terminal_values(params=p, ttm=TTM, nb_path=n, seed=3)
    data = q / TTM
    g = np.linspace(data.min() - 3 * data.std(), data.max() + 3 * data.std(), 201)
    density, stats = engine_state_kdes(get_engine(n), {sv.VariableType.Q_VAR: g}, TTM, risk_premia_gamma=[1.0, -4.45])[sv.VariableType.Q_VAR]
    assert density.shape == (2, 201)
    for i, gamma in enumerate((1.0, -4.45)):
        check_against_truth(f"divisor qvar / 0.25 n=1000 m=201 tilt x gamma={gamma}", density[i], stats[i], data, g, None, x, gamma)


# ---- 6. refusals, before any launch -----------------------------------------------------------------------------------------
def test_refusals(sv):
    from stochvolmodels_amd import _lib, analytic
    from stochvolmodels_amd._lib import SvmcError
    from stochvolmodels_amd.engine import DeviceBuffer
    L = _lib.load()
    n, m = 100, 9
    ws_bytes = analytic.kde_weighted_workspace(n)[0]
    assert ws_bytes == 8 * (2048 + analytic.KDE_MAX_POINTS) > analytic.kde_workspace(n)[0]
    nst = analytic.KDE_WEIGHTED_STATS_DOUBLES
    sentinel = np.full(m + nst, -7.0)
    with Resident(normal_samples(n)) as r, Resident(wide_grid(m)) as rg, Resident(sentinel) as res:
        ws = DeviceBuffer(ws_bytes // 8)
        good = dict(values=r.ptr, weights=None, tilt=None, gamma=1.0, n=n, divisor=1.0, limit=1e16, points=rg.ptr, n_points=m,
                    factor=0.0, density=res.ptr, stats=res.buf.offset(m), ws=ws.ptr, ws_bytes=ws_bytes)

        def call(**change):
            a = dict(good, **change)
            return L.svmc_kde_gaussian_weighted(a["values"], a["weights"], a["tilt"], a["gamma"], a["n"], a["divisor"], a["limit"],
                                                a["points"], a["n_points"], a["factor"], a["density"], a["stats"], a["ws"],
                                                a["ws_bytes"], None)
        try:
            bad = [dict(values=None), dict(points=None), dict(density=None), dict(stats=None), dict(ws=None), dict(n=0), dict(n=1 << 40),
                   dict(n_points=0), dict(n_points=-1), dict(n_points=analytic.KDE_MAX_POINTS + 1),
                   dict(divisor=0.0), dict(divisor=-1.0), dict(divisor=np.inf), dict(divisor=np.nan),
                   dict(limit=0.0), dict(limit=-1.0), dict(limit=np.inf), dict(limit=np.nan),
                   dict(factor=np.nan), dict(factor=np.inf), dict(gamma=np.nan), dict(gamma=np.inf), dict(gamma=-np.inf)]
            for change in bad:
                with pytest.raises(ValueError, match="svmc_kde_gaussian_weighted"):
                    _lib.check(call(**change))
            with pytest.raises(SvmcError, match="workspace too small"):
                _lib.check(call(ws_bytes=8 * (2048 + m) - 8))                # n_chunks = 1: one double short
            with pytest.raises(ValueError, match="svmc_kde_weighted_workspace_bytes"):
                analytic.kde_weighted_workspace(0)
            with pytest.raises(ValueError, match="svmc_kde_weighted_workspace_bytes"):
                _lib.check(L.svmc_kde_weighted_workspace_bytes(n, None, None))
            back = np.empty_like(sentinel)
            _lib.check(L.svmc_memcpy_d2h(back.ctypes.data, res.ptr, back.nbytes, None))
            _lib.check(L.svmc_stream_synchronize(None))
            assert np.array_equal(back, sentinel)                            # refused before any launch: nothing was written
            _lib.check(call(ws_bytes=8 * (2048 + m)))                        # the smallest workspace that serves: the library still answers
            _lib.check(L.svmc_memcpy_d2h(back.ctypes.data, res.ptr, back.nbytes, None))
            _lib.check(L.svmc_stream_synchronize(None))
            assert np.all(np.isfinite(back)) and back[m] == n and np.all(back[:m] >= 0.0)
        finally:
            ws.free()
    g = wide_grid(9)
    with Resident(np.full(1000, 0.5)) as r, Resident(normal_samples(1000)) as rt:       # the weighted variance is exactly zero
        with pytest.raises(np.linalg.LinAlgError):
            analytic.device_kdes_weighted([r.ptr], r.n, [g], [1.0], tilt_ptrs=[rt.ptr], gammas=[1.0])
    one = np.zeros(100)
    one[37] = 2.5
    with Resident(normal_samples(100)) as r, Resident(one) as rw:                       # a single non-zero weight: this project's rule
        with pytest.raises(np.linalg.LinAlgError):
            analytic.device_kdes_weighted([r.ptr], r.n, [g], [1.0], weight_ptrs=[rw.ptr])
    with Resident(np.array([0.1, 0.25, 0.3])) as r, Resident(np.array([np.nan, 1.0, -1.0])) as rw:      # one kept sample
        with pytest.raises(ValueError):
            analytic.device_kdes_weighted([r.ptr], r.n, [g], [1.0], weight_ptrs=[rw.ptr])


# ---- 7. pricers -------------------------------------------------------------------------------------------------------------
PRICER_GAMMAS = [-1.0, 1.0]


def check_against_scipy(name, got, data, tilt, gamma, grid):
    from scipy.stats import gaussian_kde
    sci = gaussian_kde(data, weights=np.exp(gamma * tilt))(grid)
    report(f"{name} device - scipy", float(np.max(np.abs(got - sci)) / sci.max()), SCIPY_TOL)
    return sci


def plain_bits(sv, n, sources, grids):
    """the existing launches on the engine's resident state: what a call without the keyword returned before"""
    from stochvolmodels_amd import analytic
    from stochvolmodels_amd.engine import get_engine
    eng = get_engine(n)
    src = {sv.VariableType.LOG_RETURN: (eng.x.ptr, 1.0), sv.VariableType.Q_VAR: (eng.qvar.ptr, TTM), sv.VariableType.SIGMA: (eng.vol.ptr, 1.0)}
    out = analytic.device_kdes([src[vt][0] for vt in sources], n, [grids[vt] for vt in sources], [src[vt][1] for vt in sources],
                               stream=eng.stream)
    return {vt: d for vt, (d, _) in zip(sources, out)}


def test_logsv_pricer_weighted_kdes_equal_scipy_on_the_same_sample(sv, fx):
    p = params(fx, "test")
    pricer, n = sv.LogSVPricer(), 100_000
    vts = (sv.VariableType.LOG_RETURN, sv.VariableType.Q_VAR, sv.VariableType.SIGMA)
    grids = {vt: p.get_variable_space_grid(variable_type=vt, ttm=TTM, n=200, n_stdevs=4.5) for vt in vts}
    kdes, stats = pricer.terminal_value_kdes(params=p, ttm=TTM, nb_path=n, seed=77, n=200, n_stdevs=4.5, return_stats=True,
                                             risk_premia_gamma=PRICER_GAMMAS)
    x, vol, q = pricer.simulate_terminal_values(params=p, ttm=TTM, nb_path=n, seed=77)
    for vt, data in zip(vts, (x, q / TTM, vol)):
        assert kdes[vt].shape == (2, 200) and len(stats[vt]) == 2
        for i, gamma in enumerate(PRICER_GAMMAS):
            assert stats[vt][i]["n_kept"] == n and stats[vt][i]["n_bad_weight"] == 0 and 2 <= stats[vt][i]["neff"] < n
            check_against_scipy(f"LogSV {vt.name} gamma={gamma} n=100000 m=200", kdes[vt][i], data, x, gamma, grids[vt])
    absent = pricer.terminal_value_kdes(params=p, ttm=TTM, nb_path=n, seed=77, n=200, n_stdevs=4.5)
    none = pricer.terminal_value_kdes(params=p, ttm=TTM, nb_path=n, seed=77, n=200, n_stdevs=4.5, risk_premia_gamma=None)
    want = plain_bits(sv, n, vts, grids)
    for vt in vts:
        assert np.array_equal(absent[vt], want[vt]) and np.array_equal(none[vt], want[vt]) and absent[vt].shape == (200,)
    pdf = pricer.get_log_return_mc_pdf_device(ttm=TTM, params=p, x_grid=grids[vts[0]], nb_path=n, seed=77, risk_premia_gamma=1.0)
    assert pdf.shape == (1, 200) and np.array_equal(pdf[0], kdes[vts[0]][1] / np.nansum(kdes[vts[0]][1]))


def test_heston_pricer_weighted_kdes_equal_scipy_on_the_same_sample(sv):
    h = sv.HestonParams(v0=0.04, theta=0.05, kappa=3.0, rho=-0.6, volvol=0.5)
    vts = (sv.VariableType.LOG_RETURN, sv.VariableType.Q_VAR, sv.VariableType.SIGMA)
    grids = dict(zip(vts, (np.linspace(-0.6, 0.4, 200), np.linspace(0.0, 0.2, 200), np.linspace(0.0, 0.25, 200))))
    hp, n = sv.HestonPricer(), 100_000
    kdes = hp.terminal_value_kdes(params=h, space_grids=grids, ttm=TTM, nb_path=n, seed=5, scheme="euler", risk_premia_gamma=PRICER_GAMMAS)
    x, var, q = hp.simulate_terminal_values(params=h, ttm=TTM, nb_path=n, seed=5, scheme="euler")
    for vt, data in zip(vts, (x, q / TTM, var)):
        for i, gamma in enumerate(PRICER_GAMMAS):
            check_against_scipy(f"Heston {vt.name} gamma={gamma} n=100000 m=200", kdes[vt][i], data, x, gamma, grids[vt])
    absent = hp.terminal_value_kdes(params=h, space_grids=grids, ttm=TTM, nb_path=n, seed=5, scheme="euler")
    want = plain_bits(sv, n, vts, grids)
    for vt in vts:
        assert np.array_equal(absent[vt], want[vt])


def hawkes_sample(sv, n, seed):
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    p, pricer = hp.HawkesJDParams(), hp.HawkesJDPricer()
    x, _, _ = pricer.simulate_terminal_values(params=p, ttm=TTM, nb_path=n, seed=seed)
    return p, pricer, x, np.linspace(x.mean() - 6 * x.std(), x.mean() + 6 * x.std(), 200)


def test_hawkes_pricer_weighted_log_return_pdf_equals_scipy_on_the_same_sample(sv, capsys):
    import dataclasses
    from scipy.stats import gaussian_kde
    n = 100_000
    p, pricer, x, grid = hawkes_sample(sv, n, 9)
    got, stats = pricer.get_log_return_mc_pdf_device(ttm=TTM, params=p, x_grid=grid, nb_path=n, seed=9, risk_premia_gamma=PRICER_GAMMAS,
                                                     return_stats=True)
    out = capsys.readouterr().out
    print(out, end="")
    assert out.count("in mc: num -inf = 0, num +inf = 0, num nans = 0\n") == 1
    assert got.shape == (2, 200)
    for i, gamma in enumerate(PRICER_GAMMAS):
        sci = gaussian_kde(x, weights=np.exp(gamma * x))(grid)
        want = sci / np.nansum(sci)
        report(f"Hawkes get_log_return_mc_pdf_device gamma={gamma}", float(np.max(np.abs(got[i] - want)) / want.max()), SCIPY_TOL)
        assert abs(got[i].sum() - 1.0) < 1e-12 and stats[i]["n_kept"] == n
    # the keyword absent: the existing call's bits, and params.risk_premia_gamma still ignored
    absent = pricer.get_log_return_mc_pdf_device(ttm=TTM, params=p, x_grid=grid, nb_path=n, seed=9)
    density = plain_bits(sv, n, (sv.VariableType.LOG_RETURN,), {sv.VariableType.LOG_RETURN: grid})[sv.VariableType.LOG_RETURN]
    assert np.array_equal(absent, density / np.nansum(density))
    ignored = pricer.get_log_return_mc_pdf_device(ttm=TTM, params=dataclasses.replace(p, risk_premia_gamma=1.0), x_grid=grid, nb_path=n, seed=9)
    assert np.array_equal(ignored, absent)


# ---- 8. against the model: the device adds nothing to what the host route gives ---------------------------------------------
@pytest.mark.parametrize("gamma", [1.0, -1.0])
def test_device_kde_is_as_close_to_the_model_density_under_the_kernel_as_the_host_route(sv, gamma):
    """a sanity check, not a parity check (a KDE is biased by its bandwidth): the L1 distance between the normalised weighted KDE of
    the Hawkes x and the normalised Fourier masses under the kernel (hawkesjd_pdf_under_risk_kernel) is only required not to exceed
    what SciPy's weighted estimate of the same sample gives, plus the device-versus-SciPy tolerance.  The one model identity
    asserted: the masses under the kernel sum to one over +-6 standard deviations, up to the grid's truncation and its
    rectangle rule (exponential tails beyond six standard deviations hold less than 1e-2 of the mass)."""
    from scipy.stats import gaussian_kde
    from stochvolmodels_amd.pricers.hawkes_jd_pricer import hawkesjd_pdf_under_risk_kernel
    n = 100_000
    p, pricer, x, grid = hawkes_sample(sv, n, 9)
    got = pricer.get_log_return_mc_pdf_device(ttm=TTM, params=p, x_grid=grid, nb_path=n, seed=9, risk_premia_gamma=gamma)[0]
    sci = gaussian_kde(x, weights=np.exp(gamma * x))(grid)
    host = sci / np.nansum(sci)
    masses = hawkesjd_pdf_under_risk_kernel(p, gamma, TTM, grid)
    model = masses / np.nansum(masses)
    l1_device, l1_host = np.abs(got - model).sum(), np.abs(host - model).sum()
    print(f"KDE-MODEL gamma={gamma}: L1 distance to the Fourier density under the kernel: device {l1_device:.6e}, host SciPy route "
          f"{l1_host:.6e}, device - host {l1_device - l1_host:.3e}; the masses sum to {masses.sum():.6f}")
    assert abs(masses.sum() - 1.0) < 1e-2
    assert l1_device <= l1_host + SCIPY_TOL
