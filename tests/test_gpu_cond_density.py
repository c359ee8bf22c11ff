"""
The mixture density of the simulated log-return on the GPU (include/svmc_est.h; csrc/svmc_est.hip's
cond_density_*_kernel in libsvmc_est.so).

Arithmetic.  No bound is fixed in advance.  On every case, in the same process, the PARENT's unchanged route -- row f18's
svmc_tilted_cond_greeks_chain at F = 1, K = exp(x), no recentring: K dual_gamma and its error -- is run on the same rows and its
deviation from the long-double twin (tests/cond_density_twin.py's direct()) is measured; the new kernels get
    max(4 x that deviation, 32 eps |value|)
per quantity (pdf, its error).  Why this margin: the new kernel rounds one exp where the parent rounds an exp, two CDFs and a
division, so it should sit at or below the parent; the factor 4 covers a different grouping of the sums and the floor the cases
where the parent happens to be exact.  A deviation is the largest |device - twin| / max(|twin|, 1e-290) over a case's points (a
value below 1e-290 is a denormal or 0 on the device and a smaller number yet in the twin's wider range).  New and parent are then
compared directly, within the sum of the two.  SVMC_CD_OBSERVED=<file> appends every case's figures
(profiles/cond_density_observed_tolerances.txt).

Then: the ties to rows f13 (gamma = 0) and f18 (its statistics, bit for bit), bit-equality against the company of a call, the
special cases of the header, the refusals, and the routes.
Shapes: tests/test_cond_density_host.py defines them (and shows on the CPU that the twin drops no path on them).
"""
import ctypes as C
import os

import numpy as np
import pytest

import cmc_twin as ct
import cond_density_twin as cd
from test_cond_density_host import MANY_ROWS, PATH_COUNTS, gamma_counts, gammas_of, inputs, point_counts, points_of, tile_sizes

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = 2.0 ** -52
TINY = 1e-290
XT, GT, GT_WIDE = tile_sizes()
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def largest_deviations():
    """after the module's tests: the largest deviation of each quantity, the parent's beside it (shown with -s)"""
    yield
    for k, (dev, par, where) in sorted(SEEN.items()):
        print(f"\nlargest {k} deviation: new {dev:.3e}  parent {par:.3e}  {where}", end="")
    print()


def deviation(got, want):
    want, got = np.asarray(want, dtype=LD), np.asarray(got, dtype=LD)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), TINY)))


def upload_rows(mus, cvs):
    from stochvolmodels_amd.engine import get_engine
    n, m = mus[0].size, len(mus)
    eng = get_engine(n)
    eng.reserve_snapshots(2 * m)
    for i, (mu, cv) in enumerate(zip(mus, cvs)):
        eng.upload(eng.snapshot_ptr(i), mu)
        eng.upload(eng.snapshot_ptr(m + i), cv)
    return eng


def run_new(mus, cvs, xs, gammas, rows=None):
    """engine.conditional_densities on uploaded rows: expiry i's mu in snapshot row i, its cv in row m + i (or the expiries given)"""
    m = len(mus)
    eng = upload_rows(mus, cvs)
    rows = list(range(m)) if rows is None else rows
    return eng.conditional_densities([xs[i] for i in rows], gammas, mu_rows=rows, cv_rows=[m + i for i in rows])


def run_parent(mus, cvs, xs, gammas):
    """row f18's unchanged route on the same rows -> (pdf [G][m], error [G][m], stats [G, m, 4])"""
    m = len(mus)
    eng = upload_rows(mus, cvs)
    ks = [np.exp(np.asarray(x, dtype=np.float64)) for x in xs]
    greeks, stats = eng.tilted_conditional_greeks([1.0] * m, ks, [np.zeros(k.size, dtype=np.int8) for k in ks], gammas, False,
                                                  mu_rows=list(range(m)), cv_rows=list(range(m, 2 * m)))
    return ([[k * g["dual_gamma"][i] for i, k in enumerate(ks)] for g in greeks],
            [[k * g["dual_gamma_stderr"][i] for i, k in enumerate(ks)] for g in greeks], stats)


def record(line):
    path = os.environ.get("SVMC_CD_OBSERVED")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def check_arithmetic(mus, cvs, xs, gammas, what):
    """the new kernels and the parent against the twin, case by case = (gamma, expiry); returns the new results"""
    new = run_new(mus, cvs, xs, gammas)
    par = run_parent(mus, cvs, xs, gammas)
    for g, gamma in enumerate(gammas):
        for i, (mu, cv) in enumerate(zip(mus, cvs)):
            want_p, want_e, st = cd.direct(mu, cv, xs[i], gamma)
            tag = f"{what} gamma={gamma} expiry={i} n={mu.size} P={np.size(xs[i])} G={len(gammas)}"
            assert new[2][g, i, 1:].tolist() == [st[k] for k in cd.STATS[1:]], (tag, new[2][g, i], st)
            dev_w = abs(LD(new[2][g, i, 0]) - st["sum_weights"]) / st["sum_weights"] if st["n_kept"] else abs(new[2][g, i, 0])
            assert dev_w <= 32 * EPS, (tag, dev_w)
            if np.size(xs[i]) == 0:
                assert new[0][g][i].size == 0 and new[1][g][i].size == 0
                continue
            for name, got, parent, want in (("pdf", new[0][g][i], par[0][g][i], want_p), ("stderr", new[1][g][i], par[1][g][i], want_e)):
                d_new, d_par = deviation(got, want), deviation(parent, want)
                bound = max(4.0 * d_par, 32.0 * EPS)
                d_both = deviation(got, np.asarray(parent, dtype=LD))
                line = f"{tag}: {name} new {d_new:.3e} parent {d_par:.3e} bound {bound:.3e} new-parent {d_both:.3e}"
                print(line)
                record(line)
                if d_new >= SEEN.get(name, (-1.0, 0.0, ""))[0]:
                    SEEN[name] = (d_new, d_par, tag)
                if name == "stderr" and st["n_kept"] == 1:
                    assert np.all(np.ravel(got) == 0.0), tag                       # one kept path gives error 0
                assert d_new <= bound, line
                assert d_both <= bound + d_par, line
    return new


# ---- arithmetic -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", PATH_COUNTS)
def test_arithmetic_over_path_counts(n):
    mu, cv = inputs(n, n)
    check_arithmetic([mu], [cv], [points_of(2 * XT + 3)], gammas_of(min(GT + 1, 16)), "paths")


def test_arithmetic_with_more_than_one_trip_per_block():
    """1024 x 256 + 3 paths: quote_rows' cap, every block a full trip and three lanes one more"""
    mu, cv = inputs(MANY_ROWS, MANY_ROWS)
    check_arithmetic([mu], [cv], [points_of(XT + 1)], gammas_of(2), "many rows")


@pytest.mark.parametrize("count", point_counts())
def test_arithmetic_over_point_counts(count):
    mu, cv = inputs(257, 11)
    check_arithmetic([mu], [cv], [points_of(count, count)], gammas_of(2), "points")


@pytest.mark.parametrize("count", gamma_counts())
def test_arithmetic_over_gamma_counts(count):
    mu, cv = inputs(1000, 12)
    check_arithmetic([mu], [cv], [points_of(XT + 1)], gammas_of(count), "gammas")


def three_expiries(n=257):
    rows = [inputs(n, 20 + i) for i in range(3)]
    return [r[0] for r in rows], [r[1] for r in rows], [points_of(2 * XT + 3, 1), np.zeros(0), points_of(max(XT - 1, 1), 2)]


def test_arithmetic_over_three_expiries_one_without_points():
    mus, cvs, xs = three_expiries()
    new = check_arithmetic(mus, cvs, xs, gammas_of(min(GT + 1, 16)), "three expiries")
    assert new[2].shape == (min(GT + 1, 16), 3, 5) and np.all(new[2][:, 1, 1] == 257)     # the empty expiry's statistics are returned


# ---- ties ---------------------------------------------------------------------------------------------------------------------------
def test_gamma_zero_is_row_f13s_k_dual_gamma():
    mu, cv = inputs(1000, 31)
    x = points_of(2 * XT + 3)
    k = np.exp(x)
    pdf, err, _ = run_new([mu], [cv], [x], [0.0])
    eng = upload_rows([mu], [cv])
    f13, _ = eng.conditional_greeks([1.0], [1.0], [k], [np.zeros(k.size, dtype=np.int8)], False, mu_rows=[0], cv_rows=[1])
    want_p, want_e, _ = cd.direct(mu, cv, x, 0.0)
    for name, got, other, want in (("pdf", pdf[0][0], k * f13["dual_gamma"][0], want_p), ("stderr", err[0][0], k * f13["dual_gamma_stderr"][0], want_e)):
        d_new, d_13 = deviation(got, want), deviation(other, want)
        d_both = deviation(got, np.asarray(other, dtype=LD))
        print(f"gamma = 0 against row f13: {name} new {d_new:.3e} f13 {d_13:.3e} new-f13 {d_both:.3e}")
        assert d_new <= max(4.0 * d_13, 32.0 * EPS) and d_both <= max(4.0 * d_13, 32.0 * EPS) + d_13


def test_statistics_are_row_f18s_bits():
    mus, cvs, xs = three_expiries()
    cvs[0][::7] = 0.0                                        # point masses: counted, and their weight enters sum W
    mus[2][5], cvs[2][9] = np.nan, -1.0                      # dropped by f11's rule
    gammas = gammas_of(min(GT + 1, 16))
    _, _, st = run_new(mus, cvs, xs, gammas)
    _, _, st18 = run_parent(mus, cvs, xs, gammas)
    assert np.all(st[:, :, 4] == 0)
    for col_new, col_18 in ((0, 0), (1, 1), (2, 2), (3, 3)):                       # sum W, n_kept, n_dropped, n_zero_cv
        assert np.array_equal(st[:, :, col_new], st18[:, :, col_18]), (col_new, st[:, :, col_new], st18[:, :, col_18])
    assert np.all(st[:, 0, 3] == np.sum(cvs[0] == 0.0)) and np.all(st[:, 2, 2] == 2)


# ---- bit-equality -------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_company_of_a_call():
    mus, cvs, xs = three_expiries()
    gammas = gammas_of(16)
    pdf, err, st = run_new(mus, cvs, xs, gammas)
    # fewer gammas: any subset, in any order, across the tiles
    # (up to GT gammas go through the narrow tile's kernel, more through the wide tile's: the same bits)
    for pick in ([0], [GT % 16], [15, 3, 0], list(range(GT)), list(range(1, 16, 2)), list(range(min(GT + 1, 16))), list(range(min(GT_WIDE + 1, 16)))):
        p2, e2, s2 = run_new(mus, cvs, xs, [gammas[j] for j in pick])
        for a, j in enumerate(pick):
            assert np.array_equal(s2[a], st[j])
            for i in range(3):
                assert np.array_equal(p2[a][i], pdf[j][i]) and np.array_equal(e2[a][i], err[j][i]), (pick, j, i)
    # fewer expiries
    for rows in ([0], [2], [2, 0], [1]):
        p2, e2, s2 = run_new(mus, cvs, xs, gammas, rows=rows)
        for a, i in enumerate(rows):
            assert np.array_equal(s2[:, a], st[:, i])
            for j in range(16):
                assert np.array_equal(p2[j][a], pdf[j][i]) and np.array_equal(e2[j][a], err[j][i]), (rows, j, i)
    # fewer points, other groups: every point alone, and the grid reversed
    x0 = xs[0]
    for sub in ([x0[:1]] + [x0[j:j + 1] for j in (XT - 1, XT, x0.size - 1)] + [x0[::-1].copy(), x0[1::2].copy()]):
        p2, e2, _ = run_new(mus, cvs, [sub, xs[1], xs[2]], gammas)
        idx = [int(np.where(x0 == v)[0][0]) for v in sub]
        for j in range(16):
            assert np.array_equal(p2[j][0], pdf[j][0][idx]) and np.array_equal(e2[j][0], err[j][0][idx])
            assert np.array_equal(p2[j][2], pdf[j][2])


# ---- special cases ------------------------------------------------------------------------------------------------------------------
def test_a_weight_that_overflows_at_one_gamma_only():
    mu, cv = inputs(257, 41)
    mu[100] = 130.0                                          # exp(3 x 130)^2 overflows, exp(2 x 130)^2 does not
    x = points_of(XT + 1)
    gammas = [-1.0, 3.0, 0.0, 2.0, 0.5]
    pdf, err, st = run_new([mu], [cv], [x], gammas)
    assert st[:, 0, 4].tolist() == [0, 1, 0, 0, 0] and np.all(st[:, 0, 1] == 257) and np.all(st[:, 0, 2] == 0)
    assert np.all(np.isnan(pdf[1][0])) and np.all(np.isnan(err[1][0])) and np.isfinite(st[1, 0, 0])
    others = [0, 2, 3, 4]
    p2, e2, s2 = run_new([mu], [cv], [x], [gammas[j] for j in others])
    for a, j in enumerate(others):
        assert np.all(np.isfinite(pdf[j][0])) and np.all(np.isfinite(err[j][0]))
        assert np.array_equal(p2[a][0], pdf[j][0]) and np.array_equal(e2[a][0], err[j][0]) and np.array_equal(s2[a], st[j])
        want_p, want_e, wst = cd.direct(mu, cv, x, gammas[j])
        assert deviation(pdf[j][0], want_p) <= 1e-12 and wst["n_weight_dropped"] == 0
    assert cd.stats_of(mu, cv, 3.0)["n_weight_dropped"] == 1
    # row f18 still serves that gamma: it drops the path and re-sums
    pp, _, st18 = run_parent([mu], [cv], [x], [3.0])
    assert np.all(np.isfinite(pp[0][0])) and st18[0, 0, 1] == 256


def test_paths_failing_f11s_rule_are_dropped_for_all_gammas_and_counted():
    mu, cv = inputs(257, 42)
    mu[3], mu[77], cv[200], cv[201], mu[256] = np.nan, np.inf, -1e-3, np.inf, 800.0
    assert int(np.sum(~ct.keep_mask(mu, cv))) == 5
    x = points_of(XT + 1)
    gammas = gammas_of(min(GT + 1, 16))
    pdf, err, st = run_new([mu], [cv], [x], gammas)
    assert np.all(st[:, 0, 1] == 252) and np.all(st[:, 0, 2] == 5) and np.all(st[:, 0, 4] == 0)
    keep = ct.keep_mask(mu, cv)
    p2, e2, s2 = run_new([mu[keep]], [cv[keep]], [x], gammas)
    for g, gamma in enumerate(gammas):
        want_p, want_e, _ = cd.direct(mu, cv, x, gamma)
        assert deviation(pdf[g][0], want_p) <= 1e-12 and deviation(err[g][0], want_e) <= 1e-12
        assert deviation(pdf[g][0], p2[g][0]) <= 1e-13       # (another order of the sums: the kept paths alone)


def test_all_point_masses_and_every_path_dropped():
    n = 257
    mu = inputs(n, 43)[0]
    x = points_of(XT + 1)
    pdf, err, st = run_new([mu], [np.zeros(n)], [x], [0.0, 1.0])
    for g in range(2):
        assert np.all(pdf[g][0] == 0.0) and np.all(err[g][0] == 0.0)
        assert st[g, 0, 1:].tolist() == [n, 0, n, 0] and st[g, 0, 0] > 0
    pdf, err, st = run_new([np.full(n, np.nan)], [np.full(n, 0.04)], [x], [0.0, 1.0])   # status OK: the call returns
    for g in range(2):
        assert np.all(np.isnan(pdf[g][0])) and np.all(np.isnan(err[g][0]))
        assert st[g, 0].tolist() == [0.0, 0, n, 0, 0]


def test_identical_paths_have_errors_of_zero_to_rounding():
    """identical paths: the estimate is every path's value and its error is zero in exact arithmetic.  The error is the root of
    e^{2 gamma x} S2 - 2 pdf e^{gamma x} C + pdf^2 sum W^2, a difference of three sums of n equal terms, each carrying up to
    log2(n) + 3 <= 16 roundings: up to 3 x 16 x 2^-53 = 5.4e-15 of n (W v)^2 is left, so the error is below
    sqrt(5.4e-15 n) W v / (n W) < 1e-7 v / sqrt(n) -- the bound of row f18's test of this name, v the path's Gaussian under the kernel"""
    x = np.array([-0.4, -0.03, 0.0, 0.2, 0.5])
    gammas = [-3.0, -1.0, 0.0, 0.5, 3.0]
    for n in (2, 257, 4099):
        mu, cv = np.full(n, -0.03), np.full(n, 0.0225)
        pdf, err, _ = run_new([mu], [cv], [x], gammas)
        for g, gamma in enumerate(gammas):
            want, _, _ = cd.direct(mu[:1], cv[:1], x, gamma)
            assert deviation(pdf[g][0], want) <= 1e-13
            ratio = float(np.max(err[g][0] / (1e-7 * np.asarray(want, dtype=np.float64) / np.sqrt(n) + 1e-300)))
            print(f"identical paths n={n} gamma={gamma}: largest error / bound {ratio:.3e}")
            assert ratio <= 1.0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_code_and_leaves_the_outputs_untouched():
    from stochvolmodels_amd import _lib
    E = _lib.load_est()
    n, m = 257, 2
    mus, cvs, _ = three_expiries(n)
    eng = upload_rows(mus[:2], cvs[:2])
    x, offs, g = np.array([-0.1, 0.1, 0.3]), np.array([0, 2, 3], dtype=np.uintp), np.array([0.5, -1.0])
    P, G = 3, 2
    nbytes = C.c_size_t(0)
    assert E.svmc_cond_density_workspace_bytes(n, m, P, G, C.byref(nbytes)) == _lib.OK
    ws_ptr, _ = eng.alloc_sums((nbytes.value + 7) // 8, "cond_density_workspace")
    pdf, err, stats = np.full(G * P, -7.0), np.full(G * P, -7.0), np.full(G * m * 5, -7.0)
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    rows_mu, rows_cv = (vp * 2)(eng.snapshot_ptr(0), eng.snapshot_ptr(1)), (vp * 2)(eng.snapshot_ptr(2), eng.snapshot_ptr(3))

    def call(rows_mu=rows_mu, rows_cv=rows_cv, n_path=n, n_exp=m, points=x, offsets=offs, gammas=g, ng=G, out=pdf, out_err=err,
             st=stats, workspace=ws_ptr, ws_bytes=nbytes.value):
        a = lambda v, t: None if v is None else v.ctypes.data_as(t)      # noqa: E731
        return E.svmc_cond_density_chain(rows_mu, rows_cv, n_path, n_exp, a(points, dp), a(offsets, C.POINTER(C.c_size_t)), a(gammas, dp),
                                         ng, a(out, dp), a(out_err, dp), a(st, dp), workspace, ws_bytes, eng.stream)

    for kw in (dict(rows_mu=None), dict(rows_cv=None), dict(points=None), dict(offsets=None), dict(gammas=None), dict(out=None),
               dict(out_err=None), dict(st=None), dict(workspace=None), dict(rows_mu=(vp * 2)(eng.snapshot_ptr(0), None)),
               dict(rows_cv=(vp * 2)(None, eng.snapshot_ptr(3))), dict(n_path=0), dict(n_exp=0), dict(ng=0), dict(ng=17),
               dict(offsets=np.array([1, 2, 3], dtype=np.uintp)), dict(offsets=np.array([0, 3, 2], dtype=np.uintp)),
               dict(gammas=np.array([0.5, np.nan])), dict(gammas=np.array([np.inf, 0.5])), dict(points=np.array([0.1, np.nan, 0.2])),
               dict(points=np.array([0.1, 0.2, -np.inf]))):
        assert call(**kw) == _lib.ERR_INVALID_ARGUMENT, kw
    assert call(ws_bytes=nbytes.value - 8) == _lib.ERR_WORKSPACE
    assert np.all(pdf == -7.0) and np.all(err == -7.0) and np.all(stats == -7.0)
    assert call() == _lib.OK and not np.any(pdf == -7.0) and not np.any(stats == -7.0)
    want = run_new(mus[:2], cvs[:2], [x[:2], x[2:]], g)
    assert np.array_equal(pdf.reshape(G, P), np.array([np.concatenate(p) for p in want[0]]))
    assert np.array_equal(stats.reshape(G, m, 5), want[2])


# ---- routes -------------------------------------------------------------------------------------------------------------------------
ROUTE_N, ROUTE_TTM, ROUTE_GAMMAS, ROUTE_SPY = 4096, 0.25, (-1.0, 0.0, 1.0), 48
ROUTE_X = np.linspace(-0.6, 0.5, 16).reshape(2, 8)


def route_bound(mu, cv, x, gamma, d_parent):
    """the arithmetic section's combined bound (the new kernels' and the parent's) times the identity's condition factor"""
    cond = cd.condition(mu, cv, np.ravel(x), gamma)
    return (max(4.0 * d_parent, 32.0 * EPS) + d_parent) * float(np.max(cond))


def check_route(pricer, params, conditional_state, what):
    """get_log_return_mc_pdf_mixture at one seed: the stepped rows are the conditional pricer's, the result is the Greeks-route density
    on those rows (the host-array route compute_mc_vars_greeks_conditional_with_gamma) within route_bound"""
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.engine import get_engine
    seed = 17
    pdf, err, stats = pricer.get_log_return_mc_pdf_mixture(params, ROUTE_TTM, ROUTE_X, risk_premia_gammas=ROUTE_GAMMAS, nb_path=ROUTE_N,
                                                           seed=seed, return_stderr=True, return_stats=True, nb_steps=ROUTE_SPY)
    assert pdf.shape == (3,) + ROUTE_X.shape == err.shape and len(stats) == 3
    eng = get_engine(ROUTE_N)
    rows = eng.download(eng.snapshot_ptr(0), 2 * ROUTE_N).reshape(2, ROUTE_N).copy()
    mu_c, cv_c = conditional_state(seed)                     # the conditional pricer's state at the same seed
    assert np.array_equal(rows[0], mu_c) and np.array_equal(rows[1], cv_c), what
    # without gammas: gamma 0 in x_grid's shape, the same bits
    one = pricer.get_log_return_mc_pdf_mixture(params, ROUTE_TTM, ROUTE_X, nb_path=ROUTE_N, seed=seed, nb_steps=ROUTE_SPY)
    assert one.shape == ROUTE_X.shape and np.array_equal(one, pdf[1])
    assert all(s["n_kept"] == ROUTE_N and s["n_weight_dropped"] == 0 for s in stats)
    k = np.exp(ROUTE_X)
    ref = sv.compute_mc_vars_greeks_conditional_with_gamma(rows[0], rows[1], 1.0, k, np.full(k.shape, "C"), list(ROUTE_GAMMAS))
    for g, gamma in enumerate(ROUTE_GAMMAS):
        want_p, want_e, _ = cd.direct(rows[0], rows[1], np.ravel(ROUTE_X), gamma)
        for name, got, parent, want in (("pdf", pdf[g], k * ref[g]["dual_gamma"], want_p), ("stderr", err[g], k * ref[g]["dual_gamma_stderr"], want_e)):
            d_par = deviation(np.ravel(parent), want)
            d_both = deviation(np.ravel(got), np.asarray(np.ravel(parent), dtype=LD))
            bound = route_bound(rows[0], rows[1], ROUTE_X, gamma, d_par)
            print(f"{what} gamma={gamma}: {name} new-parent {d_both:.3e} parent-twin {d_par:.3e} bound {bound:.3e}")
            assert d_both <= bound, (what, gamma, name)
    return pdf, err, stats, rows


def test_logsv_route():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.engine import get_engine
    pricer, params = sv.LogSVPricer(), sv.LOGSV_BTC_PARAMS

    def conditional_state(seed):
        sv.logsv_mc_chain_pricer_conditional(
            ttms=np.array([ROUTE_TTM]), forwards=np.array([1.0]), discfactors=np.array([1.0]), strikes_ttms=[np.array([1.0])],
            optiontypes_ttms=[np.array(["C"])], v0=params.sigma0, theta=params.theta, kappa1=params.kappa1, kappa2=params.kappa2,
            beta=params.beta, volvol=params.volvol, vol_backbone_etas=params.get_vol_backbone_etas(ttms=np.array([ROUTE_TTM])),
            nb_path=ROUTE_N, nb_steps_per_year=ROUTE_SPY, seed=seed)
        mu, cv, _, _ = get_engine(ROUTE_N).get_state_cmc()
        return mu, cv
    check_route(pricer, params, conditional_state, "logsv route")


def test_heston_route():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.engine import get_engine
    pricer, params = sv.HestonPricer(), sv.HestonParams(v0=0.3, theta=0.4, kappa=2.0, rho=-0.5, volvol=0.8)

    def conditional_state(seed):
        sv.heston_mc_chain_pricer_conditional(
            ttms=np.array([ROUTE_TTM]), forwards=np.array([1.0]), discfactors=np.array([1.0]), strikes_ttms=[np.array([1.0])],
            optiontypes_ttms=[np.array(["C"])], v0=params.v0, theta=params.theta, kappa=params.kappa, rho=params.rho,
            volvol=params.volvol, nb_path=ROUTE_N, nb_steps_per_year=ROUTE_SPY, seed=seed)
        mu, cv, _, _ = get_engine(ROUTE_N).get_state_cmc()
        return mu, cv
    check_route(pricer, params, conditional_state, "heston route")


def test_hawkes_route_is_the_greeks_route_density():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.engine import get_engine
    pricer, params = sv.HawkesJDPricer(), sv.HawkesJDParams()
    box = {}

    def conditional_state(seed):
        # the existing Greeks-route density at the same seed: its stepping call leaves the same rows
        box["pdf"], box["err"] = pricer.get_log_return_mc_pdf_conditional_under_risk_kernel(
            params, ROUTE_TTM, ROUTE_X, list(ROUTE_GAMMAS), nb_path=ROUTE_N, seed=seed, return_stderr=True, nb_steps_per_year=ROUTE_SPY)
        eng = get_engine(ROUTE_N)
        rows = eng.download(eng.snapshot_ptr(0), 2 * ROUTE_N).reshape(2, ROUTE_N)
        return rows[0].copy(), rows[1].copy()
    pdf, err, stats, rows = check_route(pricer, params, conditional_state, "hawkes route")
    for g, gamma in enumerate(ROUTE_GAMMAS):
        want_p, want_e, _ = cd.direct(rows[0], rows[1], np.ravel(ROUTE_X), gamma)
        for got, parent, want in ((pdf[g], box["pdf"][g], want_p), (err[g], box["err"][g], want_e)):
            d_par = deviation(np.ravel(parent), want)
            assert deviation(np.ravel(got), np.asarray(np.ravel(parent), dtype=LD)) <= route_bound(rows[0], rows[1], ROUTE_X, gamma, d_par)


def test_hawkes_without_jumps_is_the_closed_form_tilted_gaussian():
    """zero intensities, zero long-run levels: no jump ever, every path has mu = (mu - sigma^2 / 2) T and the density under the kernel
    is N(x; mu + gamma cv, cv), cv = sigma^2 T.  The stepped mu carries the roundings of its nb additions, and the density's relative
    sensitivity to mu is |z| / sd: bound 32 eps x the identity's condition + (|z| / sd) nb eps |mu|"""
    import stochvolmodels_amd as sv
    params = sv.HawkesJDParams(lambda_p=0.0, lambda_m=0.0, theta_p=0.0, theta_m=0.0, mu=0.03, sigma=0.4)
    n = 1000
    pdf, err, stats = sv.HawkesJDPricer().get_log_return_mc_pdf_mixture(params, ROUTE_TTM, ROUTE_X, risk_premia_gammas=ROUTE_GAMMAS,
                                                                        nb_path=n, seed=3, return_stderr=True, return_stats=True,
                                                                        nb_steps=ROUTE_SPY)
    nb = int(ROUTE_TTM * ROUTE_SPY) + 1
    cv, m0 = LD(0.4) ** 2 * LD(ROUTE_TTM), (LD(0.03) - LD(0.4) ** 2 / 2) * LD(ROUTE_TTM)
    sd = np.sqrt(cv)
    for g, gamma in enumerate(ROUTE_GAMMAS):
        z = (ROUTE_X.astype(LD) - (m0 + LD(gamma) * cv)) / sd
        want = np.exp(-z * z / 2) / (sd * cd.SQRT_2PI)
        cond = 1.0 + abs(gamma) * abs(float(m0)) + gamma * gamma * float(cv) / 2 + np.abs(gamma * ROUTE_X) + np.asarray(z * z / 2, dtype=float)
        bound = 32 * EPS * cond + np.asarray(np.abs(z) / sd, dtype=float) * nb * EPS * abs(float(m0))
        dev = np.asarray(np.abs(pdf[g].astype(LD) - want) / want, dtype=float)
        print(f"no jumps gamma={gamma}: largest deviation / bound {float(np.max(dev / bound)):.3e}")
        assert np.all(dev <= bound)
        assert np.all(err[g] <= 1e-7 * pdf[g] / np.sqrt(n))                        # identical paths
        assert stats[g]["n_kept"] == n and stats[g]["n_zero_cv"] == 0


def test_host_array_route():
    import stochvolmodels_amd as sv
    mu, cv = inputs(1000, 51)
    x = points_of(6).reshape(2, 3)
    pdf, err, st = sv.compute_mc_vars_pdf_conditional(mu, cv, x, return_stderr=True, return_stats=True)
    want_p, want_e, wst = cd.direct(mu, cv, np.ravel(x), 0.0)
    assert pdf.shape == x.shape == err.shape and deviation(np.ravel(pdf), want_p) <= 1e-13 and deviation(np.ravel(err), want_e) <= 1e-12
    assert {k: st[k] for k in cd.STATS[1:]} == {k: wst[k] for k in cd.STATS[1:]}
    many = sv.compute_mc_vars_pdf_conditional(mu, cv, x, gammas=[0.5, 0.0])
    assert many.shape == (2,) + x.shape and np.array_equal(many[1], pdf)
    flat = sv.compute_mc_vars_pdf_conditional(np.zeros(64), 0.04, np.array([0.0]), gammas=[1.0])    # a scalar cv: N(0; 0.04, 0.04)
    assert abs(flat[0, 0] - np.exp(-0.02) / np.sqrt(2 * np.pi * 0.04)) <= 1e-14
