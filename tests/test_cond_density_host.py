"""
The mixture density of the simulated log-return (include/svmc_est.h's svmc_cond_density_chain) without a GPU:
  1. tests/cond_density_twin.py's direct() -- the estimator in numpy.longdouble with no identity used -- against its sums_form(), the
     header's statement, and the degenerate cases of both;
  2. direct() against the long-double twin of row f18's K dual_gamma and of its error (tests/tilted_cond_greeks_twin.py's estimator,
     the one tests/test_tilted_cond_greeks_host.py holds to mpmath) on inputs with no dropped path.  Tolerance 1e-15 relative, scaled
     by cond_density_twin.condition(): 1 + |gamma| max|mu| + gamma^2 max cv / 2 + |gamma x| + z^2 / 2, the condition of the identity
     in extended precision (row f18's twin rounds its density's exponential to double: 1.1e-16);
  3. the twin sees a wrong term: without -2 pdf e^{gamma x} C, or with sum W for sum W^2, the error leaves that tolerance by orders of
     magnitude;
  4. the host-only entry and the refusals of the chain entry, sentinel-filled outputs untouched;
  5. the Python routes' refusals with no library loaded;
  6. the header declares the two names and _lib._declare_est binds them.
Checks 1 to 3 validate the SPECIFICATION; 4 to 6 and tests/test_gpu_cond_density.py fail without the feature.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cond_density_twin as cd  # noqa: E402
import tilted_cond_greeks_twin as tg  # noqa: E402
import tilted_cond_twin as tc  # noqa: E402

LD = np.longdouble
IDENTITY_TOL = 1e-15
GAMMAS = [-3.0, -1.0, 0.0, 0.5, 3.0]


def inputs(n, seed):
    """the GPU test's inputs: mu ~ N(0, 0.2^2), cv in [1e-4, 0.3] (log-uniform, so that small variances are met)"""
    rng = np.random.default_rng(seed)
    return 0.2 * rng.standard_normal(n), np.exp(rng.uniform(np.log(1e-4), np.log(0.3), n))


# ---- the shapes and inputs of tests/test_gpu_cond_density.py, defined here so that their twin can be looked at without a GPU ---------
def tile_sizes():
    """(XT, GT, GT_WIDE): the points a thread holds and the gammas of a tile -- the tile of calls of up to GT gammas, and the tile of
    calls of more: two instances of the main kernel --, read off the source"""
    src = open(os.path.join(ROOT, "stochvolmodels_amd", "csrc", "svmc_est.hip")).read()
    return tuple(int(re.search(r"#define %s (\d+)" % name, src).group(1)) for name in ("SVMC_CD_XT", "SVMC_CD_GT", "SVMC_CD_GT_WIDE"))


PATH_COUNTS = [1, 2, 255, 256, 257, 1000]
MANY_ROWS = 1024 * 256 + 3             # every one of the 1024 path blocks makes a full trip and three lanes of the first one more
GAMMA_POOL = [-3.0, 0.5, 0.0, -1.0, 3.0, 2.0, -2.0, 1.0, -0.5, 1.5, -1.5, 2.5, -2.5, 0.25, -0.25, 2.75]


def gammas_of(count):
    return GAMMA_POOL[:count]


def points_of(count, seed=0):
    """count points in [-1, 1]: the ends and the points between them shifted off the lattice"""
    if count == 1:
        return np.array([0.3])
    x = np.linspace(-1.0, 1.0, count)
    x[1:-1] += np.random.default_rng(900 + seed).uniform(-0.4, 0.4, count - 2) / count
    return x


def point_counts():
    xt = tile_sizes()[0]
    return sorted({1, max(xt - 1, 1), xt, xt + 1, 2 * xt + 3})


def gamma_counts():
    """1, 2, a full tile and one more of either tile size (GT + 1 is also the first count the wide tile's kernel serves), 16"""
    _, gt, wide = tile_sizes()
    return sorted({1, 2, gt, min(gt + 1, 16), wide, min(wide + 1, 16), 16})


def test_the_gpu_tests_inputs_drop_no_path_in_the_twin():
    """mu ~ N(0, 0.2^2), cv in [1e-4, 0.3], x in [-1, 1], gammas in [-3, 3]: no path fails f11's rule or loses its weight, at any of
    the path counts, and row f18's twin drops none either"""
    assert len(GAMMA_POOL) == 16 and min(GAMMA_POOL) == -3.0 and max(GAMMA_POOL) == 3.0 and len(set(GAMMA_POOL)) == 16
    assert 0.0 in gammas_of(min(tile_sizes()[1], 16)) or tile_sizes()[1] < 3
    for n in PATH_COUNTS + [MANY_ROWS]:
        mu, cv = inputs(n, n)
        assert cv.min() >= 1e-4 and cv.max() <= 0.3
        for gamma in GAMMA_POOL:
            st = cd.stats_of(mu, cv, gamma)
            assert (st["n_kept"], st["n_dropped"], st["n_weight_dropped"], st["n_zero_cv"]) == (n, 0, 0, 0)
            assert np.all(tc.keep_mask(mu, cv, 1.0, gamma))
    for c in point_counts():
        x = points_of(c)
        assert x.size == c and x.min() >= -1.0 and x.max() <= 1.0 and np.unique(x).size == c


def strikes_and_points(n_points):
    """strikes K as doubles and x = ln K in LONG DOUBLE: both twins then see the same point to 2^-64, where x = fl(ln K) in double
    would differ from ln K by 1e-16 / sd in z"""
    k = np.exp(np.linspace(-1.0, 1.0, n_points))
    return k, np.log(k.astype(LD))


def rel(a, b, cond):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b) / (np.abs(b) * cond)))


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 257])
def test_direct_form_equals_the_headers_sums(n):
    mu, cv = inputs(n, 3 + n)
    cv[::5] = 0.0 if n > 2 else cv[::5]
    x = np.linspace(-1.0, 1.0, 9)
    for gamma in GAMMAS:
        p, e, st = cd.direct(mu, cv, x, gamma)
        q, f, st2 = cd.sums_form(mu, cv, x, gamma)
        assert st == st2 and st["n_dropped"] == 0 and st["n_weight_dropped"] == 0
        cond = cd.condition(mu, cv, x, gamma)
        assert rel(q, p, cond) <= IDENTITY_TOL, (n, gamma)
        if n == 1:
            assert np.all(e == 0) and np.all(f == 0)         # one kept path gives error 0
        else:
            assert rel(f, e, cond) <= 1e-13, (n, gamma)      # (the sums form takes the error as a difference of sums)


def test_degenerate_cases_of_the_twin():
    x = np.array([-0.5, 0.0, 0.25])
    # all cv == 0: the pdf is 0, every path a point mass
    p, e, st = cd.direct(np.array([0.1, -0.2, 0.0]), 0.0, x, 1.0)
    assert np.all(p == 0) and np.all(e == 0) and st["n_zero_cv"] == 3 and st["n_kept"] == 3 and st["sum_weights"] > 0
    # paths failing f11's rule are dropped for every gamma and counted
    mu, cv = np.array([0.1, np.nan, 0.2, 800.0, 0.0]), np.array([0.04, 0.04, -1.0, 0.04, np.inf])
    for gamma in (0.0, -1.0):
        p, e, st = cd.direct(mu, cv, x, gamma)
        assert (st["n_kept"], st["n_dropped"]) == (1, 4) and np.all(e == 0) and np.all(np.isfinite(p.astype(float)))
    # every path dropped: NaN
    p, e, st = cd.direct(np.array([np.nan, np.inf]), np.array([0.1, 0.1]), x, 0.5)
    assert np.all(np.isnan(p)) and np.all(np.isnan(e)) and st["n_kept"] == 0 and st["sum_weights"] == 0
    # a weight whose square overflows at ONE gamma: that gamma is NaN and says how many, the other is served
    mu, cv = np.array([0.1, 300.0, -0.1]), np.array([0.04, 0.04, 0.04])
    p, e, st = cd.direct(mu, cv, x, 2.0)
    assert np.all(np.isnan(p)) and np.all(np.isnan(e)) and st["n_weight_dropped"] == 1 and st["n_kept"] == 3
    p, e, st = cd.direct(mu, cv, x, 0.5)
    assert np.all(np.isfinite(p.astype(float))) and st["n_weight_dropped"] == 0
    for mut in cd.MUTATIONS:
        assert np.all(np.isnan(cd.sums_form(mu, cv, x, 2.0, mut)[0]))


# ---- 2, 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 257, 1000])
def test_direct_form_equals_row_f18s_k_dual_gamma_and_its_error(n):
    """(Not at a handful of paths: where two paths' Gaussians cross, v_1 = v_2 = pdf and the error of two paths is the rounding of
    v_j - pdf in EITHER twin -- at n = 2 the two errors differ by 4e-15 of the condition at one point -- which is the condition of an
    error of two paths, not of the identity.  Small path counts are held in test_direct_form_equals_the_headers_sums.)"""
    mu, cv = inputs(n, 40 + n)
    k, x = strikes_and_points(11)
    worst = 0.0
    for gamma in GAMMAS:
        assert np.all(tc.keep_mask(mu, cv, 1.0, gamma))      # row f18 drops no path on these inputs
        g, st18 = tg.estimator(mu, cv, 1.0, k, ["C"] * k.size, gamma, False, with_price=False)
        p, e, st = cd.direct(mu, cv, x, gamma)
        assert (st["n_kept"], st["n_dropped"], st["n_zero_cv"], st["n_weight_dropped"]) == (n, 0, 0, 0)
        assert (st18["n_kept"], st18["n_zero_cv"]) == (n, 0)
        assert abs(st["sum_weights"] - st18["sum_weights"]) <= 1e-18 * abs(st18["sum_weights"]) * n
        cond = cd.condition(mu, cv, x, gamma)
        dp, de = rel(p, k.astype(LD) * g["dual_gamma"], cond), rel(e, k.astype(LD) * g["dual_gamma_stderr"], cond)
        worst = max(worst, dp, de)
        assert dp <= IDENTITY_TOL and de <= IDENTITY_TOL, (n, gamma, dp, de)
    print(f"n={n}: direct form against row f18's twin, worst deviation / condition {worst:.2e} (tolerance {IDENTITY_TOL:.0e})")


@pytest.mark.parametrize("mutation", cd.MUTATIONS)
def test_the_twin_sees_a_wrong_term(mutation):
    mu, cv = inputs(64, 77)
    k, x = strikes_and_points(7)
    seen = []
    for gamma in (-3.0, 0.5, 3.0):                           # (at gamma = 0 sum W = sum W^2 = n)
        g, _ = tg.estimator(mu, cv, 1.0, k, ["C"] * k.size, gamma, False, with_price=False)
        want = k.astype(LD) * g["dual_gamma_stderr"]
        cond = cd.condition(mu, cv, x, gamma)
        _, good, _ = cd.sums_form(mu, cv, x, gamma)
        assert rel(good, want, cond) <= 1e-13                # (the sums form takes the error as a difference of sums)
        pdf, bad, _ = cd.sums_form(mu, cv, x, gamma, mutation)
        assert rel(pdf, k.astype(LD) * g["dual_gamma"], cond) <= IDENTITY_TOL      # the value does not depend on the term
        seen.append(rel(bad, want, cond))
        assert seen[-1] >= 1e6 * IDENTITY_TOL, (mutation, gamma, seen[-1])
    print(f"{mutation}: error off by {min(seen):.1e} .. {max(seen):.1e} of the condition-scaled value")


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def test_host_only_entry_and_refusals_without_a_gpu():
    from stochvolmodels_amd import _lib
    E = _lib.load_est()
    nbytes = C.c_size_t(0)
    assert E.svmc_cond_density_workspace_bytes(257, 2, 24, 5, C.byref(nbytes)) == _lib.OK and nbytes.value > 0
    small = nbytes.value
    assert small >= 2 * 5 * 257 * 8                          # a row of weights per (expiry, gamma)
    assert E.svmc_cond_density_workspace_bytes(1 << 20, 2, 24, 5, C.byref(nbytes)) == _lib.OK and nbytes.value > small
    assert E.svmc_cond_density_workspace_bytes(257, 2, 0, 1, C.byref(nbytes)) == _lib.OK and nbytes.value > 0
    for args in ((0, 2, 24, 5), (257, 0, 24, 5), (257, 2, 24, 0), (257, 2, 24, 17)):
        assert E.svmc_cond_density_workspace_bytes(*args, C.byref(nbytes)) == _lib.ERR_INVALID_ARGUMENT
    assert E.svmc_cond_density_workspace_bytes(257, 2, 24, 5, None) == _lib.ERR_INVALID_ARGUMENT
    # the chain entry refuses before it touches the device: null pointers, sizes, offsets, values, the workspace's size
    n, m, P, G = 64, 1, 2, 1
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    x, g, offs = np.array([-0.1, 0.1]), np.array([0.5]), np.array([0, 2], dtype=np.uintp)
    pdf, err, stats = np.full(G * P, -7.0), np.full(G * P, -7.0), np.full(G * m * 5, -7.0)
    rows = (vp * 1)(0x1000)                                  # never dereferenced: every call below is refused first
    ws = vp(0x1000)

    def call(rows_mu=rows, rows_cv=rows, n_path=n, n_exp=m, points=x, offsets=offs, gammas=g, ng=G, out=pdf, out_err=err, st=stats,
             workspace=ws, ws_bytes=8):
        a = lambda v, t: None if v is None else v.ctypes.data_as(t)      # noqa: E731
        return E.svmc_cond_density_chain(rows_mu, rows_cv, n_path, n_exp, a(points, dp), a(offsets, C.POINTER(C.c_size_t)), a(gammas, dp),
                                         ng, a(out, dp), a(out_err, dp), a(st, dp), workspace, ws_bytes, None)

    assert call() == _lib.ERR_WORKSPACE
    two = (vp * 2)(0x1000, 0x1000)
    for kw in (dict(rows_mu=None), dict(rows_cv=None), dict(points=None), dict(offsets=None), dict(gammas=None), dict(out=None),
               dict(out_err=None), dict(st=None), dict(workspace=None), dict(rows_mu=(vp * 1)(None)), dict(rows_cv=(vp * 1)(None)),
               dict(n_path=0), dict(n_exp=0), dict(ng=0), dict(ng=17), dict(offsets=np.array([1, 2], dtype=np.uintp)),
               dict(offsets=np.array([0, 2, 1], dtype=np.uintp), n_exp=2, rows_mu=two, rows_cv=two),
               dict(gammas=np.array([np.nan])), dict(gammas=np.array([np.inf])), dict(points=np.array([0.1, np.nan])),
               dict(points=np.array([-np.inf, 0.1]))):
        assert call(**kw) == _lib.ERR_INVALID_ARGUMENT, kw
    assert np.all(pdf == -7.0) and np.all(err == -7.0) and np.all(stats == -7.0)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
class Two:
    world, rank = 2, 0


@pytest.fixture
def no_engine(monkeypatch):
    from stochvolmodels_amd.pricers import logsv_pricer
    from stochvolmodels_amd.utils import mc_payoffs
    asked = []

    def refuse(n, *a, **k):
        asked.append(n)
        raise AssertionError("an engine was asked for")
    for mod in (logsv_pricer, mc_payoffs):
        monkeypatch.setattr(mod, "get_engine", refuse)
    return asked


def test_the_routes_refuse_before_any_engine_is_asked_for(no_engine):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import VariableType
    x = np.linspace(-1.0, 1.0, 5)
    routes = [(sv.LogSVPricer(), sv.LOGSV_BTC_PARAMS), (sv.HestonPricer(), sv.HestonParams()), (sv.HawkesJDPricer(), sv.HawkesJDParams())]
    for pricer, params in routes:
        fn = pricer.get_log_return_mc_pdf_mixture
        for vt in (VariableType.Q_VAR, VariableType.SIGMA):
            with pytest.raises(NotImplementedError):
                fn(params, 0.25, x, nb_path=64, seed=1, variable_type=vt)
        with pytest.raises(NotImplementedError):
            fn(params, 0.25, x, nb_path=64, seed=1, comm=Two())
        with pytest.raises(NotImplementedError):
            fn(params, 0.25, x, nb_path=64, seed=1, devices=[0, 0])
        for bad in ([], [0.0] * 17, [np.nan]):
            with pytest.raises(ValueError):
                fn(params, 0.25, x, risk_premia_gammas=bad, nb_path=64, seed=1)
        with pytest.raises(ValueError):
            fn(params, 0.25, np.array([0.0, np.inf]), nb_path=64, seed=1)
    with pytest.raises(NotImplementedError, match="qe"):
        sv.HestonPricer().get_log_return_mc_pdf_mixture(sv.HestonParams(), 0.25, x, nb_path=64, seed=1, scheme="qe")
    with pytest.raises(NotImplementedError, match="is_spot_measure"):
        sv.LogSVPricer().get_log_return_mc_pdf_mixture(sv.LOGSV_BTC_PARAMS, 0.25, x, nb_path=64, seed=1, is_spot_measure=False)
    fn = sv.compute_mc_vars_pdf_conditional
    mu = np.zeros(64)
    for bad in ([], [0.0] * 17, [np.inf]):
        with pytest.raises(ValueError):
            fn(mu, 0.04, x, gammas=bad)
    with pytest.raises(ValueError):
        fn(mu, np.full(63, 0.04), x)
    with pytest.raises(ValueError):
        fn(np.zeros(0), 0.04, x)
    with pytest.raises(ValueError):
        fn(mu, 0.04, np.array([np.nan]))
    assert no_engine == []
    with pytest.raises(AssertionError, match="an engine was asked for"):        # ... and a good request does ask for one
        fn(mu, 0.04, x)
    assert no_engine == [64]


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_two_names_and_the_binding_has_them():
    from stochvolmodels_amd import _lib, engine
    text = open(os.path.join(ROOT, "include", "svmc_est.h")).read()
    declared = set(re.findall(r"SVMC_EST_API\s+int\s+(svmc_[a-z0-9_]+)\s*\(", text))
    names = {"svmc_cond_density_workspace_bytes", "svmc_cond_density_chain"}
    assert names <= declared
    assert re.search(r"#define SVMC_CD_STATS_DOUBLES 5\b", text) and engine.CD_STATS_DOUBLES == 5 == len(engine.CD_STATS_FIELDS)
    assert tuple(cd.STATS) == engine.CD_STATS_FIELDS
    E = _lib.load_est()
    assert names <= set(E._svmc_est_symbols) and set(E._svmc_est_symbols) == declared
    assert E.svmc_cond_density_chain.restype is C.c_int and len(E.svmc_cond_density_chain.argtypes) == 14
    assert len(E.svmc_cond_density_workspace_bytes.argtypes) == 5
    assert callable(engine.HipEngine.conditional_densities)
    import stochvolmodels_amd as sv
    assert callable(sv.compute_mc_vars_pdf_conditional)
    for cls in (sv.LogSVPricer, sv.HestonPricer, sv.HawkesJDPricer):
        assert callable(cls.get_log_return_mc_pdf_mixture)
    # the kernels: no existing kernel's name is a prefix of a new one's, and the source shares row f11's rule, not a copy of it
    src = open(os.path.join(ROOT, "stochvolmodels_amd", "csrc", "svmc_est.hip")).read()
    assert "cond_density_kernel" in src and "cond_density_finish_kernel" in src
    assert "tc_keep_cmc(" in src and "bool tc_keep_cmc" not in src
