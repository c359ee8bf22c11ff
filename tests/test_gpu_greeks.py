"""
Monte Carlo chain Greeks on the GPU (csrc/svmc_greeks.hip's greeks_payoff_kernel / greeks_finish_kernel,
svmc_logsv_chain_price_greeks, svmc_heston_chain_price_greeks):

  (a) the arithmetic of svmc_greeks_payoff_chain on uploaded host arrays against the long-double twin tests/greeks_twin.py, which
      reads the jobs' spot sums off the device and decides the keep rule and the indicators in double as the device does;
  (b) a quote's numbers do not change, to the bit, with the strikes, expiries or bump pairs that share the launch;
  (c) the fused drivers: price / stderr bit-equal to the single plain call at the same seed, sens against the central difference of
      *_mc_chain_pricer_many's prices at that seed, the C ABI against the Python route;
  (d) |price - (F delta + K dual_delta)| on the fused output;
  (e) a constant-volatility LogSV model (volvol = beta = kappa1 = kappa2 = 0: the log-Euler step is exact in law) against
      Black-76's value, delta, dual delta and vega, within 4 reported standard errors on all 40 figures at seed 1;
  (f) the paired error is true: over 64 seeds the spread of sens["sigma0"] over the mean reported error lies in [0.7, 1.4], and the
      error is below a tenth of what two independent prices would give;
  (g) later single calls on the engine return what they returned before the Greeks call, to the bit.

Deviations: |device - twin| / max(|twin|, 1e-4 scale), test_gpu_tilted.py's measure.  Scale: 1 for delta, dual delta and their
errors (fractions of the discount factor); F / (2 h) for a sensitivity and its error -- the size of the terms pay / (2 h) that sens
is a difference of: the rounding of one payoff, about 1e-16 F, is divided by 2 h with everything else; F for the identity of (d).
Every comparison prints its deviation and the module ends by printing the largest of each quantity (run with -s).  The bounds in TOL
are measured: ten times the largest deviation seen on the MI355X, rounded up to one digit, as
profiles/greeks_observed_tolerances.txt records them, none above the project's parity bound 1e-12.  Two leave no tenfold headroom
under it and assert 1e-12 itself: sens (3.7e-13) and sens against the many-job prices (9.0e-13).  Both are the conditioning of a
difference of payoffs divided by 2 h = 2e-3 |parameter|: one rounding of a job's recentring, 1e-16 F on every path of that job,
is 1e-13 F / |parameter| in the sensitivity; the sums' order is two orders below.  The kernels are deterministic, so the figures
repeat to the bit.
"""
import ctypes as C

import numpy as np
import pytest

import greeks_twin as gt

pytestmark = pytest.mark.gpu

L_ = np.longdouble
KT = 8                                     # SVMC_GREEKS_KT
BLOCK = 256
FIELDS = ("delta", "delta_stderr", "dual_delta", "dual_delta_stderr", "sens", "sens_stderr", "sens_vs_many", "identity")
# ten times the largest deviation observed on the MI355X, rounded up to one digit (profiles/greeks_observed_tolerances.txt)
TOL = dict(delta=3e-15, delta_stderr=3e-15, dual_delta=2e-15, dual_delta_stderr=6e-14, sens=1e-12, sens_stderr=5e-13,
           sens_vs_many=1e-12, identity=3e-14)
assert max(TOL.values()) <= 1e-12          # the project's parity bound: no bound here may exceed it
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def largest_deviations():
    """after the module's tests: the largest deviation of every quantity (shown with -s; the lines of
    profiles/greeks_observed_tolerances.txt)"""
    yield
    for k in FIELDS:
        print(f"\nlargest {k} deviation: {SEEN.get(k, float('nan')):.3e}  bound {TOL[k]:.0e}", end="")
    print()


def deviation(got, want, scale):
    """test_gpu_tilted.py's measure; where the twin is NaN or infinite the device must be the same"""
    want = np.asarray(want, dtype=L_).ravel()
    got = np.asarray(got, dtype=L_).ravel()
    odd = ~np.isfinite(want)
    if np.any(odd):
        assert np.array_equal(np.asarray(got[odd], dtype=np.float64), np.asarray(want[odd], dtype=np.float64), equal_nan=True), (got, want)
        got, want = got[~odd], want[~odd]
    if want.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), L_(1e-4) * L_(scale))))


def note(field, dev, what):
    SEEN[field] = max(SEEN.get(field, 0.0), dev)
    print(f"{what}: {field} deviation {dev:.3e} (bound {TOL[field]:.0e})")
    assert dev <= TOL[field], (what, field, dev)


def codes_of(types):
    return np.where(np.asarray(types) == "C", 0, 1).astype(np.int8)


def slice_of(n_strikes, forward):
    """n_strikes strikes around the forward, puts at or below it, calls above"""
    k = forward * (np.linspace(0.7, 1.4, n_strikes) if n_strikes > 1 else np.array([1.05]))
    return k, np.where(k <= forward, "P", "C")


def rows_of(n, seed, ttm, vol, hs, rel=(1.0, 0.3, -0.5, 2.0, 0.1, -1.5)):
    """a base row and P up / dn rows on the same normals: a constant-volatility model whose volatility moves by rel[p] h_p"""
    z = np.random.default_rng(seed).standard_normal(n)
    return (gt.gaussian_rows(z, ttm, vol), [gt.gaussian_rows(z, ttm, vol + r * h) for r, h in zip(rel, hs)],
            [gt.gaussian_rows(z, ttm, vol - r * h) for r, h in zip(rel, hs)])


def run_on_uploaded(xs, ups, dns, forwards, dfs, strikes, types, hs):
    """the tail on host arrays: xs [m], ups / dns [P][m]"""
    from stochvolmodels_amd.engine import get_engine
    return get_engine(xs[0].size).greeks_payoffs(forwards, dfs, strikes, [codes_of(t) for t in types], hs,
                                                 host_rows=(xs, ups, dns))


def check_against_twin(out, xs, ups, dns, forwards, dfs, strikes, types, hs, what):
    P = len(hs)
    for i, x in enumerate(xs):
        sums = out["spot_sums"][:, i, :]
        tw = gt.greeks(x, forwards[i], dfs[i], strikes[i], types[i], [u[i] for u in ups], [d[i] for d in dns], hs, sums=sums)
        tag = f"{what} expiry={i} n={x.size} K={len(strikes[i])} P={P}"
        assert np.array_equal(out["n_itm"][i], tw["n_itm"]), (tag, out["n_itm"][i], tw["n_itm"])
        for f in ("delta", "delta_stderr", "dual_delta", "dual_delta_stderr"):
            note(f, deviation(out[f][i], tw[f], 1.0), tag)
        for p in range(P):
            assert np.array_equal(out["n_pairs"][p][i], tw["n_pairs"][p]), (tag, p, out["n_pairs"][p][i], tw["n_pairs"][p])
            scale = forwards[i] / (2.0 * hs[p])
            note("sens", deviation(out["sens"][p][i], tw["sens"][p], scale), f"{tag} p={p}")
            note("sens_stderr", deviation(out["sens_stderr"][p][i], tw["sens_stderr"][p], scale), f"{tag} p={p}")


def three_expiries(n, P, seed=0):
    """strike counts 1, KT and KT + 1: one group, a full group, a full group and a ragged one"""
    forwards, dfs, ttms = [1.0, 1.3, 0.9], [1.0, 0.97, 0.9], [0.1, 0.25, 0.5]
    hs = [4e-4 * (1 + p) for p in range(P)]
    rows = [rows_of(n, 50 + seed + i, ttms[i], 0.4 + 0.05 * i, hs) for i in range(3)]
    xs = [r[0] for r in rows]
    ups = [[rows[i][1][p] for i in range(3)] for p in range(P)]
    dns = [[rows[i][2][p] for i in range(3)] for p in range(P)]
    ks, ts = zip(*[slice_of(c, f) for c, f in zip((1, KT, KT + 1), forwards)])
    return xs, ups, dns, forwards, dfs, list(ks), list(ts), hs


# ---- (a) --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK + 1, 3 * BLOCK + 17])
def test_arithmetic_over_path_counts(n):
    case = three_expiries(n, 1, seed=n)
    check_against_twin(run_on_uploaded(*case), *case, "paths")


@pytest.mark.parametrize("P", [0, 1, 6])
def test_arithmetic_over_pair_counts_one_and_three_expiries(P):
    case = three_expiries(3 * BLOCK + 17, P)
    check_against_twin(run_on_uploaded(*case), *case, "pairs, three expiries")
    one = tuple(c if j == 7 else ([row[2:3] for row in c] if j in (1, 2) else c[2:3]) for j, c in enumerate(case))
    check_against_twin(run_on_uploaded(*one), *one, "pairs, one expiry")


def test_arithmetic_through_the_batched_trips():
    """1024 x 256 x 5 + 3 paths: every block makes five full trips (the double-buffered loop, its drain and a single trip) and
    three lanes a ragged sixth"""
    n = 1024 * BLOCK * 5 + 3
    hs = [4e-4]
    x, up, dn = rows_of(n, 9, 0.25, 0.4, hs)
    k, t = np.array([0.9, 1.0, 1.2]), np.array(["P", "C", "C"])
    case = ([x], [[up[0]]], [[dn[0]]], [1.0], [0.99], [k], [t], hs)
    check_against_twin(run_on_uploaded(*case), *case, "batched trips")


def test_nan_inf_and_a_tie():
    n, hs = 300, [4e-4, 8e-4]
    k, t = slice_of(5, 1.1)
    # a NaN in the base row only: out of the money there, every pair kept
    x, up, dn = rows_of(n, 3, 0.25, 0.4, hs)
    x[7] = np.nan
    case = ([x], [[u] for u in up], [[d] for d in dn], [1.1], [0.98], [k], [t], hs)
    out = run_on_uploaded(*case)
    check_against_twin(out, *case, "NaN in the base row")
    assert np.all(out["n_pairs"][0][0] == n) and np.all(out["n_pairs"][1][0] == n)
    # a NaN in one up row only: that pair of that parameter is dropped, the base job and the other parameter keep every path
    x, up, dn = rows_of(n, 4, 0.25, 0.4, hs)
    up[1][11] = np.nan
    case = ([x], [[u] for u in up], [[d] for d in dn], [1.1], [0.98], [k], [t], hs)
    out = run_on_uploaded(*case)
    check_against_twin(out, *case, "NaN in an up row")
    assert np.all(out["n_pairs"][0][0] == n) and np.all(out["n_pairs"][1][0] == n - 1)
    # +inf in the base row: its mean of exp(x) is infinite; +inf in a dn row: that job's is
    for where in ("base", "dn"):
        x, up, dn = rows_of(n, 5, 0.25, 0.4, hs)
        (x if where == "base" else dn[0])[13] = np.inf
        case = ([x], [[u] for u in up], [[d] for d in dn], [1.1], [0.98], [k], [t], hs)
        check_against_twin(run_on_uploaded(*case), *case, f"+inf in the {where} row")
    # a strike equal to a path's spot to the bit: x = 0 has exp(x) = 1 on the host and on the device
    x, up, dn = rows_of(n, 6, 0.25, 0.4, hs)
    x[5] = 0.0
    plain = ([x], [[u] for u in up], [[d] for d in dn], [1.1], [0.98], [k], [t], hs)
    sums = run_on_uploaded(*plain)["spot_sums"][0, 0]
    tie = 1.1 * ((1.0 - (sums[0] / sums[1]) / 1.1) + 1.0)
    case = plain[:5] + ([np.array([tie, tie, np.nextafter(tie, 0.0), np.nextafter(tie, 9.0)])], [np.array(["C", "P", "C", "P"])], hs)
    out = run_on_uploaded(*case)
    check_against_twin(out, *case, "a tie")
    above = int(np.sum(1.1 * ((np.exp(np.delete(x, 5)) - (sums[0] / sums[1]) / 1.1) + 1.0) > tie))
    assert out["n_itm"][0].tolist() == [above, n - 1 - above, above + 1, n - above]       # the tie is in neither of the first two


def test_host_array_route():
    import stochvolmodels_amd as sv
    hs = [4e-4]
    x, up, dn = rows_of(1000, 8, 0.25, 0.4, hs)
    k, t = slice_of(6, 1.1)
    got = sv.compute_mc_vars_greeks(x, 1.1, k.reshape(2, 3), t.reshape(2, 3), 0.98, up, dn, hs)
    assert got["delta"].shape == got["sens"][0].shape == (2, 3) and got["n_pairs"][0].dtype == np.int64
    tw = gt.greeks(x, 1.1, 0.98, k, t, up, dn, hs)             # its own spot sums: a few ulp from the device's
    np.testing.assert_allclose(got["delta"].ravel(), np.asarray(tw["delta"], dtype=np.float64), rtol=1e-11)
    np.testing.assert_allclose(got["sens"][0].ravel(), np.asarray(tw["sens"][0], dtype=np.float64), rtol=1e-9)
    assert np.array_equal(got["n_itm"].ravel(), tw["n_itm"])


# ---- (b) --------------------------------------------------------------------------------------------------------------------------
def test_company_does_not_change_bits():
    xs, ups, dns, fw, dfs, ks, ts, hs = three_expiries(3 * BLOCK + 17, 6)
    full = run_on_uploaded(xs, ups, dns, fw, dfs, ks, ts, hs)
    base = ("delta", "delta_stderr", "dual_delta", "dual_delta_stderr", "n_itm")
    pair = ("sens", "sens_stderr", "n_pairs")
    for i in range(3):                                                            # the expiry alone
        one = run_on_uploaded(xs[i:i + 1], [u[i:i + 1] for u in ups], [d[i:i + 1] for d in dns], fw[i:i + 1], dfs[i:i + 1],
                              ks[i:i + 1], ts[i:i + 1], hs)
        for f in base:
            assert np.array_equal(one[f][0], full[f][i], equal_nan=True), (f, i)
        for f in pair:
            for p in range(6):
                assert np.array_equal(one[f][p][0], full[f][p][i], equal_nan=True), (f, i, p)
    for p in (0, 3, 5):                                                           # the bump pair alone
        one = run_on_uploaded(xs, ups[p:p + 1], dns[p:p + 1], fw, dfs, ks, ts, hs[p:p + 1])
        for i in range(3):
            for f in base:
                assert np.array_equal(one[f][i], full[f][i], equal_nan=True), (f, i)
            for f in pair:
                assert np.array_equal(one[f][0][i], full[f][p][i], equal_nan=True), (f, i, p)
    none = run_on_uploaded(xs, [], [], fw, dfs, ks, ts, [])                       # no pair at all
    for i in range(3):
        for f in base:
            assert np.array_equal(none[f][i], full[f][i], equal_nan=True), (f, i)
    for j in (0, 4, KT):                                                          # the strike alone (of the third expiry)
        one = run_on_uploaded(xs[2:], [u[2:] for u in ups], [d[2:] for d in dns], fw[2:], dfs[2:], [ks[2][j:j + 1]], [ts[2][j:j + 1]], hs)
        for f in base:
            assert np.array_equal(one[f][0], full[f][2][j:j + 1], equal_nan=True), (f, j)
        for f in pair:
            for p in range(6):
                assert np.array_equal(one[f][p][0], full[f][p][2][j:j + 1], equal_nan=True), (f, j, p)


# ---- (c), (d) ---------------------------------------------------------------------------------------------------------------------
CHAIN = dict(ttms=np.array([0.25, 0.5]), forwards=np.array([1.0, 1.02]), discfactors=np.array([0.99, 0.98]),
             strikes_ttms=[np.array([0.8, 0.9, 1.0, 1.1, 1.2]), 1.02 * np.array([0.75, 0.9, 1.0, 1.15, 1.3])],
             optiontypes_ttms=[np.array(["P", "P", "P", "C", "C"]), np.array(["P", "P", "C", "C", "C"])])


def fused_cases():
    import stochvolmodels_amd as sv
    lp = sv.LogSvParams(sigma0=0.4, theta=0.5, kappa1=2.0, kappa2=2.5, beta=-0.8, volvol=1.2)
    hp = sv.HestonParams(v0=0.09, theta=0.12, kappa=3.0, rho=-0.6, volvol=0.5)
    lkw = lambda p: dict(v0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2, beta=p.beta, volvol=p.volvol,     # noqa: E731
                         vol_backbone_etas=np.ones(2))
    hkw = lambda p: dict(v0=p.v0, theta=p.theta, kappa=p.kappa, rho=p.rho, volvol=p.volvol)                              # noqa: E731
    return {"logsv": (lp, sv.logsv_mc_chain_greeks, sv.logsv_mc_chain_pricer, sv.logsv_mc_chain_pricer_many, lkw, {}),
            "heston-euler": (hp, sv.heston_mc_chain_greeks, sv.heston_mc_chain_pricer, sv.heston_mc_chain_pricer_many, hkw,
                             dict(scheme="euler")),
            "heston-qe": (hp, sv.heston_mc_chain_greeks, sv.heston_mc_chain_pricer, sv.heston_mc_chain_pricer_many, hkw,
                          dict(scheme="qe"))}


@pytest.mark.parametrize("model", ["logsv", "heston-euler", "heston-qe"])
def test_fused_driver(model):
    import dataclasses
    from stochvolmodels_amd.mc_greeks import greeks_bumps
    params, greeks, single, many, kw_of, extra = fused_cases()[model]
    n, seed = 4096, 77
    out = greeks(params, nb_path=n, seed=seed, **CHAIN, **extra)
    pr, se = single(nb_path=n, seed=seed, **CHAIN, **kw_of(params), **extra)
    names = list(out["sens"])
    _, hs = greeks_bumps(model.split("-")[0], dataclasses.asdict(params))
    bumped = [dataclasses.replace(params, **{nm: getattr(params, nm) + sgn * h}) for nm, h in zip(names, hs) for sgn in (1.0, -1.0)]
    jobs = many(bumped, nb_path=n, seeds=[seed] * len(bumped), **CHAIN, **extra)
    for i in range(2):
        assert np.array_equal(out["price"][i], pr[i]) and np.array_equal(out["stderr"][i], se[i]), (model, i)
        f, k = CHAIN["forwards"][i], CHAIN["strikes_ttms"][i]
        note("identity", deviation(out["price"][i], f * out["delta"][i].astype(L_) + k * out["dual_delta"][i].astype(L_), f),
             f"{model} expiry={i}")
        for j, (nm, h) in enumerate(zip(names, hs)):
            assert np.all(out["n_pairs"][nm][i] == n)
            want = (jobs[2 * j][0][i].astype(L_) - jobs[2 * j + 1][0][i].astype(L_)) / (2 * L_(h))
            note("sens_vs_many", deviation(out["sens"][nm][i], want, f / (2.0 * h)), f"{model} expiry={i} {nm}")
            assert np.all(out["sens_stderr"][nm][i] > 0.0)


def test_c_abi_equals_the_python_route():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import _lib
    from stochvolmodels_amd.engine import marshalled_chain
    from stochvolmodels_amd.mc_greeks import LOGSV_GREEK_PARAMS, greeks_bumps, greeks_job_table
    params = fused_cases()["logsv"][0]
    n, seed, wrt = 4096, 78, ("sigma0", "volvol")
    out = sv.logsv_mc_chain_greeks(params, nb_path=n, seed=seed, wrt=wrt, **CHAIN)
    names, hs = greeks_bumps("logsv", {k: getattr(params, k) for k in LOGSV_GREEK_PARAMS}, wrt)
    rows = np.ascontiguousarray(greeks_job_table("logsv", [getattr(params, k) for k in LOGSV_GREEK_PARAMS] + [1.0, 1.0], names, hs))
    ch = marshalled_chain(CHAIN["ttms"], CHAIN["forwards"], CHAIN["discfactors"], CHAIN["strikes_ttms"],
                          [codes_of(t) for t in CHAIN["optiontypes_ttms"]])
    L, dp, K = _lib.load(), C.POINTER(C.c_double), 10
    prices, stderrs, base, sens = np.empty(K), np.empty(K), np.empty((5, K)), np.empty((2, 3, K))
    sess = C.c_void_p()
    _lib.check(L.svmc_session_create(C.byref(sess), n, 2, K))
    try:
        call = lambda P, r, h, codes=ch["codes"]: L.svmc_logsv_chain_price_greeks(                                    # noqa: E731
            sess, ch["ttms"], ch["forwards"], ch["discfactors"], 2, ch["strikes"], codes, ch["offsets"], P, r.ctypes.data_as(dp),
            h.ctypes.data_as(dp), 1, 360, seed, 0, prices.ctypes.data_as(dp), stderrs.ctypes.data_as(dp), base.ctypes.data_as(dp),
            sens.ctypes.data_as(dp))
        # everything is checked before anything is launched
        assert call(32, rows, hs) == _lib.ERR_INVALID_ARGUMENT
        assert call(-1, rows, hs) == _lib.ERR_INVALID_ARGUMENT
        assert call(2, rows, np.array([hs[0], 0.0])) == _lib.ERR_INVALID_ARGUMENT
        assert call(2, rows, np.array([np.nan, hs[1]])) == _lib.ERR_INVALID_ARGUMENT
        inv = np.array([0, 1, 2, 0, 1, 0, 1, 0, 1, 0], dtype=np.int8)
        assert call(2, rows, hs, inv.ctypes.data_as(C.POINTER(C.c_int8))) == _lib.ERR_UNKNOWN_PAYOFF
        _lib.check(call(2, rows, hs))
    finally:
        L.svmc_session_destroy(sess)
    flat = lambda parts: np.concatenate([np.ravel(p) for p in parts])                                                     # noqa: E731
    assert np.array_equal(prices, flat(out["price"])) and np.array_equal(stderrs, flat(out["stderr"]))
    for r, f in enumerate(("delta", "delta_stderr", "dual_delta", "dual_delta_stderr", "n_itm")):
        assert np.array_equal(base[r], flat(out[f])), f
    for j, nm in enumerate(names):
        for r, f in enumerate(("sens", "sens_stderr", "n_pairs")):
            assert np.array_equal(sens[j, r], flat(out[f][nm])), (nm, f)


# ---- (e), (f) ---------------------------------------------------------------------------------------------------------------------
SIGMA = 0.4


def flat_model():
    import stochvolmodels_amd as sv
    return sv.LogSvParams(sigma0=SIGMA, theta=SIGMA, kappa1=0.0, kappa2=0.0, beta=0.0, volvol=0.0)


def test_constant_volatility_against_black76_at_seed_1():
    """fixed before looking: seed=1.  40 figures within 4 of their reported standard errors; at a sound seed the chance of a miss
    is 40 x 6.3e-5 = 0.25 %."""
    import stochvolmodels_amd as sv
    out = sv.logsv_mc_chain_greeks(flat_model(), wrt=("sigma0",), nb_path=1 << 16, seed=1, **CHAIN)
    zs = []
    for i in range(2):
        price, delta, dual, vega = gt.black76(CHAIN["forwards"][i], CHAIN["strikes_ttms"][i], CHAIN["ttms"][i], SIGMA,
                                              CHAIN["discfactors"][i], CHAIN["optiontypes_ttms"][i])
        for name, got, err, want in (("price", out["price"][i], out["stderr"][i], price),
                                     ("delta", out["delta"][i], out["delta_stderr"][i], delta),
                                     ("dual_delta", out["dual_delta"][i], out["dual_delta_stderr"][i], dual),
                                     ("sens sigma0", out["sens"]["sigma0"][i], out["sens_stderr"]["sigma0"][i], vega)):
            z = (got - want) / err
            print(f"expiry={i} {name}: z = {np.round(z, 2)}")
            zs.append(z)
    zs = np.concatenate(zs)
    assert zs.size == 40 and np.all(np.abs(zs) <= 4.0), zs


def test_the_paired_error_is_true_and_is_the_point():
    import dataclasses
    import stochvolmodels_amd as sv
    p, h, n = flat_model(), 1e-3 * SIGMA, 4096
    runs = [sv.logsv_mc_chain_greeks(p, wrt=("sigma0",), nb_path=n, seed=seed, **CHAIN) for seed in range(1, 65)]
    for i in range(2):
        sens = np.array([r["sens"]["sigma0"][i] for r in runs])
        err = np.array([r["sens_stderr"]["sigma0"][i] for r in runs])
        ratio = sens.std(axis=0, ddof=1) / err.mean(axis=0)
        print(f"expiry={i}: spread of 64 sens over the mean reported error = {np.round(ratio, 3)}")
        assert np.all((ratio >= 0.7) & (ratio <= 1.4)), (i, ratio)
    up, dn = sv.logsv_mc_chain_pricer_many([dataclasses.replace(p, sigma0=SIGMA + h), dataclasses.replace(p, sigma0=SIGMA - h)],
                                           nb_path=n, seeds=[1, 1], **CHAIN)
    for i in range(2):
        unpaired = np.sqrt(up[1][i] ** 2 + dn[1][i] ** 2) / (2 * h)
        print(f"expiry={i}: paired over unpaired error = {np.round(runs[0]['sens_stderr']['sigma0'][i] / unpaired, 5)}")
        assert np.all(runs[0]["sens_stderr"]["sigma0"][i] < 0.1 * unpaired), i


# ---- (g) --------------------------------------------------------------------------------------------------------------------------
def test_later_single_calls_are_undisturbed():
    import stochvolmodels_amd as sv
    params, _, _, _, kw_of, _ = fused_cases()["logsv"]
    n, seed = 4000, 31                         # a path count no other test of the module uses: its engine is fresh
    others = [params, sv.LogSvParams(sigma0=0.5, theta=0.4, kappa1=1.0, kappa2=1.0, beta=-0.5, volvol=0.8)]

    def calls():
        a = sv.logsv_mc_chain_pricer(nb_path=n, seed=seed, **CHAIN, **kw_of(params))
        b = sv.logsv_mc_chain_pricer_many(others, nb_path=n, seeds=[seed, seed + 1], **CHAIN)
        c = sv.logsv_mc_chain_pricer_conditional(nb_path=n, seed=seed, **CHAIN, **kw_of(params))
        return [np.concatenate(part) for part in (a[0], a[1], b[0][0], b[0][1], b[1][0], b[1][1], c[0], c[1])]

    before = calls()
    sv.logsv_mc_chain_greeks(params, nb_path=n, seed=seed + 5, **CHAIN)
    sv.heston_mc_chain_greeks(fused_cases()["heston-qe"][0], nb_path=n, seed=seed, scheme="qe", **CHAIN)
    for x, y in zip(before, calls()):
        assert np.array_equal(x, y)
