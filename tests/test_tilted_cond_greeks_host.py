"""
Host checks of the conditional Monte Carlo Greeks under the exponential risk-premia kernel (include/svmc_est.h).
No GPU.

  1. The per-path terms W delta_j, W dual_delta_j, W dual_gamma_j of tests/tilted_cond_greeks_twin.py against mpmath: the first two
     are quadratures of exp(gamma x) times the payoff's derivative in F and in K under the normal density, over the side of the kink
     where the option is in the money; the third is the density term exp(gamma x*) N(x*; mu, cv) / K' at the kink x* = ln(K' / F).
     First derivatives to ESSCHER_BOUND relative (floored at 1e-4), the dual gamma to DUAL_GAMMA_BOUND.
  2. The twin's closed forms against central differences of tilted_cond_twin.estimator's prices in F and in K (2 000 paths, h = 1e-5),
     price = F delta + K dual_delta, and the reported errors against the leave-one-out jackknife of the values.
  3. Four deliberate errors of the twin (mutate=), each of which must break a named check of 1 or 2.
  4. The errors are calibrated: over 64 seeds of hawkes_cmc_twin.np_chain at 4 096 paths the deviation of an estimate over the seeds
     against the root mean square of its reported error, the median over the 42 quotes, per gamma and quantity in 0.73 .. 1.27.
  5. The third library: it builds, exports what svmc_est.h declares, the binding covers the header, no undefined svmc_ symbol, gfx950
     inside, every kernel without scratch, LDS for the block sums' exchange only, stale when its source is newer, and its
     host-only entry with its refusals.  No export or kernel is held to a literal list or a count: the header is the reference.  The LDS
     bound is asserted for the four kernels the unit has today, by name; a kernel added later is held to zero scratch and to whole
     exchange buffers (a multiple of 32 bytes) until it is given its own line.

Checks 1 to 4 exercise tests/tilted_cond_greeks_twin.py alone: they validate the SPECIFICATION -- the formulas of the header, which the
GPU tests then hold the device to -- and pass without the library.  What holds the shipped code is check 5 here,
tests/test_tilted_cond_greeks_routes_host.py and tests/test_gpu_tilted_cond_greeks.py; those fail without the feature.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import hawkes_cmc_twin as hc  # noqa: E402
import tilted_cond_greeks_twin as tg  # noqa: E402
import tilted_cond_twin as tc  # noqa: E402

LD = np.longdouble
GAMMAS = (-3.0, -1.0, 0.0, 0.5, 3.0)
ESSCHER_BOUND = 1e-13                  # the project's bound of a single path's term against quadrature (tests/test_tilted_cond_host.py)
# ten times the largest deviation of W dual_gamma_j from mpmath over mpmath_cases(), rounded up to one digit
# (profiles/tilted_cond_greeks_observed_tolerances.txt: 1.1e-16 observed, the rounding of the double exponential behind the twin's density)
DUAL_GAMMA_BOUND = 2e-15
CAL_BAND = (0.73, 1.27)                # the project's band for a 64-sample deviation, applied to the median over the quotes (row f14)
CAL_GAMMAS = (-3.0, -1.0, 0.0, 1.0, 3.0)
CAL_SEEDS = range(1000, 1064)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
def to_mp(mp, v):
    """a long double as an mpf, exactly: its nearest double plus the remainder"""
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(LD(v) - LD(hi)))


def quad_derivatives(mp, mu, cv, forward, strike, put, gamma, corr):
    """(d/dF, d/dK) of E[exp(gamma x) payoff(F e^x - F c - K)] for x ~ N(mu, cv), c = corr / F held fixed, by quadrature of
    exp(gamma x) times the payoff's derivative over the in-the-money side of the kink, and the density term
    exp(gamma x*) N(x*; mu, cv) / K' at x* = ln(K' / F), all at mpmath's precision"""
    M = mp.mpf
    mu, cv, F, kp, gamma, c = M(mu), M(cv), M(forward), M(strike) + M(corr), M(gamma), M(corr) / M(forward)
    sd = mp.sqrt(cv)
    s = -1 if put else 1

    def dens(x):
        return mp.exp(-(x - mu) ** 2 / (2 * cv)) / (sd * mp.sqrt(2 * mp.pi))

    # the integrands peak at mu + gamma cv (the strike's term) and mu + (gamma + 1) cv (the spot's)
    centre = mu + gamma * cv
    lo, hi = centre - 45 * sd, centre + cv + 45 * sd
    if kp > 0:
        kink = mp.log(kp / F)
        a, b = (lo, min(kink, hi)) if put else (max(kink, lo), hi)
        density = mp.exp(gamma * kink) * dens(kink) / kp
    else:                                                   # K' <= 0: a call is in the money everywhere, a put nowhere
        a, b = (lo, lo) if put else (lo, hi)
        density = M(0)
    if not a < b:
        return M(0), M(0), density
    pts = sorted({a, b} | {p for p in (centre, centre + cv) if a < p < b})
    d_f = mp.quad(lambda x: mp.exp(gamma * x) * s * (mp.exp(x) - c) * dens(x), pts)
    d_k = mp.quad(lambda x: mp.exp(gamma * x) * (-s) * dens(x), pts)
    return d_f, d_k, density


def mpmath_cases():
    forward = 1.3
    for mu in (-0.2, 0.1):
        for cv in (0.01, 0.09):
            for gamma in GAMMAS:
                for rel in (0.8, 1.0, 1.25):
                    for put in (False, True):
                        for corr in (0.0, 0.03 * forward):
                            yield mu, cv, forward, rel * forward, put, gamma, corr
    for gamma in GAMMAS:                                    # K' = K + corr <= 0
        for put in (False, True):
            yield 0.05, 0.04, forward, 0.5 * forward, put, gamma, -0.5 * forward
            yield 0.05, 0.04, forward, 0.5 * forward, put, gamma, -2.0 * forward


_MP_WANT = []


def mpmath_references():
    """quad_derivatives of every case at 40 digits, computed once and left unchanged"""
    import mpmath
    if not _MP_WANT:
        with mpmath.workdps(40):
            _MP_WANT.extend(quad_derivatives(mpmath, *case) for case in mpmath_cases())
    return _MP_WANT


def mpmath_deviations(mutate=None):
    """[cases][3]: the relative deviations (floored at 1e-4) of W delta_j, W dual_delta_j, W dual_gamma_j from mpmath"""
    import mpmath
    out = []
    with mpmath.workdps(40):
        for (mu, cv, forward, k, put, gamma, corr), want in zip(mpmath_cases(), mpmath_references()):
            w, *terms = tg.path_terms([mu], [cv], forward, k, put, gamma, corr, mutate)
            out.append([float(abs(to_mp(mpmath, w[0]) * to_mp(mpmath, t[0]) - v) / max(abs(v), mpmath.mpf(1e-4)))
                        for t, v in zip(terms, want)])
    return np.array(out)


@pytest.fixture(scope="module")
def mp_dev():
    return mpmath_deviations()


def test_the_per_path_terms_against_mpmath(mp_dev):
    worst = mp_dev.max(axis=0)
    print(f"{mp_dev.shape[0]} single-path cases: largest deviation of W delta {worst[0]:.3e}, W dual delta {worst[1]:.3e} "
          f"(bound {ESSCHER_BOUND:.0e}), W dual gamma {worst[2]:.3e} (bound {DUAL_GAMMA_BOUND:.0e})")
    assert mp_dev.shape == (260, 3)
    cases = list(mpmath_cases())
    assert {c[4] for c in cases} == {False, True} and {c[5] for c in cases} == set(GAMMAS) and any(c[6] > 0 for c in cases)
    assert DUAL_GAMMA_BOUND <= 1e-12
    assert worst[0] <= ESSCHER_BOUND and worst[1] <= ESSCHER_BOUND, mp_dev
    assert worst[2] <= DUAL_GAMMA_BOUND, mp_dev[:, 2]


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
FD_F, FD_K, FD_T, FD_H = 1.3, (0.9, 1.2, 1.3, 1.5), ("P", "P", "C", "C"), 1e-5
FD_BOUNDS = dict(delta=1e-9, dual_delta=1e-9, dual_gamma=1e-5)       # the last relative, floored at 1e-3
HOMOGENEITY_BOUND = ESSCHER_BOUND      # price = F delta + K dual_delta is exact in exact arithmetic: what is left is the CDFs' rounding


def fd_rows():
    rng = np.random.default_rng(18)
    mu = 0.2 * rng.standard_normal(2000) - 0.02
    cv = 0.05 * rng.random(2000)
    cv[::7] = 0.0
    return mu, cv


def finite_difference_deviations(mutate=None):
    """{(recenter, gamma): dict(delta, dual_delta, dual_gamma, homogeneity, jackknife, weight_share)} -- the largest deviations over
    the four quotes of the twin's closed forms from central differences of row f17's twin's prices, of price - F delta - K dual_delta,
    and of jackknife error / reported error - 1 over the three quantities"""
    mu, cv = fd_rows()
    k0, h = np.array(FD_K), FD_H
    out = {}
    for recenter in (False, True):
        for gamma in GAMMAS:
            g, st = tg.estimator(mu, cv, FD_F, k0, FD_T, gamma, recenter, mutate)
            price = lambda f, k: tc.estimator(mu, cv, f, k, FD_T, gamma, recenter)[0]     # noqa: E731
            p0 = price(FD_F, k0)
            d_f = (price(FD_F + h, k0) - price(FD_F - h, k0)) / (2 * LD(h))
            pk_up, pk_dn = price(FD_F, k0 + h), price(FD_F, k0 - h)
            d_k = (pk_up - pk_dn) / (2 * LD(h))
            d_kk = (pk_up - 2 * p0 + pk_dn) / (LD(h) * LD(h))
            row = dict(delta=float(np.abs(g["delta"] - d_f).max()), dual_delta=float(np.abs(g["dual_delta"] - d_k).max()),
                       dual_gamma=float((np.abs(g["dual_gamma"] - d_kk) / np.maximum(np.abs(d_kk), LD(1e-3))).max()),
                       homogeneity=float(np.abs(p0 - FD_F * g["delta"] - k0 * g["dual_delta"]).max()))
            # the leave-one-out jackknife of value = sum W v / sum W: an error formed from the values alone
            keep = tc.keep_mask(mu, cv, FD_F, gamma)
            n, jack = int(keep.sum()), 0.0
            for q, (k, t) in enumerate(zip(k0, FD_T)):
                w, *terms = tg.path_terms(mu[keep], cv[keep], FD_F, k, t == "P", gamma, st["corr"])
                for name, v in zip(("delta", "dual_delta", "dual_gamma"), terms):
                    loo = ((w * v).sum() - w * v) / (w.sum() - w)
                    err_j = np.sqrt((n - 1) / LD(n) * ((loo - loo.mean()) ** 2).sum())
                    jack = max(jack, abs(float(err_j / g[name + "_stderr"][q]) - 1.0))
            w = tg.path_terms(mu[keep], cv[keep], FD_F, 1.0, False, gamma)[0]
            row.update(jackknife=jack, weight_share=float(w.max() / w.sum()), n=n)
            out[(recenter, gamma)] = row
    return out


def fd_failures(dev):
    """the named checks of 2 that `dev` misses"""
    bad = set()
    for key, row in dev.items():
        for name, bound in FD_BOUNDS.items():
            if not row[name] <= bound:
                bad.add(name)
        if not row["homogeneity"] <= HOMOGENEITY_BOUND:
            bad.add("homogeneity")
        # jackknife^2 = (n - 1) / n sum_j (W_j (v_j - value) / (sum W - W_j))^2 less the square of the leave-one-out mean's offset: with
        # r = max W_j / sum W it lies within (1 - r)^-2 and (n - 1) / n (1 - r^2 / (1 - r)^2) of the reported error's square
        if not row["jackknife"] <= 2.0 * row["weight_share"] + 1.0 / row["n"]:
            bad.add("jackknife")
    return bad


@pytest.fixture(scope="module")
def fd_dev():
    return finite_difference_deviations()


def test_the_closed_forms_against_central_differences_of_the_price(fd_dev):
    for (recenter, gamma), row in fd_dev.items():
        print(f"recenter={recenter!s:5} gamma={gamma:+.1f}: delta {row['delta']:.2e}, dual delta {row['dual_delta']:.2e}, dual gamma "
              f"{row['dual_gamma']:.2e} (relative), |price - F delta - K dual_delta| {row['homogeneity']:.2e}, jackknife / error - 1 "
              f"{row['jackknife']:.2e} (bound {2.0 * row['weight_share'] + 1.0 / row['n']:.2e})")
    assert len(fd_dev) == 10 and fd_failures(fd_dev) == set()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_each_deliberate_error_breaks_a_named_check(mp_dev):
    assert set(tg.MUTATIONS) == {"no_c_bk", "no_forward_shift", "d1_in_dual_gamma", "unweighted_error"}
    cases = list(mpmath_cases())
    live = np.array([c[3] + c[6] > 0 for c in cases])      # (at K' <= 0 the terms are constants)
    gam = np.array([c[5] for c in cases])
    corr = np.array([c[6] for c in cases])
    # c B_k dropped from delta: check 1 on W delta wherever corr != 0, and check 2's delta with recentring
    dev = mpmath_deviations("no_c_bk")
    assert np.all(dev[live & (corr != 0), 0] > 1e3 * ESSCHER_BOUND) and np.all(dev[corr == 0, 0] <= ESSCHER_BOUND)
    assert np.all(dev[:, 1:] <= np.maximum(mp_dev[:, 1:], ESSCHER_BOUND))
    assert "delta" in fd_failures(finite_difference_deviations("no_c_bk"))
    # the forward's shift gamma cv left out: check 1 on all three terms at gamma != 0
    dev = mpmath_deviations("no_forward_shift")
    assert np.all(dev[live & (gam != 0), :] > 1e3 * ESSCHER_BOUND), dev[live & (gam != 0), :].min()
    assert np.all(dev[gam == 0] <= np.maximum(mp_dev[gam == 0], ESSCHER_BOUND))
    # d1 where d2 belongs: check 1 on W dual gamma alone
    dev = mpmath_deviations("d1_in_dual_gamma")
    assert np.all(dev[live, 2] > 1e3 * DUAL_GAMMA_BOUND) and np.array_equal(dev[:, :2], mp_dev[:, :2])
    # the unweighted error: check 2's jackknife wherever the weights differ
    fd = finite_difference_deviations("unweighted_error")
    assert fd_failures(fd) == {"jackknife"}
    assert fd_failures({k: v for k, v in fd.items() if k[1] == 0.0}) == set()       # at gamma = 0 the two formulas are one


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def calibration_ratios(estimate, n_quotes):
    """estimate(seed) -> {gamma: {quantity: (values [quotes], errors [quotes])}}; returns {gamma: {quantity: ratios [quotes]}}, the
    deviation of the estimate over CAL_SEEDS over the root mean square of its reported error"""
    runs = [estimate(seed) for seed in CAL_SEEDS]
    out = {}
    for gamma in CAL_GAMMAS:
        out[gamma] = {}
        for q in tg.QUANTITIES:
            v = np.array([r[gamma][q][0] for r in runs], dtype=np.float64)
            e = np.array([r[gamma][q][1] for r in runs], dtype=np.float64)
            assert v.shape == (len(CAL_SEEDS), n_quotes)
            out[gamma][q] = v.std(axis=0, ddof=1) / np.sqrt((e * e).mean(axis=0))
    return out


def check_calibration(ratios, write=print):
    for gamma, per_q in ratios.items():
        for q, r in per_q.items():
            write(f"gamma={gamma:+.0f} {q:10s} median {np.median(r):.3f}  quotes {r.min():.3f} .. {r.max():.3f}  "
                  + " ".join(f"{x:.2f}" for x in r))
    for gamma, per_q in ratios.items():
        for q, r in per_q.items():
            assert CAL_BAND[0] <= np.median(r) <= CAL_BAND[1], (gamma, q, np.median(r))


def stat_grid():
    nb, dts, t0 = [], [], 0.0
    for t in hc.STAT_TTMS:
        nb.append(max(int(np.ceil((t - t0) * hc.STAT_SPY)), 1))
        dts.append((t - t0) / nb[-1])
        t0 = t
    return nb, dts


def test_the_reported_errors_are_calibrated_on_the_twin():
    import stochvolmodels_amd as sv
    p = sv.HawkesJDParams().to_dict()                       # the parameters of tests/golden/hawkes_mc.npz: the defaults
    chain, _ = hc.stat_chain(p)
    nb, dts = stat_grid()
    cvs = hc.host_cv(p["sigma"], nb, dts)
    n = 4096

    def estimate(seed):
        states = hc.np_chain(p, seed, n, nb, dts)
        out = {}
        for gamma in CAL_GAMMAS:
            parts = [tg.estimator(mu, np.full(n, cv), 1.0, chain["strikes_ttms"][i], chain["optiontypes_ttms"][i], gamma, False,
                                  with_price=False)[0] for i, ((mu, _, _), cv) in enumerate(zip(states, cvs))]
            out[gamma] = {q: (np.concatenate([g[q] for g in parts]), np.concatenate([g[q + "_stderr"] for g in parts]))
                          for q in tg.QUANTITIES}
        return out

    check_calibration(calibration_ratios(estimate, 42))


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def declared_est():
    text = open(os.path.join(ROOT, "include", "svmc_est.h")).read()
    return sorted(set(re.findall(r"SVMC_EST_API\s+int\s+(svmc_[a-z0-9_]+)\s*\(", text)))


def test_the_third_library_exports_what_its_header_declares():
    from stochvolmodels_amd import _lib, build
    build.build()
    assert os.path.exists(build.EST_LIB) and os.path.basename(build.EST_LIB) == "libsvmc_est.so"
    declared = declared_est()
    assert {"svmc_est_version", "svmc_tilted_cond_greeks_workspace_bytes", "svmc_tilted_cond_greeks_chain"} <= set(declared)
    nm = subprocess.run(["nm", "-D", "--defined-only", build.EST_LIB], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\bT (svmc_[a-z0-9_]+)", nm))) == declared
    undefined = subprocess.run(["nm", "-D", "--undefined-only", build.EST_LIB], capture_output=True, text=True, check=True).stdout
    assert not re.search(r"\bsvmc_", undefined), "libsvmc_est.so links nothing from libsvmc.so or libsvmc_ext.so"
    E = _lib.load_est()
    assert sorted(E._svmc_est_symbols) == declared and E.svmc_est_version() == 100
    header = open(os.path.join(ROOT, "include", "svmc_est.h")).read()
    assert re.search(r"#define SVMC_EST_VERSION 100\b", header)
    # neither of the other libraries has any of it
    L, X = _lib.load(), _lib.load_ext()
    assert not set(L._svmc_symbols) & set(declared) and not set(X._svmc_ext_symbols) & set(declared)
    assert not any(hasattr(L, name) or hasattr(X, name) for name in declared)
    out = subprocess.run(["strings", "-a", build.EST_LIB], capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_every_kernel_of_the_third_library_is_without_scratch():
    from stochvolmodels_amd import build
    build.build()
    meta = json.load(open(build.EST_ISA_JSON))["metadata"]
    assert meta and any("tilted_cond_greeks_kernel" in k for k in meta)
    for name, m in meta.items():                            # EVERY kernel, however many there are
        assert m["scratch_bytes"] == 0, (name, m)
        assert m["lds_bytes"] % (4 * 8) == 0, (name, m)     # whole exchange buffers: one double per wave and value
    # LDS is the block sums' exchange and nothing else: 4 waves x block_sum_padded(values) doubles, the values read off the source
    src = open(build.EST_SRC).read()
    const = lambda pattern: int(re.search(pattern, src).group(1))      # noqa: E731
    cols, nstat, kt = const(r"TCG_COLS = (\d+);"), const(r"TCG_NSTAT = (\d+);"), const(r"#define SVMC_TCG_KT (\d+)")
    values = {"tilted_cond_greeks_forward_kernel": 3, "tilted_cond_greeks_forward_finish_kernel": 1,
              "tilted_cond_greeks_kernel": (cols * kt + nstat + 7) // 8 * 8, "tilted_cond_greeks_finish_kernel": 1}
    for short, nv in values.items():
        hit = [k for k in meta if short + "E" in k or short + "I" in k]    # (the mangled name: the identifier, then its arguments)
        assert len(hit) == 1, (short, sorted(meta))
        assert meta[hit[0]]["lds_bytes"] <= 4 * nv * 8, (short, meta[hit[0]])


def test_the_third_library_is_stale_when_its_source_is_newer(tmp_path, monkeypatch):
    from stochvolmodels_amd import build
    build.build()
    assert not build.est_is_stale()
    lib = tmp_path / "libsvmc_est.so"
    lib.write_bytes(b"")
    old = os.path.getmtime(build.EST_SRC) - 10.0
    os.utime(lib, (old, old))
    monkeypatch.setattr(build, "EST_LIB", str(lib))
    assert build.est_is_stale()                             # older than its source
    monkeypatch.setattr(build, "EST_LIB", str(tmp_path / "absent.so"))
    assert build.est_is_stale()


def test_host_only_entry_and_refusals_without_a_gpu():
    import ctypes as C
    from stochvolmodels_amd import _lib
    E = _lib.load_est()
    nbytes = C.c_size_t(0)
    assert E.svmc_tilted_cond_greeks_workspace_bytes(257, 2, 24, 5, C.byref(nbytes)) == _lib.OK and nbytes.value > 0
    small = nbytes.value
    assert E.svmc_tilted_cond_greeks_workspace_bytes(1 << 20, 2, 24, 5, C.byref(nbytes)) == _lib.OK and nbytes.value > small
    assert E.svmc_tilted_cond_greeks_workspace_bytes(257, 2, 0, 1, C.byref(nbytes)) == _lib.OK and nbytes.value > 0
    for args in ((0, 2, 24, 5), (257, 0, 24, 5), (257, 2, 24, 0), (257, 2, 24, 17)):
        assert E.svmc_tilted_cond_greeks_workspace_bytes(*args, C.byref(nbytes)) == _lib.ERR_INVALID_ARGUMENT
    assert E.svmc_tilted_cond_greeks_workspace_bytes(257, 2, 24, 5, None) == _lib.ERR_INVALID_ARGUMENT
    # the chain entry refuses before it touches the device: null pointers, sizes, offsets, values, types, the workspace's size
    n, m, K, G = 64, 1, 2, 1
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    fwd, k, g = np.array([1.0]), np.array([0.9, 1.1]), np.array([0.5])
    types, offs = np.array([0, 1], dtype=np.int8), np.array([0, 2], dtype=np.uintp)
    greeks, stats = np.full(G * 8 * K, -7.0), np.full(G * m * 4, -7.0)
    rows = (vp * 1)(0x1000)                                 # never dereferenced: every call below is refused first
    ws = vp(0x1000)

    def call(rows_mu=rows, rows_cv=rows, n_path=n, forwards=fwd, n_exp=m, strikes=k, codes=types, offsets=offs, gammas=g, ng=G,
             out=greeks, st=stats, workspace=ws, ws_bytes=8):
        a = lambda v, t: None if v is None else v.ctypes.data_as(t)      # noqa: E731
        return E.svmc_tilted_cond_greeks_chain(rows_mu, rows_cv, n_path, a(forwards, dp), n_exp, a(strikes, dp),
                                               a(codes, C.POINTER(C.c_int8)), a(offsets, C.POINTER(C.c_size_t)), a(gammas, dp), ng, 0,
                                               a(out, dp), a(st, dp), workspace, ws_bytes, None)

    assert call() == _lib.ERR_WORKSPACE
    for kw in (dict(rows_mu=None), dict(rows_cv=None), dict(forwards=None), dict(strikes=None), dict(codes=None), dict(offsets=None),
               dict(gammas=None), dict(out=None), dict(st=None), dict(workspace=None), dict(rows_mu=(vp * 1)(None)), dict(n_path=0),
               dict(n_exp=0), dict(ng=0), dict(ng=17), dict(offsets=np.array([1, 2], dtype=np.uintp)),
               dict(offsets=np.array([0, 2, 1], dtype=np.uintp), n_exp=2, forwards=np.array([1.0, 1.0]), rows_mu=(vp * 2)(0x1000, 0x1000),
                    rows_cv=(vp * 2)(0x1000, 0x1000)),
               dict(gammas=np.array([np.nan])), dict(forwards=np.array([np.inf])), dict(forwards=np.array([0.0])),
               dict(strikes=np.array([0.9, np.nan]))):
        assert call(**kw) == _lib.ERR_INVALID_ARGUMENT, kw
    assert call(codes=np.array([0, 2], dtype=np.int8)) == _lib.ERR_UNKNOWN_PAYOFF
    assert np.all(greeks == -7.0) and np.all(stats == -7.0)
