"""
Host checks of conditional Monte Carlo under the exponential risk-premia kernel (include/svmc_ext.h).  No GPU.

  1. The Esscher identity: for single paths W B of tests/tilted_cond_twin.py against mpmath.quad of exp(gamma x) payoff(F e^x - corr)
     under the normal density, split at the payoff's kink, to 1e-13 relative (floored at 1e-4 F); the twin with the forward's shift
     gamma cv left out must miss it.
  2. The twin against the plain estimator under the kernel on x = mu + sqrt(cv) Z over hawkes_cmc_twin.np_chain paths (2^15 paths,
     the twin's stat_chain, gamma -3, -1, +1, +3): all 168 figures within Z_BOUND combined standard errors, and every conditional error
     below its plain one.
  3. The second library: it builds, exports exactly what svmc_ext.h declares, the binding covers the header, no kernel of it has
     scratch or LDS beyond the block sums' exchange buffers; the core keeps its kernels (tests/golden/libsvmc_kernel_names.json, the
     names of the build before this library existed) and its 143 / 143 entry points.
  4. The routes: the refusals before any engine is asked for, what is handed to the engine, the shapes, one gamma = the list form.
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

import cmc_twin as ct  # noqa: E402
import hawkes_cmc_twin as hc  # noqa: E402
import tilted_cond_twin as tc  # noqa: E402
from fake_engine import FakeEngine  # noqa: E402

LD = np.longdouble
GAMMAS = (-3.0, -1.0, 0.0, 0.5, 3.0)
ESSCHER_BOUND = 1e-13
Z_BOUND = hc.Z_BOUND                   # 4.5 combined standard errors, as the twins of row f16 are held; the experiment alone shows 2.25
EXT_SYMBOLS = ("svmc_ext_version", "svmc_tilted_cond_workspace_bytes", "svmc_tilted_cond_payoff_chain")
# LDS of the block sums' exchange buffers and nothing else: 4 waves x block_sum_padded(values) doubles
LDS_BOUND = {"tilted_cond_forward_kernel": 4 * 3 * 8, "tilted_cond_forward_finish_kernel": 4 * 8,
             "tilted_cond_payoff_kernel": 4 * 32 * 8, "tilted_cond_finish_kernel": 4 * 8}


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
def quad_term(mp, mu, cv, forward, strike, put, gamma, corr):
    """E[exp(gamma x) payoff(F e^x - corr)] for x ~ N(mu, cv) by quadrature at mpmath's precision, split at the kink"""
    F = mp.mpf
    mu, cv, forward, kp, gamma = F(mu), F(cv), F(forward), F(strike) + F(corr), F(gamma)
    sd = mp.sqrt(cv)
    sign = -1 if put else 1

    def f(x):
        pay = sign * (forward * mp.exp(x) - kp)
        return mp.exp(gamma * x) * (pay if pay > 0 else F(0)) * mp.exp(-(x - mu) ** 2 / (2 * cv)) / (sd * mp.sqrt(2 * mp.pi))

    # the two terms of the integrand peak at mu + gamma cv (the strike's) and mu + (gamma + 1) cv (the spot's)
    centre = mu + gamma * cv
    lo, hi = centre - 45 * sd, centre + cv + 45 * sd
    pts = {lo, centre, centre + cv, hi}
    if kp > 0:
        kink = mp.log(kp / forward)
        if lo < kink < hi:
            pts.add(kink)
    return mp.quad(f, sorted(pts))


def to_mp(mp, v):
    """a long double as an mpf, exactly: its nearest double plus the remainder"""
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(LD(v) - LD(hi)))


def esscher_cases():
    forward = 1.3
    for mu in (-0.2, 0.1):
        for cv in (0.01, 0.09):
            for gamma in GAMMAS:
                for rel in (0.8, 1.0, 1.25):
                    for put in (False, True):
                        yield mu, cv, forward, rel * forward, put, gamma, 0.0
    for gamma in GAMMAS:                                    # K' = K + corr <= 0: a call pays F_t - K', a put nothing
        for put in (False, True):
            yield 0.05, 0.04, forward, 0.5 * forward, put, gamma, -0.5 * forward
            yield 0.05, 0.04, forward, 0.5 * forward, put, gamma, -2.0 * forward


def esscher_deviations(shift_forward):
    import mpmath
    out = []
    with mpmath.workdps(40):
        for mu, cv, forward, k, put, gamma, corr in esscher_cases():
            w, _, b = tc.path_terms([mu], [cv], forward, k, put, gamma, corr, shift_forward)
            want = quad_term(mpmath, mu, cv, forward, k, put, gamma, corr)
            got = to_mp(mpmath, w[0]) * to_mp(mpmath, b[0])
            out.append(float(abs(got - want) / max(abs(want), mpmath.mpf(1e-4) * forward)))
    return np.array(out)


def test_the_esscher_identity_against_quadrature():
    dev = esscher_deviations(True)
    print(f"Esscher identity: {dev.size} single-path terms, largest deviation {dev.max():.3e} (bound {ESSCHER_BOUND:.0e})")
    assert dev.size == 140 and dev.max() <= ESSCHER_BOUND, dev
    wrong = esscher_deviations(False)                       # the forward without its shift gamma cv
    gam = np.array([c[5] for c in esscher_cases()])
    print(f"... without the forward's shift: smallest deviation at gamma != 0 {wrong[gam != 0.0].min():.3e}")
    assert np.all(wrong[gam == 0.0] <= ESSCHER_BOUND)       # at gamma = 0 there is nothing to leave out
    live = (gam != 0.0) & np.array([not (c[4] and c[3] + c[6] <= 0.0) for c in esscher_cases()])     # (a put at K' <= 0 is 0 either way)
    assert np.all(wrong[live] > 1e3 * ESSCHER_BOUND), wrong[live].min()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def test_the_twin_against_the_plain_estimator_under_the_kernel():
    """the settings of the experiment the estimator was proposed on: default HawkesJDParams, hawkes_cmc_twin.stat_chain, 2^15 paths of
    np_chain at seed 7 on ceil(dT x 480) steps per slice, the normals of default_rng(1) drawn expiry by expiry"""
    import stochvolmodels_amd as sv
    p = sv.HawkesJDParams().to_dict()
    n = 1 << 15
    chain, _ = hc.stat_chain(p)
    nb, dts, t0 = [], [], 0.0
    for t in hc.STAT_TTMS:
        nb.append(max(int(np.ceil((t - t0) * hc.STAT_SPY)), 1))
        dts.append((t - t0) / nb[-1])
        t0 = t
    states, cvs = hc.np_chain(p, 7, n, nb, dts), hc.host_cv(p["sigma"], nb, dts)
    rng = np.random.default_rng(1)
    z_normal = np.stack([rng.standard_normal(n) for _ in nb])
    figures, worst = 0, 0.0
    for gamma in (-3.0, -1.0, 1.0, 3.0):
        for i, ((mu, _, _), cv) in enumerate(zip(states, cvs)):
            k, t = chain["strikes_ttms"][i], chain["optiontypes_ttms"][i]
            cp, ce, cst = tc.estimator(mu, np.full(n, cv), 1.0, k, t, gamma)
            pp, pe, pst = tc.plain_tilted(mu + np.sqrt(cv) * z_normal[i], 1.0, k, t, gamma)
            z = np.asarray((cp - pp) / np.hypot(ce, pe), dtype=np.float64)
            ratio = np.asarray((pe / ce) ** 2, dtype=np.float64)
            print(f"gamma={gamma:+.0f} T={hc.STAT_TTMS[i]:.4f}: max |z| {np.max(np.abs(z)):.2f}, plain error^2 / conditional "
                  f"{ratio.min():.2f} .. {ratio.max():.2f} (median {np.median(ratio):.2f}), effective sample size / n "
                  f"{pst['effective_sample_size'] / n:.3f} -> {float(cst['effective_sample_size']) / n:.3f}")
            assert cst["n_kept"] == n and np.all(np.abs(z) <= Z_BOUND), (gamma, i, z)
            assert np.all(ce < pe), (gamma, i, ratio)
            assert float(cst["effective_sample_size"]) > pst["effective_sample_size"]
            figures += z.size
            worst = max(worst, float(np.max(np.abs(z))))
    print(f"{figures} figures, largest |z| {worst:.2f} (bound {Z_BOUND})")
    assert figures == 168


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def declared_ext():
    text = open(os.path.join(ROOT, "include", "svmc_ext.h")).read()
    return sorted(set(re.findall(r"SVMC_EXT_API\s+int\s+(svmc_[a-z0-9_]+)\s*\(", text)))


def test_the_second_library_exports_what_its_header_declares_and_the_core_is_closed():
    from stochvolmodels_amd import _lib, build
    build.build()
    assert os.path.exists(build.EXT_LIB) and os.path.basename(build.EXT_LIB) == "libsvmc_ext.so"
    assert declared_ext() == sorted(EXT_SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", build.EXT_LIB], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\bT (svmc_[a-z0-9_]+)", nm))) == declared_ext()
    undefined = subprocess.run(["nm", "-D", "--undefined-only", build.EXT_LIB], capture_output=True, text=True, check=True).stdout
    assert not re.search(r"\bsvmc_", undefined), "libsvmc_ext.so links nothing from libsvmc.so"
    E = _lib.load_ext()
    assert sorted(E._svmc_ext_symbols) == declared_ext() and E.svmc_ext_version() == 100
    # the core: 143 declared, 143 bound, and none of them is the new library's
    header = open(os.path.join(ROOT, "include", "svmc.h")).read()
    assert len(re.findall(r"^SVMC_API ", header, flags=re.M)) == 143
    L = _lib.load()
    assert len(L._svmc_symbols) == 143 and not set(L._svmc_symbols) & set(EXT_SYMBOLS)
    assert not any(hasattr(L, name) for name in EXT_SYMBOLS)
    out = subprocess.run(["strings", "-a", build.EXT_LIB], capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_host_only_entries_and_refusals_without_a_gpu():
    import ctypes as C
    from stochvolmodels_amd import _lib
    E = _lib.load_ext()
    nbytes = C.c_size_t(0)
    assert E.svmc_tilted_cond_workspace_bytes(257, 2, 24, 5, C.byref(nbytes)) == _lib.OK and nbytes.value > 0
    small = nbytes.value
    assert E.svmc_tilted_cond_workspace_bytes(1 << 20, 2, 24, 5, C.byref(nbytes)) == _lib.OK and nbytes.value > small
    for args in ((0, 2, 24, 5), (257, 0, 24, 5), (257, 2, 24, 0), (257, 2, 24, 17)):
        assert E.svmc_tilted_cond_workspace_bytes(*args, C.byref(nbytes)) == _lib.ERR_INVALID_ARGUMENT
    assert E.svmc_tilted_cond_workspace_bytes(257, 2, 24, 5, None) == _lib.ERR_INVALID_ARGUMENT


def test_the_new_kernels_use_no_scratch_and_the_core_keeps_its_kernels():
    from stochvolmodels_amd import build
    build.build()
    meta = json.load(open(build.EXT_ISA_JSON))["metadata"]
    assert len(meta) == 4, sorted(meta)
    for short, lds in LDS_BOUND.items():
        hit = [k for k in meta if short + "E" in k]         # (the mangled name: the identifier, then its argument list)
        assert len(hit) == 1, (short, sorted(meta))
        assert meta[hit[0]]["scratch_bytes"] == 0, (short, meta[hit[0]])
        assert meta[hit[0]]["lds_bytes"] <= lds, (short, meta[hit[0]])
    core = json.load(open(build.ISA_JSON))["metadata"]
    want = json.load(open(os.path.join(HERE, "golden", "libsvmc_kernel_names.json")))
    assert sorted(core) == sorted(want)
    assert not any("tilted_cond" in k for k in core)
    assert all(v["scratch_bytes"] == 0 for v in core.values())
    assert len([k for k in core if "cmc" in k]) == 8 and len([k for k in core if "hawkesjd" in k]) == 3


def test_the_library_is_stale_when_a_dependency_is_newer(tmp_path, monkeypatch):
    from stochvolmodels_amd import build
    build.build()
    assert not build.ext_is_stale() and not build.is_stale()
    lib = tmp_path / "libsvmc_ext.so"
    lib.write_bytes(b"")
    old = os.path.getmtime(build.EXT_SRC) - 10.0
    os.utime(lib, (old, old))
    monkeypatch.setattr(build, "EXT_LIB", str(lib))
    assert build.ext_is_stale()                             # older than its source
    monkeypatch.setattr(build, "EXT_LIB", str(tmp_path / "absent.so"))
    assert build.ext_is_stale()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
CHAIN = dict(ttms=np.array([0.25, 0.5]), forwards=np.array([1.0, 1.02]), discfactors=np.array([1.0, 0.99]),
             strikes_ttms=[np.array([[0.9, 1.0, 1.1]]), np.array([1.0])], optiontypes_ttms=[np.array([["C", "P", "C"]]), np.array(["P"])])


class Two:
    world, rank = 2, 0


class Recorder(FakeEngine):
    """the fake engine with the conditional call under the kernel recorded"""

    def price_hawkesjd_chain_tilted_cond(self, ch, params, nb_steps_per_year, seed, call_id, gammas, recenter):
        from stochvolmodels_amd.engine import tilted_results
        self.calls.append(("tilted_cond", ch, np.array(params), nb_steps_per_year, seed, call_id, np.array(gammas), recenter))
        G, K, m = len(gammas), ch["total"], ch["m"]
        prices = np.arange(G * K, dtype=np.float64) + 100.0 * np.repeat(np.asarray(gammas), K)
        stats = np.arange(G * m * 8, dtype=np.float64)
        return tilted_results(prices, -prices, stats, dict(ch, gammas=np.asarray(gammas)))

    def tilted_conditional_payoffs(self, forwards, strikes, codes, gammas, recenter=False, mu_rows=None, cv_rows=None, shifts=None):
        from stochvolmodels_amd.engine import tilted_chain_arrays, tilted_results
        ch = tilted_chain_arrays(forwards, strikes, codes, gammas)
        self.calls.append(("tail", ch, recenter, mu_rows, cv_rows, self.x.a.copy(), self.cv.a.copy()))
        G, K = ch["gammas"].size, ch["total"]
        return tilted_results(np.arange(G * K, dtype=np.float64), np.ones(G * K), np.arange(G * 8, dtype=np.float64), ch)

    # the host-array route uploads mu to x and cv to the fourth state array: both as the HIP engine's buffers, with a .ptr
    class _Buf:
        def __init__(self, n):
            self.a = np.zeros(n)
            self.ptr = self.a.ctypes.data

    def __init__(self, n_path):
        super().__init__(n_path)
        self.x, self.cv = self._Buf(n_path), self._Buf(n_path)

    def upload(self, ptr, host):
        import ctypes as C
        host = np.ascontiguousarray(host, dtype=np.float64)
        C.memmove(ptr, host.ctypes.data, host.nbytes)


@pytest.fixture
def fake(monkeypatch):
    from stochvolmodels_amd.pricers import hawkes_jd_pricer
    from stochvolmodels_amd.utils import mc_payoffs
    eng = Recorder(64)
    eng.requests = []
    for mod in (hawkes_jd_pricer, mc_payoffs):
        monkeypatch.setattr(mod, "get_engine", lambda n, *a, **k: eng.requests.append(n) or eng)
    return eng


def option_chain(sv, chain=CHAIN):
    """(an OptionChain's slices are one-dimensional)"""
    flat = dict(chain, strikes_ttms=[np.ravel(k) for k in chain["strikes_ttms"]],
                optiontypes_ttms=[np.ravel(t) for t in chain["optiontypes_ttms"]])
    return sv.OptionChain(ids=np.array(["a", "b"]), **flat)


def test_the_routes_refuse_before_any_engine_is_asked_for(fake):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import VariableType
    kw = sv.HawkesJDParams().to_dict()
    kw.pop("risk_premia_gamma")
    ic = dict(CHAIN, optiontypes_ttms=[np.array([["IC", "C", "C"]]), np.array(["P"])])
    ip = dict(CHAIN, optiontypes_ttms=[np.array([["C", "C", "C"]]), np.array(["IP"])])
    many = sv.hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas
    one = sv.hawkesjd_mc_chain_pricer_conditional_with_risk_premia
    for fn, g in ((many, dict(risk_premia_gammas=[-1.0, 1.0])), (one, dict(risk_premia_gamma=-1.0))):
        for inverse in (ic, ip):
            with pytest.raises(ValueError, match="not implemented"):
                fn(nb_path=64, seed=1, **inverse, **kw, **g)
        for vt in (VariableType.Q_VAR, VariableType.SIGMA):
            with pytest.raises(NotImplementedError):
                fn(nb_path=64, seed=1, variable_type=vt, **CHAIN, **kw, **g)
        with pytest.raises(NotImplementedError):
            fn(nb_path=64, seed=1, comm=Two(), **CHAIN, **kw, **g)
        with pytest.raises(NotImplementedError):
            fn(nb_path=64, seed=1, devices=2, **CHAIN, **kw, **g)
    for bad in ([], [0.0] * 17, [np.nan]):
        with pytest.raises(ValueError):
            many(nb_path=64, seed=1, risk_premia_gammas=bad, **CHAIN, **kw)
    with pytest.raises(ValueError, match="risk_premia_gamma must be set"):
        one(nb_path=64, seed=1, **CHAIN, **kw)
    pricer, params = sv.HawkesJDPricer(), sv.HawkesJDParams(risk_premia_gamma=0.5)
    route = pricer.model_mc_price_chain_conditional_with_risk_premia
    with pytest.raises(ValueError, match="risk_premia_gamma must be set"):
        route(option_chain(sv), sv.HawkesJDParams(), nb_path=64, seed=1)
    with pytest.raises(ValueError, match="not implemented"):
        route(option_chain(sv, ic), params, nb_path=64, seed=1)
    with pytest.raises(NotImplementedError):
        route(option_chain(sv), params, nb_path=64, seed=1, variable_type=VariableType.Q_VAR)
    with pytest.raises(NotImplementedError):
        route(option_chain(sv), params, nb_path=64, seed=1, comm=Two())
    with pytest.raises(NotImplementedError):
        route(option_chain(sv), params, nb_path=64, seed=1, devices=[0, 0])
    mu, cv = np.zeros(64), np.full(64, 0.04)
    with pytest.raises(ValueError, match="not implemented"):
        sv.compute_mc_vars_payoff_conditional_with_gamma(mu, cv, 1.0, np.array([1.0]), np.array(["IC"]), 0.5)
    with pytest.raises(NotImplementedError):
        sv.compute_mc_vars_payoff_conditional_with_gamma(mu, cv, 1.0, np.array([1.0]), np.array(["C"]), 0.5, variable_type=VariableType.Q_VAR)
    with pytest.raises(ValueError):
        sv.compute_mc_vars_payoff_conditional_with_gamma(mu, cv[:3], 1.0, np.array([1.0]), np.array(["C"]), 0.5)
    assert fake.requests == [] and fake.calls == []


def test_what_the_routes_hand_the_engine_and_their_shapes(fake):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    params = sv.HawkesJDParams(mu=0.01, sigma=0.3, lambda_p=5.0, lambda_m=7.0, risk_premia_gamma=0.25)
    kw = params.to_dict()
    kw.pop("risk_premia_gamma")
    gammas = [-1.0, 0.0, 2.0]
    prices, stderrs, fwds = sv.hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas(
        nb_path=777, seed=11, risk_premia_gammas=gammas, recenter_forward=True, return_forwards=True, **CHAIN, **kw)
    assert fake.requests == [777]
    what, ch, block, spy, seed, call_id, g, recenter = fake.calls[-1]
    assert what == "tilted_cond" and (spy, seed, call_id, recenter) == (hp.NB_STEPS_PER_YEAR, 11, 0, True) and spy == 1800
    assert block.tolist() == [float(params.to_dict()[k]) for k in hp.PARAM_NAMES] and g.tolist() == gammas
    assert ch["ttms"].tolist() == [0.25, 0.5] and ch["forwards"].tolist() == [1.0, 1.02] and ch["offs"].tolist() == [0, 3, 4]
    assert ch["strikes"].tolist() == [0.9, 1.0, 1.1, 1.0] and ch["codes"].tolist() == [0, 1, 0, 1]
    # [gamma][expiry] in the strikes' shapes; the third item per gamma (normalizers, gamma forwards, stats [m, 8])
    assert len(prices) == len(stderrs) == len(fwds) == 3
    assert [p.shape for p in prices[1]] == [(1, 3), (1,)] and prices[2][1].tolist() == [211.0] and stderrs[0][0].tolist() == [[100.0, 99.0, 98.0]]
    norm, gfwd, st = fwds[1]
    assert st.shape == (2, 8) and norm.tolist() == st[:, 0].tolist() == [16.0, 24.0] and gfwd.tolist() == [18.0, 26.0]
    # without return_forwards two items; nb_steps_per_year and the default recenter_forward=False are passed on
    out = sv.hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas(nb_path=777, seed=12, risk_premia_gammas=gammas,
                                                                          nb_steps_per_year=360, **CHAIN, **kw)
    assert len(out) == 2 and fake.calls[-1][3:6] == (360, 12, 0) and fake.calls[-1][7] is False
    # one gamma is the list form at that gamma
    p1, e1, f1 = sv.hawkesjd_mc_chain_pricer_conditional_with_risk_premia(nb_path=777, seed=11, risk_premia_gamma=2.0,
                                                                          return_forwards=True, **CHAIN, **kw)
    assert fake.calls[-1][6].tolist() == [2.0] and fake.calls[-1][3:6] == (1800, 11, 0)
    assert [p.shape for p in p1] == [(1, 3), (1,)] and len(f1) == 3 and f1[2].shape == (2, 8)
    p1, e1 = sv.hawkesjd_mc_chain_pricer_conditional_with_risk_premia(nb_path=777, seed=11, risk_premia_gamma=2.0, **CHAIN, **kw)
    assert p1[0].tolist() == [[200.0, 201.0, 202.0]] and e1[1].tolist() == [-203.0]
    # without a seed: the process seed and the NEXT call id, once per call
    sv.set_seed(2024)
    sv.hawkesjd_mc_chain_pricer_conditional_with_risk_premia(nb_path=777, risk_premia_gamma=2.0, **CHAIN, **kw)
    first = fake.calls[-1]
    sv.hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas(nb_path=777, risk_premia_gammas=gammas, **CHAIN, **kw)
    assert first[4] == fake.calls[-1][4] == 2024 and fake.calls[-1][5] == first[5] + 1
    # the class route: the chain's arrays, the parameter set's fields and ITS gamma
    sv.HawkesJDPricer().model_mc_price_chain_conditional_with_risk_premia(option_chain(sv), params, nb_path=777, seed=11,
                                                                          recenter_forward=True)
    assert fake.calls[-1][2].tolist() == block.tolist() and fake.calls[-1][6].tolist() == [0.25] and fake.calls[-1][7] is True


def test_the_host_array_route(fake):
    import stochvolmodels_amd as sv
    rng = np.random.default_rng(5)
    mu, cv = 0.1 * rng.standard_normal(64), 0.04 * rng.random(64)
    k, t = np.array([[0.9, 1.0], [1.1, 1.2]]), np.array([["P", "P"], ["C", "C"]])
    p, e, st = sv.compute_mc_vars_payoff_conditional_with_gamma(mu, cv, 1.05, k, t, -1.0, recenter=True, return_stats=True)
    assert fake.requests == [64]
    what, ch, recenter, mu_rows, cv_rows, x_up, cv_up = fake.calls[-1]
    assert what == "tail" and recenter is True and mu_rows is None and cv_rows is None
    assert np.array_equal(x_up, mu) and np.array_equal(cv_up, cv)
    assert ch["forwards"].tolist() == [1.05] and ch["gammas"].tolist() == [-1.0] and ch["codes"].tolist() == [1, 1, 0, 0]
    assert p.shape == e.shape == (2, 2) and p.tolist() == [[0.0, 1.0], [2.0, 3.0]]
    from stochvolmodels_amd.engine import TILTED_COND_STATS_FIELDS, TILTED_STATS_FIELDS
    assert TILTED_COND_STATS_FIELDS is TILTED_STATS_FIELDS and tuple(st) == TILTED_STATS_FIELDS and isinstance(st["n_kept"], int)
    # several gammas: lists, one entry per gamma
    ps, es = sv.compute_mc_vars_payoff_conditional_with_gamma(mu, cv, 1.05, k, t, [-1.0, 2.0])
    assert len(ps) == len(es) == 2 and ps[1].shape == (2, 2) and ps[1].tolist() == [[4.0, 5.0], [6.0, 7.0]]
    assert fake.calls[-1][1]["gammas"].tolist() == [-1.0, 2.0] and fake.calls[-1][2] is False
