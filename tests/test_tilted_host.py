"""
Host side of the Monte Carlo prices under the exponential risk-premia kernel, no GPU: every request the
pricers refuse is refused before the library is loaded; what the engine route sends to the library and how it cuts the answer
into the strikes' shapes, against a stand-in that records every call; the new names in the header, the ctypes table and the
package; the new kernels' registers in the build's metadata.
"""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest

import stochvolmodels_amd as sv
from stochvolmodels_amd import _lib, engine
from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN = dict(ttms=np.array([0.1, 0.2]), forwards=np.array([1.0, 1.01]), discfactors=np.array([0.99, 0.98]),
             strikes_ttms=[np.array([0.9, 1.0, 1.1]), np.array([1.0, 1.2])],
             optiontypes_ttms=[np.array(["P", "P", "C"]), np.array(["P", "C"])])


def model_kw():
    kw = hp.HawkesJDParams().to_dict()
    kw.pop("risk_premia_gamma")
    return kw


@pytest.fixture
def no_library(monkeypatch):
    """any attempt to load the library, or to make an engine, fails the test"""
    def boom(*a, **k):
        raise AssertionError("the library was loaded before the request was refused")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(hp, "get_engine", boom)
    from stochvolmodels_amd.utils import mc_payoffs
    monkeypatch.setattr(mc_payoffs, "get_engine", boom)


def test_refusals_come_before_the_library(no_library):
    gam = hp.hawkesjd_mc_chain_pricer_with_risk_premia_gammas
    one = hp.hawkesjd_mc_chain_pricer_with_risk_premia
    for bad in ("IC", "IP", "X"):
        chain = dict(CHAIN, optiontypes_ttms=[np.array(["P", bad, "C"]), np.array(["P", "C"])])
        with pytest.raises(ValueError, match="^not implemented$"):
            gam(risk_premia_gammas=[1.0], nb_path=64, seed=1, **chain, **model_kw())
        with pytest.raises(ValueError, match="^not implemented$"):
            sv.compute_mc_vars_payoff_with_gamma(np.zeros(8), 1.0, np.array([0.9, 1.0, 1.1]), np.array(["P", bad, "C"]), 1.0)
    for vt in (sv.VariableType.Q_VAR, sv.VariableType.SIGMA):
        with pytest.raises(NotImplementedError):
            gam(risk_premia_gammas=[1.0], nb_path=64, variable_type=vt, **CHAIN, **model_kw())
        with pytest.raises(NotImplementedError):
            sv.compute_mc_vars_payoff_with_gamma(np.zeros(8), 1.0, np.array([1.0]), np.array(["C"]), 1.0, variable_type=vt)
    for gammas in ([], list(np.zeros(engine.TILTED_MAX_GAMMAS + 1)), [np.nan], [1.0, np.inf]):
        with pytest.raises(ValueError):
            gam(risk_premia_gammas=gammas, nb_path=64, **CHAIN, **model_kw())
    with pytest.raises(ValueError):
        sv.compute_mc_vars_payoff_with_gamma(np.zeros(8), 1.0, np.array([1.0]), np.array(["C"]), np.nan)
    with pytest.raises(ValueError, match="risk_premia_gamma must be set for the risk-premia pricer"):
        one(nb_path=64, **CHAIN, **model_kw())
    with pytest.raises(ValueError, match="risk_premia_gamma must be set for the risk-premia pricer"):
        chain = sv.OptionChain(ttms=CHAIN["ttms"], forwards=CHAIN["forwards"], discfactors=CHAIN["discfactors"],
                               strikes_ttms=tuple(CHAIN["strikes_ttms"]), optiontypes_ttms=tuple(CHAIN["optiontypes_ttms"]), ids=None)
        sv.HawkesJDPricer().model_mc_price_chain_with_risk_premia(chain, hp.HawkesJDParams(), nb_path=64)
    with pytest.raises(ValueError):                              # one forward per maturity
        gam(risk_premia_gammas=[1.0], nb_path=64, **dict(CHAIN, forwards=np.array([1.0])), **model_kw())
    with pytest.raises(ValueError):                              # strikes and types of a slice differ in length
        gam(risk_premia_gammas=[1.0], nb_path=64, **dict(CHAIN, strikes_ttms=[np.array([0.9, 1.0]), np.array([1.0, 1.2])]), **model_kw())
    with pytest.raises(ValueError):
        gam(risk_premia_gammas=[1.0], nb_path=64, **dict(CHAIN, strikes_ttms=[np.array([0.9, np.nan, 1.0]), np.array([1.0, 1.2])]),
            **model_kw())
    world2 = types.SimpleNamespace(world=2, rank=0)
    for kw in (dict(comm=world2), dict(devices=[0, 1])):
        with pytest.raises(NotImplementedError):
            gam(risk_premia_gammas=[1.0], nb_path=64, **CHAIN, **model_kw(), **kw)
        with pytest.raises(NotImplementedError):
            one(risk_premia_gamma=1.0, nb_path=64, **CHAIN, **model_kw(), **kw)


def test_the_plain_pricer_still_ignores_gamma():
    import inspect
    assert inspect.signature(hp.hawkesjd_mc_chain_pricer).parameters["risk_premia_gamma"].default == 0.0
    assert "accepted and unused" in hp.hawkesjd_mc_chain_pricer.__doc__


class StubLib:
    """libsvmc stand-in: every call succeeds and is recorded; svmc_memcpy_d2h fills the destination with `answer`"""

    def __init__(self):
        self.calls, self.answer = [], None

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name,) + args)
            if name == "svmc_memcpy_d2h":
                a = np.ascontiguousarray(self.answer, dtype=np.float64)
                assert a.nbytes == args[2]
                C.memmove(args[0].value if hasattr(args[0], "value") else args[0], a.ctypes.data, a.nbytes)
            elif name == "svmc_host_alloc":
                self.pinned = np.zeros(args[1] // 8)
                args[0]._obj.value = self.pinned.ctypes.data
            return 0
        return call


def stub_engine(lib, n_path=1000):
    eng = engine.HipEngine.__new__(engine.HipEngine)
    ns = types.SimpleNamespace
    eng.lib, eng.n_path, eng.stream = lib, n_path, 9
    eng.x, eng.ws, eng.ws_bytes = ns(ptr=1 << 20), ns(ptr=1 << 21), 4096
    eng._snap = ns(offset=lambda k: (1 << 22) + 8 * k)
    eng._sums, eng._pinned, eng._pinned_doubles = {}, None, 0
    eng.alloc_sums = lambda n, tag="sums": ({"tilted": 1 << 24, "tilted_spot": 1 << 23}[tag], None)
    return eng


def test_engine_route_arguments_and_shapes():
    lib = StubLib()
    strikes = [np.array([[0.9, 1.0], [1.1, 1.2]]), np.array([1.0, 1.2, 1.3])]
    codes = [np.array([1, 1, 0, 0], dtype=np.int8), np.array([1, 0, 0], dtype=np.int8)]
    G, K, m = 2, 7, 2
    prices, stderrs = np.arange(G * K) + 0.25, np.arange(G * K) + 100.5
    stats = np.arange(G * m * 8) * 1.0
    lib.answer = np.concatenate([prices, stderrs, stats])
    eng = stub_engine(lib)
    p, e, s = eng.tilted_payoffs([1.0, 1.05], strikes, codes, [-1.0, 1.0], recenter=True, snap_rows=[3, 5])
    names = [c[0] for c in lib.calls]
    assert names.count("svmc_spot_sums") == 2 and names.count("svmc_tilted_payoff_chain") == 1 and names.count("svmc_memcpy_d2h") == 1
    assert names.index("svmc_tilted_payoff_chain") > max(i for i, c in enumerate(names) if c == "svmc_spot_sums")
    spots = [c for c in lib.calls if c[0] == "svmc_spot_sums"]
    assert [c[1] for c in spots] == [(1 << 22) + 8 * 3000, (1 << 22) + 8 * 5000] and [c[4] for c in spots] == [1 << 23, (1 << 23) + 16]
    c = next(c for c in lib.calls if c[0] == "svmc_tilted_payoff_chain")
    (_, xs, n, fw, n_exp, ks, cs, sh, offs, gm, n_g, recenter, spot, out_p, out_e, out_s, ws, ws_bytes, stream) = c
    assert list(xs) == [(1 << 22) + 8 * 3000, (1 << 22) + 8 * 5000] and (n, n_exp, n_g, recenter) == (1000, 2, 2, 1)
    assert [fw[i] for i in range(2)] == [1.0, 1.05] and [gm[i] for i in range(2)] == [-1.0, 1.0]
    assert [ks[i] for i in range(K)] == [0.9, 1.0, 1.1, 1.2, 1.0, 1.2, 1.3] and [cs[i] for i in range(K)] == [1, 1, 0, 0, 1, 0, 0]
    assert [offs[i] for i in range(3)] == [0, 4, 7]
    want = np.concatenate([engine.payoff_shifts(k.ravel(), cc, f, 1) for k, cc, f in zip(strikes, codes, (1.0, 1.05))])
    assert [sh[i] for i in range(K)] == want.tolist()                       # the intrinsic values at the forward
    assert (spot, out_p, out_e, out_s) == (1 << 23, 1 << 24, (1 << 24) + 8 * G * K, (1 << 24) + 16 * G * K)
    assert (ws, ws_bytes, stream) == (1 << 21, 4096, 9)
    for g in range(G):
        assert p[g][0].shape == e[g][0].shape == (2, 2) and p[g][1].shape == (3,)
        assert np.array_equal(p[g][0].ravel(), prices[g * K:g * K + 4]) and np.array_equal(p[g][1], prices[g * K + 4:g * K + 7])
        assert np.array_equal(e[g][1], stderrs[g * K + 4:g * K + 7])
    assert s.shape == (G, m, 8) and np.array_equal(s.ravel(), stats)
    # the current state serves one expiry, with no recentring sums unless asked for
    lib.calls.clear()
    lib.answer = np.zeros(2 * 3 + 8)
    p, e, s = eng.tilted_payoffs([1.0], [strikes[1]], [codes[1]], [0.5])
    c = next(c for c in lib.calls if c[0] == "svmc_tilted_payoff_chain")
    assert list(c[1]) == [1 << 20] and c[11] == 0 and c[12] is None and "svmc_spot_sums" not in [k[0] for k in lib.calls]
    with pytest.raises(ValueError):
        eng.tilted_payoffs([1.0, 1.05], strikes, codes, [0.5])
    d = engine.tilted_stats_dicts(np.arange(16.0).reshape(2, 8))
    assert list(d[0]) == list(engine.TILTED_STATS_FIELDS) and d[1]["n_kept"] == 13 and isinstance(d[1]["n_dropped"], int)


def test_new_symbols_in_header_ctypes_and_package():
    text = open(os.path.join(ROOT, "include", "svmc.h")).read()
    src = open(os.path.join(ROOT, "stochvolmodels_amd", "_lib.py")).read()
    for name in ("svmc_tilted_payoff_chain", "svmc_hawkesjd_chain_price_tilted"):
        assert re.search(r"SVMC_API int " + name + r"\(", text) and f'"{name}"' in src
    assert int(re.search(r"#define SVMC_TILTED_MAX_GAMMAS (\d+)", text).group(1)) == engine.TILTED_MAX_GAMMAS
    assert int(re.search(r"#define SVMC_TILTED_STATS_DOUBLES (\d+)", text).group(1)) == engine.TILTED_STATS_DOUBLES
    assert len(engine.TILTED_STATS_FIELDS) == engine.TILTED_STATS_DOUBLES
    assert "KEEP RULE" in text and "(w_j spot_j)^2 are all finite" in text
    for name in ("compute_mc_vars_payoff_with_gamma", "hawkesjd_mc_chain_pricer_with_risk_premia",
                 "hawkesjd_mc_chain_pricer_with_risk_premia_gammas"):
        assert name in sv.__all__ and callable(getattr(sv, name))
    assert callable(sv.HawkesJDPricer.model_mc_price_chain_with_risk_premia)
    assert "accepted and ignored" in hp.hawkesjd_mc_chain_pricer_with_risk_premia_gammas.__doc__


def test_new_kernels_use_no_scratch_and_only_the_block_sums_lds():
    path = os.path.join(ROOT, "stochvolmodels_amd", "libsvmc.isa.json")
    if not os.path.exists(path):
        from stochvolmodels_amd import build
        build.build()
    meta = json.load(open(path))["metadata"]
    tilted = {k: v for k, v in meta.items() if "tilted_payoff_group_kernel" in k}
    widths = sorted(int(re.search(r"tilted_payoff_group_kernelILi(\d+)E", k).group(1)) for k in tilted)
    assert widths == [4, 8, 16, 22]
    for name, v in tilted.items():
        kt = int(re.search(r"KernelILi(\d+)E|kernelILi(\d+)E", name).group(2))
        nv = 3 * kt + 7
        assert v["scratch_bytes"] == 0, name
        assert v["lds_bytes"] == 8 * 4 * ((nv + 7) // 8 * 8), name          # the block sum's exchange buffer, nothing else
        assert v["vgpr"] <= (168 if kt <= 4 else 256), name                 # three / two waves per SIMD
    finish = [v for k, v in meta.items() if "tilted_finish_kernel" in k]
    assert len(finish) == 1 and finish[0]["scratch_bytes"] == 0 and finish[0]["lds_bytes"] == 0
    assert all(v["scratch_bytes"] == 0 for v in meta.values())              # no kernel of the library spills


def test_the_stepping_kernels_are_what_they_were():
    """the feature adds kernels beside the stepping kernels and must leave those alone: the same kernels, and for each the
    scratch, the LDS and the waves per SIMD its registers allow (512 VGPRs per lane in units of 8, at most 8 waves) as in the
    record taken before the tilted kernels existed (tests/golden/stepping_kernel_registers.json).  Exact register counts move
    with the compiler and are not held."""
    path = os.path.join(ROOT, "stochvolmodels_amd", "libsvmc.isa.json")
    if not os.path.exists(path):
        from stochvolmodels_amd import build
        build.build()
    meta = json.load(open(path))["metadata"]
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "stepping_kernel_registers.json")))
    held = lambda v: (v["scratch_bytes"], v["lds_bytes"], min(8, 512 // ((v["vgpr"] + 7) // 8 * 8)))     # noqa: E731
    got = {k: held(v) for k, v in meta.items() if "rng_kernel" in k}
    assert len(want) >= 6 and got == {k: held(v) for k, v in want.items()}
