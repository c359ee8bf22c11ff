"""
The Hawkes jump-diffusion's CPU gate: the NumPy twin of the generator (tests/hawkes_twin.py) against the fixtures the unmodified
reference produced on the same stream (tests/golden/make_golden_hawkes.py), the twin's Philox and inverse normal CDF against
the C oracle bit for bit, the parameter dataclass against the reference's, and the host-side errors of the pricer module.
No GPU needed.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import hawkes_twin as twin


def _chain(f):
    m = f["ttms"].size
    return (f["ttms"], f["forwards"], f["discfactors"], [f[f"strikes_{i}"] for i in range(m)], [f[f"types_{i}"] for i in range(m)])


def _params(f):
    return dict(zip(twin.PARAM_NAMES, f["params"]))


@pytest.mark.parametrize("name", ["hawkes_mc", "hawkes_mc_excited"])
def test_twin_reproduces_the_reference_on_the_stream(golden, name):
    f = golden(name)
    ttms, fw, df, ks, ts = _chain(f)
    stats = {}
    prices, stderrs, states = twin.mc_chain(ttms, fw, df, ks, ts, _params(f), int(f["n_path"]), int(f["seed"]), keep=256,
                                            stats=stats)
    np.testing.assert_allclose(np.stack(states), f["states"], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(np.concatenate(prices), f["prices"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(np.concatenate(stderrs), f["stderrs"], rtol=1e-12, atol=1e-15)
    assert (stats["jumps_p"], stats["jumps_m"], stats["both"]) == (int(f["jumps_p"]), int(f["jumps_m"]), int(f["jumps_both"]))
    assert stats["both"] > 100                 # clustered jumps: both sides in one step are exercised
    assert int(f["nb_steps_total"]) == 780


def test_numpy_philox_is_the_oracles_at_seven_rounds(oracle):
    f = oracle.lib().svo_philox4x32
    u32 = C.c_uint32
    f.argtypes = [C.POINTER(u32), C.POINTER(u32), C.c_int, C.POINTER(u32)]
    f.restype = None
    rng = np.random.default_rng(7)
    ctr = rng.integers(0, 1 << 32, size=(256, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, size=(256, 2), dtype=np.uint64)
    ctr[:4] = [[0, 0, 0, 0], [0xFFFFFFFF] * 4, [1, 0, 780, 6], [4095, 0, 779, 7 | 5 << 8]]
    for c, k in zip(ctr, key):
        mine = twin.philox4x32(*[np.uint64(v) for v in c], int(k[0]), int(k[1]))
        out = (u32 * 4)()
        f((u32 * 4)(*[int(v) for v in c]), (u32 * 2)(int(k[0]), int(k[1])), 7, out)
        assert tuple(int(v) for v in mine) == tuple(out)
    # vectorised over a whole block of counters: the same words as one at a time
    many = twin.philox4x32(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], 12345, 678)
    one = twin.philox4x32(ctr[17, 0], ctr[17, 1], ctr[17, 2], ctr[17, 3], 12345, 678)
    assert tuple(int(w[17]) for w in many) == tuple(int(w) for w in one)


def test_vectorised_normals_are_the_oracles_bit_for_bit(oracle):
    rng = np.random.default_rng(3)
    words = [rng.integers(0, 1 << 32, size=4096, dtype=np.uint64).astype(np.uint32)]
    special = [0, 0x80000000, 1, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000001]      # z = 0 at the two unpaired words
    m = twin.icdf_table()[0]
    for e in range(31):                                                     # every segment edge, both signs, +-1
        for k in range(1 << m):
            v = int((1 << e) * (1 + k / (1 << m)))
            for d in (-1, 0, 1):
                if 0 < v + d < (1 << 31):
                    special += [v + d, (-(v + d)) & 0xFFFFFFFF]
    words.append(np.array(special, dtype=np.uint32))
    w = np.concatenate(words)
    z = twin.normal_from_words(w)
    ref = np.array([oracle.normal_from_word(int(x)) for x in w])
    assert np.array_equal(z.view(np.int64), ref.view(np.int64))
    assert z[4096] == 0.0 and z[4097] == 0.0


def test_emulated_fma_rounds_once():
    # (1 + 2^-52)(1 - 2^-52) - 1 = -2^-104 exactly: a separate multiply rounds the product to 1 and returns 0
    a, b = 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52
    assert twin.fma(a, b, -1.0) == -(2.0 ** -104)
    rng = np.random.default_rng(11)
    x, y, c = rng.standard_normal((3, 1000))
    from fractions import Fraction
    for i in range(0, 1000, 97):
        exact = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(c[i]))
        assert twin.fma(x[i], y[i], c[i]) == float(exact)


def test_dataclass_matches_the_references(golden):
    from stochvolmodels_amd.pricers.hawkes_jd_pricer import PARAM_NAMES, HawkesJDParams
    f = golden("hawkes_analytic")
    p = HawkesJDParams()
    assert [fl.name for fl in dataclasses.fields(HawkesJDParams)] == list(PARAM_NAMES) + ["risk_premia_gamma"]
    assert PARAM_NAMES == twin.PARAM_NAMES
    np.testing.assert_array_equal([getattr(p, k) for k in PARAM_NAMES], f["params"])
    np.testing.assert_array_equal([p.compensator_p, p.compensator_m], f["compensators"])
    np.testing.assert_array_equal([p.jump1_cond, p.jump2_cond], f["conds"])
    e = HawkesJDParams(**dict(zip(PARAM_NAMES, f["excited_params"])))
    np.testing.assert_array_equal([e.compensator_p, e.compensator_m], f["excited_compensators"])
    np.testing.assert_array_equal([e.jump1_cond, e.jump2_cond], f["excited_conds"])
    q = HawkesJDParams.copy(p)
    assert q == p and q.compensator_p == p.compensator_p
    assert p.exp_jump_p == p.shift_p + p.mean_p and p.jumps_var_m == p.shift_m ** 2 + p.mean_m ** 2


def test_root_exports():
    import stochvolmodels_amd as svm
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    assert svm.HawkesJDParams is hp.HawkesJDParams and svm.HawkesJDPricer is hp.HawkesJDPricer
    assert {"HawkesJDParams", "HawkesJDPricer"} <= set(svm.__all__)


def test_host_logic_errors(golden):
    """the errors raise on the host, before any device work"""
    from stochvolmodels_amd.data.option_chain import OptionChain
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    from stochvolmodels_amd.utils.config import VariableType
    f = golden("hawkes_mc")
    ttms, fw, df, ks, ts = _chain(f)
    p = hp.HawkesJDParams()
    kw = {k: v for k, v in p.to_dict().items()}
    for vt in (VariableType.Q_VAR, VariableType.SIGMA):
        with pytest.raises(NotImplementedError):
            hp.hawkesjd_mc_chain_pricer(ttms=ttms, forwards=fw, discfactors=df, strikes_ttms=ks, optiontypes_ttms=ts,
                                        nb_path=64, variable_type=vt, **kw)
        with pytest.raises(NotImplementedError):
            hp.hawkesjd_chain_pricer(model_params=p, ttms=ttms, forwards=fw, discfactors=df, strikes_ttms=ks,
                                     optiontypes_ttms=ts, variable_type=vt)
    chain = OptionChain(ttms=ttms, forwards=fw, discfactors=df, strikes_ttms=tuple(ks), optiontypes_ttms=tuple(ts), ids=None)
    with pytest.raises(NotImplementedError):
        hp.HawkesJDPricer().price_chain(chain, hp.HawkesJDParams(risk_premia_gamma=0.5))
    np.testing.assert_array_equal(hp.params_block(**kw), f["params"])
    assert hp.set_vol_scaler(0.45, 0.02) == np.clip(0.45, 0.2, 0.5) * np.sqrt(0.02)
    assert hp.NB_STEPS_PER_YEAR == 1800


def test_sharded_default_comm_raises(monkeypatch, golden):
    from stochvolmodels_amd import dist as svdist
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp

    class TwoRanks:
        rank, world = 0, 2

    monkeypatch.setattr(svdist, "get_default_comm", lambda: TwoRanks())
    f = golden("hawkes_mc")
    ttms, fw, df, ks, ts = _chain(f)
    with pytest.raises(NotImplementedError):
        hp.hawkesjd_mc_chain_pricer(ttms=ttms, forwards=fw, discfactors=df, strikes_ttms=ks, optiontypes_ttms=ts, nb_path=64,
                                    **hp.HawkesJDParams().to_dict())
