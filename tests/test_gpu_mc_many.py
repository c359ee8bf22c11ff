"""
Many independent jobs of one chain in one call (svmc_logsv_chain_price_many / svmc_heston_chain_price_many and the Python
functions over them): every job's prices and standard errors are np.array_equal to the single call with the job's parameters
and stream, on either side of the few-waves / full-launch switch, for the chain variants, unseeded, chunked, through the
pricer methods and from C; a batch leaves later single calls unchanged; the C ABI's error codes.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

import stochvolmodels_amd as sv
from stochvolmodels_amd import _lib
from stochvolmodels_amd.engine import MANY_MAX_JOBS, marshalled_chain, option_type_codes
from stochvolmodels_amd.utils.config import VariableType
from stochvolmodels_amd.utils.funcs import get_rng_state, set_seed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LP = sv.LOGSV_BTC_PARAMS


def chain_4x13():
    """the 4 x 13 chain of tools/bench_calibration_mc.py"""
    ttms = np.array([1 / 12, 0.25, 0.5, 1.0])
    k = np.linspace(0.7, 1.3, 13)
    strikes = [k.copy() for _ in ttms]
    types = [np.where(k < 1.0, "P", "C") for _ in ttms]
    return dict(ttms=ttms, forwards=np.ones(4), discfactors=np.ones(4), strikes_ttms=strikes, optiontypes_ttms=types)


def logsv_sets(n):
    """n distinct LogSV parameter sets; the third carries a vol backbone (etas != 1)"""
    out = []
    for j in range(n):
        p = sv.LogSvParams(sigma0=LP.sigma0 * (1.0 + 0.05 * j), theta=LP.theta * (1.0 - 0.03 * j), kappa1=LP.kappa1,
                           kappa2=LP.kappa2 + 0.1 * j, beta=LP.beta - 0.05 * j, volvol=LP.volvol * (1.0 - 0.02 * j))
        if j == 2:
            p.vol_backbone = pd.Series([0.8, 1.0, 1.2, 1.1], index=[1 / 12, 0.25, 0.5, 1.0])
        out.append(p)
    return out


def logsv_single(p, ch, seed=None, **kw):
    return sv.logsv_mc_chain_pricer(v0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2, beta=p.beta, volvol=p.volvol,
                                    vol_backbone_etas=p.get_vol_backbone_etas(ttms=ch["ttms"]), seed=seed, **ch, **kw)


def heston_single(p, ch, seed=None, **kw):
    return sv.heston_mc_chain_pricer(v0=p.v0, theta=p.theta, kappa=p.kappa, rho=p.rho, volvol=p.volvol, seed=seed, **ch, **kw)


def assert_same(batch, singles):
    assert len(batch) == len(singles)
    for j, ((bp, be), (sp, se)) in enumerate(zip(batch, singles)):
        for i, (a, b) in enumerate(zip(bp, sp)):
            assert np.array_equal(a, b), (j, i, a, b)
        for i, (a, b) in enumerate(zip(be, se)):
            assert np.array_equal(a, b), (j, i, a, b)


def test_logsv_distinct_params_and_seeds():
    ch = chain_4x13()
    sets = logsv_sets(5)
    assert not np.all(sets[2].get_vol_backbone_etas(ttms=ch["ttms"]) == 1.0)
    seeds = [11, 22, 33, 44, 55]
    batch = sv.logsv_mc_chain_pricer_many(sets, nb_path=100_000, seeds=seeds, **ch)
    assert_same(batch, [logsv_single(p, ch, s, nb_path=100_000) for p, s in zip(sets, seeds)])
    assert not np.array_equal(batch[0][0][0], batch[1][0][0])


@pytest.mark.parametrize("n_jobs,nb_path", [(4, 100_000), (5, 100_000), (3, 30_011)])
def test_either_side_of_the_form_switch(n_jobs, nb_path):
    """4 x 10^5 paths run the few-waves form, 5 x 10^5 are past the 458 752-path switch; 30 011 leaves every job a partial
    last block"""
    ch = chain_4x13()
    sets = logsv_sets(n_jobs)
    seeds = [100 + j for j in range(n_jobs)]
    batch = sv.logsv_mc_chain_pricer_many(sets, nb_path=nb_path, seeds=seeds, **ch)
    assert_same(batch, [logsv_single(p, ch, s, nb_path=nb_path) for p, s in zip(sets, seeds)])


def test_chain_variants_qvar_and_inverse_measure():
    ch = chain_4x13()
    sets = logsv_sets(3)
    seeds = [7, 8, 9]
    q = sv.logsv_mc_chain_pricer_many(sets, nb_path=50_000, seeds=seeds, variable_type=VariableType.Q_VAR, **ch)
    assert_same(q, [logsv_single(p, ch, s, nb_path=50_000, variable_type=VariableType.Q_VAR) for p, s in zip(sets, seeds)])
    inv = dict(ch, optiontypes_ttms=[np.where(np.asarray(k) < 1.0, "IP", "IC") for k in ch["strikes_ttms"]])
    b = sv.logsv_mc_chain_pricer_many(sets, nb_path=50_000, seeds=seeds, is_spot_measure=False, **inv)
    assert_same(b, [logsv_single(p, inv, s, nb_path=50_000, is_spot_measure=False) for p, s in zip(sets, seeds)])


def test_unseeded_batch_takes_consecutive_call_ids():
    ch = chain_4x13()
    sets = logsv_sets(4)
    set_seed(2024)
    singles = [logsv_single(p, ch, nb_path=40_000) for p in sets]
    after_singles = get_rng_state()
    set_seed(2024)
    batch = sv.logsv_mc_chain_pricer_many(sets, nb_path=40_000, **ch)
    assert get_rng_state() == after_singles == (2024, 4)
    assert_same(batch, singles)


def test_heston_euler_and_qe():
    ch = chain_4x13()
    euler = [sv.HestonParams(v0=0.04, theta=0.04, kappa=4.0, rho=-0.5, volvol=0.4),
             sv.HestonParams(v0=0.8, theta=1.0, kappa=2.0, rho=0.0, volvol=2.0),
             sv.HestonParams(v0=0.09, theta=0.06, kappa=2.0, rho=-0.7, volvol=0.6)]
    seeds = [3, 4, 5]
    b = sv.heston_mc_chain_pricer_many(euler, nb_path=100_000, seeds=seeds, **ch)
    assert_same(b, [heston_single(p, ch, s, nb_path=100_000) for p, s in zip(euler, seeds)])
    # QE: a set whose QE step is quadratic-only (Feller, rho <= 0) and one that is not -- the batch runs the general kernel
    quad, general = euler[0], sv.HestonParams(v0=0.04, theta=0.04, kappa=1.0, rho=-0.5, volvol=1.0)   # volvol^2 > 3 kappa theta
    for sets in ([quad, general], [quad]):
        s2 = seeds[:len(sets)]
        b = sv.heston_mc_chain_pricer_many(sets, nb_path=100_000, seeds=s2, scheme="qe", **ch)
        assert_same(b, [heston_single(p, ch, s, nb_path=100_000, scheme="qe") for p, s in zip(sets, s2)])


def test_edge_sizes_one_job_and_past_the_cap():
    ch = chain_4x13()
    p = logsv_sets(1)
    assert_same(sv.logsv_mc_chain_pricer_many(p, nb_path=20_000, seeds=[77], **ch), [logsv_single(p[0], ch, 77, nb_path=20_000)])
    n = MANY_MAX_JOBS + 3
    sets = [logsv_sets(5)[j % 5] for j in range(n)]
    seeds = [1000 + j for j in range(n)]
    batch = sv.logsv_mc_chain_pricer_many(sets, nb_path=4096, seeds=seeds, **ch)
    assert_same(batch, [logsv_single(q, ch, s, nb_path=4096) for q, s in zip(sets, seeds)])


def test_pricer_methods():
    c = chain_4x13()
    chain = sv.OptionChain(ids=None, **c)
    sets = logsv_sets(3)
    seeds = [21, 22, 23]
    b = sv.LogSVPricer().model_mc_price_chain_many(chain, sets, nb_path=30_000, seeds=seeds)
    assert_same(b, [sv.LogSVPricer().model_mc_price_chain(chain, p, nb_path=30_000, seed=s) for p, s in zip(sets, seeds)])
    hs = [sv.HestonParams(), sv.HestonParams(v0=0.09, rho=-0.3)]
    b = sv.HestonPricer().model_mc_price_chain_many(chain, hs, nb_path=30_000, seeds=seeds[:2], scheme="qe")
    assert_same(b, [sv.HestonPricer().model_mc_price_chain(chain, p, nb_path=30_000, seed=s, scheme="qe")
                    for p, s in zip(hs, seeds[:2])])


def test_a_batch_leaves_later_single_calls_unchanged():
    ch = chain_4x13()
    p = logsv_sets(1)[0]
    before = logsv_single(p, ch, 5, nb_path=60_000)
    sv.logsv_mc_chain_pricer_many(logsv_sets(6), nb_path=60_000, seeds=list(range(6)), variable_type=VariableType.Q_VAR, **ch)
    sv.heston_mc_chain_pricer_many([sv.HestonParams()] * 2, nb_path=60_000, seeds=[1, 2], **ch)
    assert_same([logsv_single(p, ch, 5, nb_path=60_000)], [before])


def test_error_codes():
    L = _lib.load()
    ch = chain_4x13()
    m = marshalled_chain(ch["ttms"], ch["forwards"], ch["discfactors"], ch["strikes_ttms"],
                         [option_type_codes(t) for t in ch["optiontypes_ttms"]])
    dp = C.POINTER(C.c_double)
    params = np.tile(np.r_[LP.sigma0, LP.theta, LP.kappa1, LP.kappa2, LP.beta, LP.volvol, np.ones(4)], (2, 1))
    seeds = np.array([1, 2], dtype=np.uint64)
    ids = np.zeros(2, dtype=np.uint32)
    out = np.zeros((2, 2, m["total"]))
    args = lambda sess, n_jobs, pp=params.ctypes.data_as(dp): (  # noqa: E731
        sess, m["ttms"], m["forwards"], m["discfactors"], 4, m["strikes"], m["codes"], m["offsets"], n_jobs, pp,
        seeds.ctypes.data_as(C.POINTER(C.c_uint64)), ids.ctypes.data_as(C.POINTER(C.c_uint32)), 1, 120, 1,
        out[0].ctypes.data_as(dp), out[1].ctypes.data_as(dp))
    sess = C.c_void_p()
    assert L.svmc_session_create(C.byref(sess), 4096, 4, m["total"]) == 0
    small = C.c_void_p()
    assert L.svmc_session_create(C.byref(small), 4096, 2, m["total"]) == 0
    try:
        assert L.svmc_logsv_chain_price_many(*args(sess, 0)) == 1                    # SVMC_ERR_INVALID_ARGUMENT
        assert L.svmc_logsv_chain_price_many(*args(sess, MANY_MAX_JOBS + 1)) == 1
        assert L.svmc_logsv_chain_price_many(*args(sess, 2, None)) == 1               # null params
        assert L.svmc_logsv_chain_price_many(*args(None, 2)) == 1                     # null session
        assert L.svmc_logsv_chain_price_many(*args(small, 2)) == 5                    # SVMC_ERR_WORKSPACE: chain > session
        hp = np.tile([0.04, 0.04, 4.0, -0.5, 0.4], (2, 1))
        a = list(args(small, 2, hp.ctypes.data_as(dp)))
        a[12] = 0                                                                   # Euler
        assert L.svmc_heston_chain_price_many(*a) == 5
        a[0], a[8] = sess, 0
        assert L.svmc_heston_chain_price_many(*a) == 1
        a[8], a[12] = 2, 7                                                          # unknown scheme
        assert L.svmc_heston_chain_price_many(*a) == 1
        assert L.svmc_logsv_chain_price_many(*args(sess, 2)) == 0                    # and the same call, well formed, runs
        assert np.all(np.isfinite(out))
    finally:
        L.svmc_session_destroy(sess)
        L.svmc_session_destroy(small)


def test_c_example_matches_the_python_batch(tmp_path):
    from stochvolmodels_amd import build
    lib = build.build()
    exe = str(tmp_path / "price_chain_many")
    libdir = os.path.dirname(lib)
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "price_chain_many.c"), "-o", exe, "-L" + libdir, "-lsvmc",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-lm"], check=True)
    n, seed = 32768, 20240601
    res = json.loads(subprocess.run([exe, str(n), str(seed)], capture_output=True, text=True, check=True, timeout=120).stdout)
    ch = dict(ttms=np.array([0.1, 0.25]), forwards=np.array([1.0, 1.01]), discfactors=np.array([0.99, 0.98]),
              strikes_ttms=[np.array([0.8, 1.0, 1.2]), np.array([0.8, 1.0, 1.2]) * 1.01],
              optiontypes_ttms=[np.array(["P", "C", "C"]), np.array(["IP", "IC", "C"])])
    lsets = [sv.LogSvParams(sigma0=0.8376, theta=1.0413, kappa1=3.1844, kappa2=3.058, beta=0.1514, volvol=1.8458),
             sv.LogSvParams(sigma0=0.6, theta=0.7, kappa1=2.0, kappa2=2.5, beta=-0.3, volvol=1.2),
             sv.LogSvParams(sigma0=0.8376, theta=1.0413, kappa1=3.1844, kappa2=3.058, beta=0.1514, volvol=1.8458)]
    # job 2's etas (0.9, 1.1): the Python batch takes them from a vol backbone
    lsets[2].vol_backbone = pd.Series([0.9, 1.1], index=[0.1, 0.25])
    assert np.array_equal(lsets[2].get_vol_backbone_etas(ttms=ch["ttms"]), [0.9, 1.1])
    seeds = [seed + j for j in range(3)]
    b = sv.logsv_mc_chain_pricer_many(lsets, nb_path=n, nb_steps_per_year=120, seeds=seeds, **ch)
    assert np.array_equal(np.concatenate([np.concatenate(pr) for pr, _ in b]), res["logsv_prices"])
    assert np.array_equal(np.concatenate([np.concatenate(se) for _, se in b]), res["logsv_stderrs"])
    hsets = [sv.HestonParams(v0=0.04, theta=0.04, kappa=4.0, rho=-0.5, volvol=0.4),
             sv.HestonParams(v0=0.09, theta=0.06, kappa=2.0, rho=-0.7, volvol=0.6),
             sv.HestonParams(v0=0.8, theta=1.0, kappa=2.0, rho=0.0, volvol=2.0)]
    b = sv.heston_mc_chain_pricer_many(hsets, nb_path=n, seeds=seeds, **ch)
    assert np.array_equal(np.concatenate([np.concatenate(pr) for pr, _ in b]), res["heston_prices"])
    assert np.array_equal(np.concatenate([np.concatenate(se) for _, se in b]), res["heston_stderrs"])
