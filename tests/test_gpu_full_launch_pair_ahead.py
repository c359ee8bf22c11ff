"""The full-launch LogSV stepping kernels (logsv_rng_kernel, logsv_chain_rng_kernel, logsv_chain_rng_many_kernel) run their time
loop one pair of normals ahead (svmc_rng.h rng_time_loop_pair_ahead): an odd first step, the full calls, an even last step are
three pieces of code, so a slice's first and last chain-global step decide which of them run.  Every case here is priced twice,
each time in a child process of its own, because SVMC_FEW_WAVES_MAX_PATHS is read once per process:

    default                        the few-waves kernels (at these path counts), the pipelined loop
    SVMC_FEW_WAVES_MAX_PATHS=0     the full-launch kernels

The two families perform the same operations on the same Philox words, so prices, standard errors and terminal states are
compared bit for bit.  Path counts 1, 63, 64, 65, 511, 512, 513, 1025 (a lone lane, a partial and a full wave, a partial and a full
512-thread block, a second 1024-thread block); chains with steps per expiry (3, 4, 1), (1,) and (2, 2) -- slices that start and
end on odd and on even global steps --, both payoff kinds, the many-job entry point with two jobs, and one 7-step slice with step
offsets 3 and 4 through the C ABI (HipEngine.logsv_rng).  One case is also held to the CPU oracle on the same stream.

As a program this file is the child:  python tests/test_gpu_full_launch_pair_ahead.py OUT.npz"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

PATHS = (1, 63, 64, 65, 511, 512, 513, 1025)
SPY = 10
# ttms -> steps per expiry int(dT * SPY) + 1
CHAINS = {"s341": (np.array([0.25, 0.6, 0.65]), (3, 4, 1)), "s1": (np.array([0.05]), (1,)), "s22": (np.array([0.15, 0.3]), (2, 2))}
KINDS = ("LOG_RETURN", "Q_VAR")
SEED, SEED_OTHER = 20240611, 77
OFFSETS = (3, 4)                                           # 7 steps from an odd and from an even chain-global step
ORACLE_CASE = ("s341", 513)
ST = dict(rtol=1e-11, atol=1e-13)                          # the parity tests' tolerance against the oracle (tests/test_gpu_parity.py)


def chain_keywords(name, kind):
    ttms, _ = CHAINS[name]
    m = len(ttms)
    fw = np.array([1.0, 1.02, 0.97])[:m]
    if kind == "Q_VAR":
        strikes, types = [np.array([0.02, 0.1, 0.4])] * m, [np.array(["C", "P", "C"])] * m
    else:
        strikes, types = [f * np.array([0.8, 1.0, 1.2]) for f in fw], [np.array(["P", "C", "C"])] * m
    return dict(ttms=ttms, forwards=fw, discfactors=np.full(m, 0.99), strikes_ttms=strikes, optiontypes_ttms=types,
                nb_steps_per_year=SPY)


def child(out_path):
    sys.path.insert(0, ROOT)
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.engine import HipEngine
    from stochvolmodels_amd.utils.funcs import time_grid_steps

    p = sv.LOGSV_BTC_PARAMS
    other = sv.LogSvParams(sigma0=1.1 * p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2 + 0.2, beta=p.beta, volvol=0.9 * p.volvol)
    for ttms, steps in CHAINS.values():
        assert tuple(time_grid_steps(float(d), SPY)[0] for d in np.diff(np.concatenate([[0.0], ttms]))) == steps
    out = {}
    for n in PATHS:
        for name, (ttms, _) in CHAINS.items():
            for kind in KINDS:
                kw = dict(chain_keywords(name, kind), nb_path=n, variable_type=getattr(sv.VariableType, kind))
                pr, sd = sv.logsv_mc_chain_pricer(v0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2, beta=p.beta, volvol=p.volvol,
                                                  vol_backbone_etas=np.ones(len(ttms)), seed=SEED, **kw)
                out[f"single_{name}_{kind}_{n}_prices"], out[f"single_{name}_{kind}_{n}_stderrs"] = np.stack(pr), np.stack(sd)
                if name == "s341":
                    for j, (jpr, jsd) in enumerate(sv.logsv_mc_chain_pricer_many([p, other], seeds=[SEED, SEED_OTHER], **kw)):
                        out[f"many{j}_{name}_{kind}_{n}_prices"], out[f"many{j}_{name}_{kind}_{n}_stderrs"] = np.stack(jpr), np.stack(jsd)
        eng = HipEngine(n)
        try:
            for off in OFFSETS:
                eng.set_state(np.zeros(n), np.full(n, p.sigma0), np.zeros(n))
                eng.logsv_rng(7, 0.01, p.theta, p.kappa1, p.kappa2, p.beta, p.volvol, 1.0, True, SEED, 0, off)
                out[f"slice7_off{off}_{n}_state"] = np.stack(eng.get_state())
        finally:
            eng.close()
    np.savez(out_path, **out)
    return 0


def run_child(tmp, tag, few_waves_max_paths):
    env = {k: v for k, v in os.environ.items() if k != "SVMC_FEW_WAVES_MAX_PATHS"}
    if few_waves_max_paths is not None:
        env["SVMC_FEW_WAVES_MAX_PATHS"] = few_waves_max_paths
    path = os.path.join(str(tmp), tag + ".npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, (tag, r.returncode, r.stderr[-2000:])      # a failed child: no further child is started
    with np.load(path) as g:
        return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pair_ahead")
    few = run_child(tmp, "few_waves", None)
    full = run_child(tmp, "full_launch", "0")
    return few, full


def expected_keys():
    keys = []
    for n in PATHS:
        for name in CHAINS:
            for kind in KINDS:
                for what in ("prices", "stderrs"):
                    keys.append(f"single_{name}_{kind}_{n}_{what}")
                    if name == "s341":
                        keys += [f"many{j}_{name}_{kind}_{n}_{what}" for j in range(2)]
        keys += [f"slice7_off{off}_{n}_state" for off in OFFSETS]
    return sorted(keys)


@pytest.mark.gpu
def test_full_launch_equals_few_waves_bit_for_bit(runs):
    few, full = runs
    assert sorted(few) == sorted(full) == expected_keys()
    # equal_nan: a one-path standard error has no sample variance behind it and may be NaN on both sides
    different = [k for k in few if not np.array_equal(few[k], full[k], equal_nan=True)]
    assert not different, different
    assert all(np.all(np.isfinite(a)) for k, a in full.items() if not k.endswith("_1_stderrs"))
    # job 0 of the many-job batch is the single chain on the same stream; job 1 has other parameters and another stream
    for n in PATHS:
        for kind in KINDS:
            for what in ("prices", "stderrs"):
                np.testing.assert_array_equal(full[f"many0_s341_{kind}_{n}_{what}"], full[f"single_s341_{kind}_{n}_{what}"])
            if n > 1:                                      # (a lone path can leave every option of both jobs worthless)
                assert not np.array_equal(full[f"many1_s341_{kind}_{n}_prices"], full[f"many0_s341_{kind}_{n}_prices"])
    # a slice from step 3 and one from step 4 see different words
    for n in PATHS:
        assert not np.array_equal(full[f"slice7_off3_{n}_state"], full[f"slice7_off4_{n}_state"])


@pytest.mark.gpu
def test_full_launch_matches_oracle_on_the_same_stream(runs):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import stochvolmodels_amd as sv
    from oracle import oracle
    from stochvolmodels_amd.utils.funcs import time_grid_steps

    _, full = runs
    name, n = ORACLE_CASE
    p = sv.LOGSV_BTC_PARAMS
    kw = chain_keywords(name, "LOG_RETURN")
    x, s, q = np.zeros(n), p.sigma0 * np.ones(n), np.zeros(n)
    t0, step0 = 0.0, 0
    for i, ttm in enumerate(kw["ttms"]):
        nb, dt = time_grid_steps(float(ttm - t0), SPY)
        x, s, q = oracle.logsv_terminal_rng(x, s, q, nb, dt, p.theta, p.kappa1, p.kappa2, p.beta, p.volvol, SEED, step_offset=step0)
        step0, t0 = step0 + nb, ttm
        pr, sd = oracle.payoff(x, q, float(ttm), float(kw["forwards"][i]), kw["strikes_ttms"][i], kw["optiontypes_ttms"][i],
                               float(kw["discfactors"][i]))
        np.testing.assert_allclose(full[f"single_{name}_LOG_RETURN_{n}_prices"][i], pr, **ST)
        np.testing.assert_allclose(full[f"single_{name}_LOG_RETURN_{n}_stderrs"][i], sd, **ST)
    assert step0 == 8


if __name__ == "__main__":
    sys.exit(child(sys.argv[1]))
