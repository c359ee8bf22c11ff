"""
The Monte Carlo step kernels against the extended-precision recursion of tests/golden/mc_steps.npz
(tests/golden/make_golden_mc_steps.py: the reference's recursion in 256-bit mpmath on the product's own random stream).

Every generator is driven through the engine in each of its forms -- randoms supplied (logsv_w, heston_w, heston_qe_w, rough_logsv
with Z), drawn on the device in the few-waves form (logsv_rng, heston_rng Euler and QE, rough_logsv, hawkesjd_rng at 130 and 64
paths) and, in a child process with SVMC_FEW_WAVES_MAX_PATHS=0 (tests/mc_steps_worker.py), drawn on the device by the full-launch
kernels -- and the terminal x, volatility-like state and qvar are compared with the truth on the paths the fixture does not flag
fragile, in the measure |d - truth| / max(|truth|, scale) (scale: 1 for x, sigma0 / theta for the state, theta^2 T for qvar; the
fixture records each case's).

The bound is relative to the fp64 oracle's own error, which the fixture stores per case and quantity:
gpu_err <= max(MARGIN x oracle_err, FLOOR_ULPS x 2^-52), per generator (mc_steps_worker.bound).  A correct step in another grouping rounds like
the oracle does; a construct that loses bits does not.  tests/test_mc_steps_host.py shows that a step constant off by 1e-13 breaks
this bound.  Each figure is printed before it is asserted (pytest -s); profiles/mc_step_observed_tolerances.txt keeps a run.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import mc_steps_worker as mw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import _lib
    f = mw.Fixture()
    have = _lib.load().svmc_rng_stream_version()
    assert f.meta["rng_stream_version"] == have == sv.RNG_STREAM_VERSION, (
        f"tests/golden/mc_steps.npz was made on random stream version {f.meta['rng_stream_version']}, the library draws version "
        f"{have}: regenerate it (python tests/golden/make_golden_mc_steps.py)")
    return f


def check(fx, states, form):
    """print the figures of every (case, form) in `states`, then assert the bound on all of them"""
    bad = []
    for (cid, _), st in states.items():
        case = fx.by_id[cid]
        err, oerr = np.array(fx.error(case, st)), np.array(case["oracle_err"])
        lim = mw.bound(oerr, case["gen"])
        with np.errstate(all="ignore"):
            ratio = err / oerr
        print(f"mc_steps {cid} {form} oracle_err " + " ".join(f"{e:.2e}" for e in oerr) + " gpu_err " + " ".join(f"{e:.2e}" for e in err)
              + " ratio " + " ".join(f"{r:.2f}" for r in ratio) + " ulps " + " ".join(f"{e / mw.ULP:.2f}" for e in err))
        if not np.all(err <= lim):
            bad.append((cid, form, err.tolist(), lim.tolist()))
    assert not bad, f"{len(bad)} of {len(states)} cases past max(MARGIN x oracle_err, FLOOR_ULPS ulp) (mc_steps_worker.py): {bad[:6]}"


@pytest.mark.parametrize("gen", ["logsv", "far", "heston", "qe", "rough", "hawkes"])
def test_inputs_are_the_fixture_s(fx, gen):
    """the oracle and the twin still produce the random inputs the truth was computed on"""
    for case in fx.cases:
        if case["gen"] == gen:
            assert mw.inputs(fx, case)[1] == case["checksum"], (case["id"], "regenerate tests/golden/mc_steps.npz")


@pytest.mark.parametrize("gen,form", [(g, f) for g, forms in mw.FORMS.items() for f in forms])
def test_step_kernels_against_the_extended_precision_recursion(fx, gen, form):
    cases = [c for c in fx.cases if c["gen"] == gen]
    assert cases
    check(fx, mw.run_forms(fx, [(c, form) for c in cases]), form)


def test_full_launch_forms(fx, tmp_path):
    """the device-draw cases of LogSV (far states included), Heston Euler and Heston QE on the FULL-LAUNCH kernels"""
    out = str(tmp_path / "full_launch.npz")
    r = subprocess.run([sys.executable, os.path.join(mw.HERE, "mc_steps_worker.py"), out],
                       env=dict(os.environ, SVMC_FEW_WAVES_MAX_PATHS="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    g = np.load(out)
    want = [c["id"] for c in fx.cases if c["gen"] in mw.FULL_LAUNCH_GENS]
    assert sorted(g.files) == sorted(want)
    check(fx, {(cid, "rng"): g[cid] for cid in want}, "rng_full")
