"""
The multi-set LogSV stepping kernels against the extended-precision recursion of tests/golden/chain_sets_steps.npz
(tests/golden/make_golden_chain_sets_steps.py: make_golden_mc_steps.py's 256-bit LogSV recursion on the product's stream).

After a sets launch x and qvar of every (set, expiry) lie in the session's snapshot rows, set-major.  They are read back
(chain_sets_steps.session_rows, through the engine's download) and compared with the truth in the measure and under the bound of
tests/test_gpu_mc_steps.py: gpu_err <= mc_steps_worker.bound(oracle_err, "logsv"), oracle_err the fp64 oracle's own error, stored
per (measure, set, slice).  No number is new: the margin is the single-set LogSV generator's.

Widths 4 (the three-piece loop without parking), 7 (the two-piece loop with parking) and 8 (on the frozen route the launch with
s0 = 4), both measures, a chain of slices of 1, 2, 5 and 40 steps on 130 paths, the odd sets with a backbone eta off 1.  The frozen
route (logsv_chain_rng_sets_kernel) draws the stream (seed, call 0) in registers; the resident route (logsv_chain_w_sets_kernel) gets
the same normals uploaded as W0 / W1: one truth serves both families.  Each figure is printed before it is asserted (pytest -s);
profiles/chain_sets_observed_tolerances.txt keeps a run.
"""
import numpy as np
import pytest

import chain_sets_steps as cs
import mc_steps_worker as mw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import _lib
    f = cs.Fixture()
    have = _lib.load().svmc_rng_stream_version()
    assert f.meta["rng_stream_version"] == have == sv.RNG_STREAM_VERSION, (
        f"tests/golden/chain_sets_steps.npz was made on random stream version {f.meta['rng_stream_version']}, the library draws "
        f"version {have}: regenerate it (python tests/golden/make_golden_chain_sets_steps.py)")
    return f


@pytest.fixture(scope="module")
def randoms(fx):
    """the frozen stream and the same normals resident; freed at the end"""
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.utils.funcs import time_grid_steps
    t0, steps = 0.0, []
    for t in fx.ttms:                                        # slices of 1, 2, 5 and 40 steps of 2^-9 each
        nb, dt = time_grid_steps(t - t0, fx.spy)
        assert dt == fx.dt == 2.0 ** -9
        steps.append(nb)
        t0 = t
    assert steps == fx.steps == [1, 2, 5, 40]
    W0, W1, checksum = fx.normals()
    assert checksum == fx.meta["checksum"], "the random inputs moved: regenerate tests/golden/chain_sets_steps.npz"
    cuts = np.cumsum([0] + steps)
    W0s, W1s = ([W[a:b] for a, b in zip(cuts, cuts[1:])] for W in (W0, W1))
    out = dict(frozen=sv.draw_fixed_randoms_on_device(np.array(fx.ttms), nb_path=fx.n, nb_steps_per_year=fx.spy, seed=fx.seed),
               resident=sv.upload_fixed_randoms(W0s, W1s, [fx.dt] * len(steps)))
    assert out["frozen"].nb_steps == steps and out["frozen"].dts == [fx.dt] * len(steps)
    yield out
    for r in out.values():
        r.free()


def device_rows(fx, res, width, spot):
    """[width][m][2][n]: x and qvar of the sets 0 .. width - 1 after each slice, from ONE sets call"""
    import pandas as pd
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.engine import get_engine
    ttms = np.array(fx.ttms)
    m = ttms.size
    plist = [sv.LogSvParams(**{k: p[k] for k in cs.PARAM_NAMES},
                            vol_backbone=None if p["eta"] == 1.0 else pd.Series(np.full(m, p["eta"]), index=ttms))
             for p in fx.sets[:width]]
    for p, q in zip(plist, fx.sets):
        assert np.array_equal(p.get_vol_backbone_etas(ttms=ttms), np.full(m, q["eta"]))
    strikes = (np.array([0.5, 1.0, 1.5]),) * m                               # realised-variance quotes: the launch writes qvar rows too
    out = sv.logsv_mc_chain_pricer_fixed_randoms_batch(
        params_list=plist, W0s=res, is_spot_measure=spot, variable_type=sv.VariableType.Q_VAR, ttms=ttms, forwards=np.ones(m),
        discfactors=np.ones(m), strikes_ttms=tuple(s * t for s, t in zip(strikes, ttms)), optiontypes_ttms=(np.array(["C", "P", "C"]),) * m)
    assert len(out) == width
    x, q = cs.session_rows(get_engine(fx.n), res._session_sets, fx.n, *res._session_sets_size, width, m, True)
    return np.stack([x, q], axis=2)


@pytest.mark.parametrize("route", ("frozen", "resident"))
@pytest.mark.parametrize("spot", (True, False), ids=("spot", "inv"))
@pytest.mark.parametrize("width", cs.WIDTHS)
def test_sets_kernels_against_the_extended_precision_recursion(fx, randoms, width, spot, route):
    assert width in fx.meta["widths"]
    rows = device_rows(fx, randoms[route], width, spot)
    err, oerr = fx.errors(spot, rows)
    lim = mw.bound(oerr, "logsv")
    bad = []
    for q in range(width):
        for i in range(len(fx.steps)):
            with np.errstate(all="ignore"):
                ratio = err[q, i] / oerr[q, i]
            print(f"chain_sets {route} P={width} {cs.case_id(spot, q, i)} oracle_err " + " ".join(f"{e:.2e}" for e in oerr[q, i])
                  + " gpu_err " + " ".join(f"{e:.2e}" for e in err[q, i]) + " ratio " + " ".join(f"{r:.2f}" for r in ratio)
                  + " ulps " + " ".join(f"{e / mw.ULP:.2f}" for e in err[q, i]))
            if not np.all(err[q, i] <= lim[q, i]):
                bad.append((cs.case_id(spot, q, i), err[q, i].tolist(), lim[q, i].tolist()))
    assert not bad, f"{len(bad)} of {width * len(fx.steps)} rows past max(MARGIN x oracle_err, FLOOR_ULPS ulp) (mc_steps_worker.py): {bad[:6]}"
