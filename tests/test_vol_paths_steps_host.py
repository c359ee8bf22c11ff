"""
tests/golden/vol_paths_steps.npz (make_golden_vol_paths_steps.py: the volatility-path recursion in 256-bit mpmath) and the bound
that tests/test_gpu_vol_paths_steps.py asserts against it, checked without a device:

  * the fp64 oracle (oracle/svmc_oracle.c:svo_logsv_vol_paths) on the fixture's increments reproduces the errors the fixture stores
    for it (the yardstick of the device test), and the increments are the ones the truth was computed on (checksums);
  * every case of the table is there;
  * mutation: ONE step constant of the oracle scaled so that the last row of a 64-step case moves by 1e-13 relative is past the
    device test's bound on that row, for every constant of the step.
"""
import re

import numpy as np
import pytest

import mc_steps_worker as mw
import vol_paths_steps as vp
from test_mc_steps_host import MOVE, reproduced

MUTATION_CASE = "vp-btc-spot-s64"


@pytest.fixture(scope="module")
def fx():
    return vp.Fixture()


def test_oracle_reproduces_the_stored_errors(fx, oracle):
    for case in fx.cases:
        w = vp.increments(case)
        assert mw.checksum(w) == case["checksum"], (case["id"], "the increments moved: regenerate tests/golden/vol_paths_steps.npz")
        err = fx.error(case, vp.oracle_rows(case, w))
        assert np.all(np.isfinite(case["oracle_err"]))
        assert reproduced(err, case["oracle_err"]), (case["id"], err.tolist(), case["oracle_err"])


def test_stream_version_is_recorded(fx):
    header = open(mw.os.path.join(mw.ROOT, "include", "svmc.h")).read()
    assert fx.meta["rng_stream_version"] == int(re.search(r"#define SVMC_RNG_STREAM_VERSION (\d+)", header).group(1)), \
        "regenerate tests/golden/vol_paths_steps.npz"


def test_every_case_of_the_table_is_there(fx):
    ordinary, far = vp.expected_ids()
    assert set(ordinary) <= set(fx.by_id)
    assert all(set(ids) <= set(fx.by_id) for ids in far.values())         # no far start was dropped: every truth is finite
    for case in fx.cases:
        s = case["steps"]
        assert case["dt"] == 1.0 / 360.0
        assert case["n"] == (64 if s == vp.LONG_STEPS else 130)
        assert case["rows"] == list({64: vp.ROWS_64, vp.LONG_STEPS: vp.ROWS_LONG}.get(s, range(1, s + 1)))
        hi, lo = fx.truth(case)
        assert hi.shape == (len(case["rows"]), case["n"]) and np.all(np.isfinite(hi)) and np.all(hi > 0.0)
        assert np.all(np.abs(lo) <= 2.0 ** -53 * hi * (1.0 + 2.0 ** -20))
    p = fx.by_id["vp-far-div50-s1"]["params"]
    assert [fx.by_id[f"vp-far-{t}-s7"]["v0"] for t in vp.FAR_STARTS] == [p["theta"] * f for f in vp.FAR_STARTS.values()]
    assert not fx.by_id["vp-btc-inv-s64"]["spot"] and fx.by_id["vp-btc-spot-s64"]["spot"] and fx.by_id["vp-test-spot-s64"]["spot"]


@pytest.mark.parametrize("name", vp.STEP_CONSTANTS)
def test_a_step_constant_off_by_1e_13_breaks_the_device_bound(fx, oracle, name):
    case = fx.by_id[MUTATION_CASE]
    assert case["steps"] == 64 and case["rows"][-1] == 64
    w = vp.increments(case)
    hi, _ = fx.truth(case)
    base = vp.oracle_rows(case, w)
    lim = fx.bound(case)
    assert np.all(fx.error(case, base) <= lim)               # the unmutated oracle is inside the bound

    def move(rows):
        return float(np.max(np.abs(rows[-1] - base[-1]) / hi[-1]))

    probe = 1e-9
    m0 = move(vp.oracle_rows(case, w, scaled=(name, 1.0 + probe)))
    assert m0 > 0.0
    mutated = vp.oracle_rows(case, w, scaled=(name, 1.0 + probe * MOVE / m0))
    assert 0.5 * MOVE <= move(mutated) <= 2.0 * MOVE, move(mutated)
    err = fx.error(case, mutated)
    print(f"vol_paths_steps mutation {name}: last row err {err[-1]:.2e} bound {lim[-1]:.2e}")
    assert err[-1] > lim[-1], (name, err.tolist(), lim.tolist())
