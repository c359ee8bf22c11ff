"""
logsv_vol_paths_kernel against the extended-precision recursion of tests/golden/vol_paths_steps.npz
(tests/golden/make_golden_vol_paths_steps.py: the reference's recursion in 256-bit mpmath on the product's own random stream).

svmc_logsv_vol_paths is driven through the C ABI on every case in both of its loop forms -- the increments uploaded as `brownians`
(the loop that prefetches groups of four) and the device draw at the case's seed (the loop that consumes the Philox stream call by
call) -- and the stored rows are compared with the truth as |d / truth - 1|, the largest over the paths.

The bound is relative to the fp64 oracle's own error, which the fixture stores per case and row:
gpu_err <= max(MARGIN x oracle_err, FLOOR_ULPS x 2^-52) with the margins tests/mc_steps_worker.py asserts for the LogSV generator
("logsv"; the far starts "far"), which steps in the same form (log units, rcp_1n, exp2u_tab).  tests/test_vol_paths_steps_host.py
shows that a step constant off by 1e-13 breaks it.  Each figure is printed before it is asserted (pytest -s);
profiles/vol_paths_step_observed_tolerances.txt keeps a run.

Also here: padded layouts (ld > n_path, ldb > n_path), the device draw at a path offset and at a call id.
"""
import numpy as np
import pytest

import mc_steps_worker as mw
import vol_paths_steps as vp

pytestmark = pytest.mark.gpu

BTC = dict(theta=1.0413, kappa1=3.1844, kappa2=3.058, beta=0.1514, volvol=1.8458)
V0, DT = 0.8376, 1.0 / 360.0


@pytest.fixture(scope="module")
def fx():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import _lib
    f = vp.Fixture()
    have = _lib.load().svmc_rng_stream_version()
    assert f.meta["rng_stream_version"] == have == sv.RNG_STREAM_VERSION, (
        f"tests/golden/vol_paths_steps.npz was made on random stream version {f.meta['rng_stream_version']}, the library draws "
        f"version {have}: regenerate it (python tests/golden/make_golden_vol_paths_steps.py)")
    return f


@pytest.mark.parametrize("form", ["w", "rng"])
@pytest.mark.parametrize("group", ["ordinary", "long", "far"])
def test_vol_paths_kernel_against_the_extended_precision_recursion(fx, group, form):
    cases = [c for c in fx.cases if c["group"] == group]
    assert cases
    bad = []
    for case in cases:
        w = vp.increments(case)
        assert mw.checksum(w) == case["checksum"], (case["id"], "regenerate tests/golden/vol_paths_steps.npz")
        err, oerr, lim = fx.error(case, vp.device_rows(case, form, w)), np.array(case["oracle_err"]), fx.bound(case)
        print(f"vol_paths_steps {case['id']} {form} rows " + " ".join(str(r) for r in case["rows"])
              + " oracle_err " + " ".join(f"{e:.2e}" for e in oerr) + " gpu_err " + " ".join(f"{e:.2e}" for e in err)
              + " ratio " + " ".join(f"{r:.2f}" for r in err / oerr) + " ulps " + " ".join(f"{e / mw.ULP:.2f}" for e in err)
              + f" worst gpu_err / bound {np.max(err / lim):.2f}")
        if not np.all(err <= lim):
            bad.append((case["id"], form, err.tolist(), lim.tolist()))
    assert not bad, f"{len(bad)} of {len(cases)} cases past max(MARGIN x oracle_err, FLOOR_ULPS ulp) (mc_steps_worker.py): {bad[:4]}"


@pytest.mark.parametrize("steps", [7, 9])
@pytest.mark.parametrize("spot", [True, False])
def test_padded_layouts(fx, steps, spot):
    """ld = n_path + 3 and ldb = n_path + 5: the rows are the compact run's bit for bit, and the output's padding keeps the sentinel
    it was prefilled with (so does the compact run's array: row 0 is v0, nothing else is left over)"""
    n = 130
    w = np.sqrt(DT) * np.random.default_rng(steps).standard_normal((steps, n))
    compact = vp.device_vol_paths(n, steps, DT, V0, BTC, spot, w=w)
    assert compact.shape == (steps + 1, n) and np.all(compact[0] == V0) and np.all(compact > 0.0)
    for ld, ldb in ((n + 3, n), (n, n + 5), (n + 3, n + 5)):
        got = vp.device_vol_paths(n, steps, DT, V0, BTC, spot, w=w, ld=ld, ldb=ldb)
        np.testing.assert_array_equal(got[:, :n], compact)
        assert np.all(got[:, n:] == vp.SENTINEL)
    drawn = vp.device_vol_paths(n, steps, DT, V0, BTC, spot, seed=11)
    got = vp.device_vol_paths(n, steps, DT, V0, BTC, spot, seed=11, ld=n + 3)
    np.testing.assert_array_equal(got[:, :n], drawn)
    assert np.all(got[:, n:] == vp.SENTINEL) and not np.array_equal(drawn, compact)


@pytest.mark.parametrize("steps", [7, 9])
def test_device_draw_with_a_path_offset(fx, steps):
    """paths 77 .. 206 of a 207-path run at offset 0 are the 130 paths of a run at path_offset 77, bit for bit"""
    whole = vp.device_vol_paths(207, steps, DT, V0, BTC, True, seed=13)
    part = vp.device_vol_paths(130, steps, DT, V0, BTC, True, seed=13, path_offset=77)
    np.testing.assert_array_equal(part, whole[:, 77:207])
    assert len(np.unique(whole[-1])) == 207                   # every path drew for itself


def test_device_draw_with_a_call_id(fx):
    a = vp.device_vol_paths(130, 7, DT, V0, BTC, True, seed=13, call_id=0)
    b = vp.device_vol_paths(130, 7, DT, V0, BTC, True, seed=13, call_id=5)
    again = vp.device_vol_paths(130, 7, DT, V0, BTC, True, seed=13, call_id=5)
    np.testing.assert_array_equal(b, again)
    assert np.all(a[0] == b[0]) and np.all(a[1:] != b[1:])
