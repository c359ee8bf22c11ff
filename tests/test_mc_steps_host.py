"""
tests/golden/mc_steps.npz (make_golden_mc_steps.py: the Monte Carlo step recursions in 256-bit mpmath) and the bound that
tests/test_gpu_mc_steps.py asserts against it, checked without a device:

  * the fp64 oracles -- oracle/svmc_oracle.c, the NumPy restatements np_logsv_terminal_w / np_heston_terminal_w and
    hawkes_twin.simulate_terminal -- on the fixture's recorded inputs reproduce the errors the fixture stores for them (the
    yardstick of the device test), and the inputs are the ones the truth was computed on (checksums);
  * mutation: ONE step constant of a restatement scaled so that the terminal state moves by 1e-13 -- a tenth of what the parity
    tests against the oracle allow -- is past the device test's bound on the 64-step case, for every constant of the step;
  * at most 1 % of the paths of any case are fragile.
"""
import numpy as np
import pytest

import mc_steps_worker as mw

MOVE = 1e-13
# a stored error is reproduced when the recomputed one is within a factor two of it, give or take two ulp: the C library's exp and
# log may round differently from the one the fixture was made with (<= 1 ulp per call)
REPRO_FACTOR, REPRO_ULPS = 2.0, 2.0
MUTATED = {"logsv": ("theta", "kappa1", "kappa2", "beta", "volvol", "eta", "dt"),
           "heston": ("theta", "kappa", "rho", "volvol", "dt"),
           "hawkes": ("sigma", "shift_p", "mean_p", "shift_m", "mean_m", "theta_p", "kappa_p", "beta1_p", "beta2_p", "theta_m", "kappa_m",
                      "beta1_m", "beta2_m", "dt")}
MUTATION_CASES = {"logsv": "logsv-btc-spot-eta1-s64-o0", "heston": "heston-base-s64-o0", "hawkes": "hawkes-hawkes_mc-s64-o0"}


@pytest.fixture(scope="module")
def fx():
    return mw.Fixture()


def reproduced(got, stored):
    got, stored = np.asarray(got), np.asarray(stored)
    slack = REPRO_ULPS * mw.ULP
    return bool(np.all(got <= REPRO_FACTOR * stored + slack) and np.all(got >= stored / REPRO_FACTOR - slack))


@pytest.mark.parametrize("gen", ["logsv", "far", "heston", "qe", "rough", "hawkes"])
def test_oracles_reproduce_the_stored_errors(fx, oracle, gen):
    cases = [c for c in fx.cases if c["gen"] == gen]
    assert cases
    for case in cases:
        arrs, cs = mw.inputs(fx, case)
        assert cs == case["checksum"], (case["id"], "the random inputs moved: regenerate tests/golden/mc_steps.npz")
        restated = gen == "hawkes"                           # the twin IS the Hawkes oracle
        err = fx.error(case, mw.oracle_state(fx, case, arrs, restatement=restated))
        assert reproduced(err, case["oracle_err"]), (case["id"], err, case["oracle_err"])
        if "numpy_err" in case:
            err = fx.error(case, mw.oracle_state(fx, case, arrs, restatement=True))
            assert reproduced(err, case["numpy_err"]), (case["id"], err, case["numpy_err"])
        assert np.all(np.isfinite(case["oracle_err"]))


def test_stream_version_is_recorded(fx):
    import re
    header = open(mw.os.path.join(mw.ROOT, "include", "svmc.h")).read()
    assert fx.meta["rng_stream_version"] == int(re.search(r"#define SVMC_RNG_STREAM_VERSION (\d+)", header).group(1)), \
        "regenerate tests/golden/mc_steps.npz"


@pytest.mark.parametrize("gen", sorted(MUTATED))
def test_a_step_constant_off_by_1e_13_breaks_the_device_bound(fx, oracle, gen):
    case = fx.by_id[MUTATION_CASES[gen]]
    assert case["steps"] == 64
    arrs, _ = mw.inputs(fx, case)
    hi, _, fragile = fx.truth(case)
    scale = np.maximum(np.abs(hi), np.asarray(case["scales"])[:, None])[:, ~fragile]
    base = mw.oracle_state(fx, case, arrs, restatement=True)
    lim = mw.bound(case["oracle_err"], gen)
    assert np.all(np.array(fx.error(case, base)) <= lim)      # the unmutated restatement is inside the bound

    def move(state):
        return float(np.max(np.abs(state - base)[:, ~fragile] / scale))

    for name in MUTATED[gen]:
        probe = 1e-9
        m0 = move(mw.oracle_state(fx, case, arrs, restatement=True, scaled=(name, 1.0 + probe)))
        assert m0 > 0.0, name
        mutated = mw.oracle_state(fx, case, arrs, restatement=True, scaled=(name, 1.0 + probe * MOVE / m0))
        assert 0.5 * MOVE <= move(mutated) <= 2.0 * MOVE, (name, move(mutated))
        err = np.array(fx.error(case, mutated))
        assert np.any(err > lim), (name, err.tolist(), lim.tolist())


def test_fragile_share(fx):
    for case in fx.cases:
        fragile = fx.truth(case)[2]
        assert int(fragile.sum()) == case["fragile_paths"]
        assert fragile.mean() <= fx.meta["max_fragile_share"] == 0.01, case["id"]


def test_every_case_of_the_table_is_there(fx):
    """generator x parameter set x step count x step_offset, as the fixture's generator lists them"""
    ids = set(fx.by_id)
    for s in ("btc", "test"):
        for m in ("spot", "inv"):
            for eta in ("1", "0.7"):
                for st in (1, 2, 3, 7, 64):
                    for off in (0, 1):
                        assert f"logsv-{s}-{m}-eta{eta}-s{st}-o{off}" in ids
    for st in (1, 2, 3, 7, 64):
        for off in (0, 1):
            assert all(f"heston-{s}-s{st}-o{off}" in ids for s in ("base", "btc"))
            assert all(f"qe-{s}-s{st}-o{off}" in ids for s in ("general", "quad", "quad_tiny_volvol"))
    assert {"logsv-btc-spot-eta1-s1024-o0", "heston-btc-s1024-o0", "qe-general-s1024-o0"} <= ids
    for st in (1, 2, 5, 40):
        for off in (0, 1):
            assert all(f"rough-{h}-s{st}-o{off}" in ids for h in ("h010", "h045", "h050"))
    assert sorted(len(fx.by_id[f"rough-{h}-s1-o0"]["nodes"]) for h in ("h010", "h045", "h050")) == [1, 2, 3]
    for st in (1, 2, 3, 7, 64, 451):
        for off in (0, 1):
            for s in ("hawkes_mc", "hawkes_mc_excited"):
                assert min(fx.by_id[f"hawkes-{s}-s{st}-o{off}"]["jumped"]) >= 0.05
    for r in ("explosive", "collapse"):
        assert all(f"far-{r}-s{st}-o{off}" in ids for st in (1, 2) for off in (0, 1))
        assert fx.far_start[r].shape == (3, 130)
    assert all(c["n"] == (64 if c["steps"] == 1024 else 130) for c in fx.cases)
