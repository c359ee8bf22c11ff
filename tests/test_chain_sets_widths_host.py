"""
What tests/test_gpu_chain_sets_widths.py and tests/test_gpu_chain_sets_steps.py rest on, checked without a device:

  * width coverage: every instantiation of logsv_chain_w_sets_kernel<P> and logsv_chain_rng_sets_kernel<P> that
    tests/golden/libsvmc_kernel_names.json lists is launched by the width grid of tests/test_gpu_chain_sets_widths.py (through the
    dispatch: one set on resident randoms goes to the single-set kernel, eight frozen sets run as two launches of <4>), and the
    widths held to the recursion are among them -- an instantiation added without a test fails here;
  * tests/golden/chain_sets_steps.npz: its random inputs are the generator's (checksum), the fp64 oracle on them reproduces the
    errors the fixture stores and is inside the device bound, and no more paths are flagged fragile than in the LogSV cases of
    tests/golden/mc_steps.npz (none: the recursion takes no discrete decision);
  * sensitivity, per set: ONE step constant of ONE set off so that its rows move by 1e-13 is past the device bound on that set's
    rows and leaves every other set's rows where they were.
"""
import json
import os
import re

import numpy as np
import pytest

import chain_sets_steps as cs
import mc_steps_worker as mw
import test_gpu_chain_sets_widths as widths
from test_mc_steps_host import MOVE, MUTATED, reproduced

FAMILIES = ("logsv_chain_w_sets_kernel", "logsv_chain_rng_sets_kernel")


@pytest.fixture(scope="module")
def fx():
    return cs.Fixture()


def instantiations():
    """{family: set of P} from the library's kernel names"""
    names = json.load(open(os.path.join(mw.HERE, "golden", "libsvmc_kernel_names.json")))
    names = names["kernels"] if isinstance(names, dict) else names
    out = {f: set() for f in FAMILIES}
    for name in names:
        hit = re.match(r"_ZN4svmc\d+(logsv_chain_(?:w|rng)_sets_kernel)ILi(\d+)EEE", name)
        if hit:
            out[hit.group(1)].add(int(hit.group(2)))
    return out


def test_the_width_grid_launches_every_instantiation():
    have = instantiations()
    assert have["logsv_chain_w_sets_kernel"] and have["logsv_chain_rng_sets_kernel"]
    launched = {f: set() for f in FAMILIES}
    for route, width, n in widths.WIDTH_GRID:
        assert route in widths.ROUTES and n >= 1
        for family, p in widths.launches_of(route, width):
            if family in launched:
                launched[family].add(p)
    assert launched == have, (launched, have)
    # every instantiation also meets the path counts around a wave and a block
    for family, route in zip(FAMILIES, widths.ROUTES):
        for p in have[family]:
            ns = {n for r, w, n in widths.WIDTH_GRID if r == route and (family, p) in widths.launches_of(r, w)}
            assert set(widths.BASE_PATHS) <= ns, (family, p)
    for w in widths.EDGE_WIDTHS:
        for route in widths.ROUTES:
            assert {n for r, ww, n in widths.WIDTH_GRID if r == route and ww == w} == set(widths.EDGE_PATHS)


def test_the_dispatch_the_grid_assumes():
    assert widths.launches_of("resident", 1) == [("logsv_chain_w_indirect_kernel", 1)]
    assert widths.launches_of("resident", 9) == [("logsv_chain_w_sets_kernel", 8), ("logsv_chain_w_indirect_kernel", 1)]
    assert widths.launches_of("frozen", 8) == [("logsv_chain_rng_sets_kernel", 4)] * 2
    assert widths.launches_of("frozen", 15) == [("logsv_chain_rng_sets_kernel", 4)] * 2 + [("logsv_chain_rng_sets_kernel", 7)]
    assert widths.launches_of("frozen", 1) == [("logsv_chain_rng_sets_kernel", 1)]
    src = open(os.path.join(mw.ROOT, "stochvolmodels_amd", "csrc", "svmc_internal.h")).read()
    assert int(re.search(r"constexpr int MAX_FUSED_SETS = (\d+);", src).group(1)) == widths.MAX_SETS_PER_LAUNCH
    assert int(re.search(r"constexpr int MAX_FUSED_SLICES = (\d+);", src).group(1)) == widths.MAX_CHAIN_SLICES


def test_the_recursion_widths_are_instantiations(fx):
    have = instantiations()
    assert tuple(fx.meta["widths"]) == cs.WIDTHS == (4, 7, 8)
    for w in cs.WIDTHS:
        assert ("logsv_chain_w_sets_kernel", w) in widths.launches_of("resident", w) and w in have["logsv_chain_w_sets_kernel"]
        assert all(p in have["logsv_chain_rng_sets_kernel"] for _, p in widths.launches_of("frozen", w))
    assert len(fx.sets) == max(cs.WIDTHS) and fx.n == 130 and fx.steps == [1, 2, 5, 40]
    for name in cs.PARAM_NAMES:                             # set q differs from every other in every model parameter
        assert len({p[name] for p in fx.sets}) == len(fx.sets), name
    assert [p["eta"] != 1.0 for p in fx.sets] == [q % 2 == 1 for q in range(len(fx.sets))]
    for spot in (True, False):
        for q in range(len(fx.sets)):
            for i, steps in enumerate(np.cumsum(fx.steps)):
                c = fx.by_id[cs.case_id(spot, q, i)]
                assert (c["set"], c["slice"], c["spot"], c["steps"], c["n"], c["nq"]) == (q, i, spot, steps, fx.n, 2)
                assert c["scales"] == [1.0, fx.sets[q]["theta"] ** 2 * steps * fx.dt]


def test_stream_version_is_recorded(fx):
    header = open(os.path.join(mw.ROOT, "include", "svmc.h")).read()
    assert fx.meta["rng_stream_version"] == int(re.search(r"#define SVMC_RNG_STREAM_VERSION (\d+)", header).group(1)), \
        "regenerate tests/golden/chain_sets_steps.npz"


def test_the_grid_is_the_drivers(fx):
    from stochvolmodels_amd.utils.funcs import chain_step_grid
    nbs, dts = chain_step_grid(fx.ttms, fx.spy)
    assert nbs == fx.steps and dts == [fx.dt] * len(fx.steps) and fx.dt == 2.0 ** -9


@pytest.mark.parametrize("spot", (True, False), ids=("spot", "inv"))
def test_inputs_are_the_fixture_s_and_the_oracle_is_inside_the_bound(fx, oracle, spot):
    W0, W1, checksum = fx.normals()
    assert checksum == fx.meta["checksum"], "the random inputs moved: regenerate tests/golden/chain_sets_steps.npz"
    for restatement, key in ((False, "oracle_err"), (True, "numpy_err")):
        rows = cs.oracle_rows(fx, W0, W1, spot, range(len(fx.sets)), restatement=restatement)
        err, oerr = fx.errors(spot, rows)
        stored = np.array([[fx.by_id[cs.case_id(spot, q, i)][key] for i in range(len(fx.steps))] for q in range(len(fx.sets))])
        assert reproduced(err, stored), (key, err.tolist(), stored.tolist())
        if not restatement:
            assert np.all(np.isfinite(oerr)) and np.all(err <= mw.bound(oerr, "logsv"))


def test_fragile_share(fx):
    """a cap, read from the LogSV cases of mc_steps.npz: the same recursion flags no larger a share here"""
    ref = mw.Fixture()
    cap = max(float(ref.truth(c)[2].mean()) for c in ref.cases if c["gen"] == "logsv")
    for case in fx.cases:
        fragile = fx.truth(case)[2]
        assert int(fragile.sum()) == case["fragile_paths"]
        assert fragile.mean() <= cap, case["id"]


@pytest.mark.parametrize("spot", (True, False), ids=("spot", "inv"))
def test_a_step_constant_of_one_set_off_by_1e_13_breaks_that_set_s_rows_only(fx, oracle, spot):
    """the sensitivity check of tests/test_mc_steps_host.py per set, at the widest case: the seven constants of the step, each
    on another set in turn"""
    W0, W1, _ = fx.normals()
    sets = range(len(fx.sets))
    base = cs.oracle_rows(fx, W0, W1, spot, sets, restatement=True)
    err, oerr = fx.errors(spot, base)
    lim = mw.bound(oerr, "logsv")
    assert np.all(err <= lim)                                 # the unmutated restatement is inside the bound
    last = len(fx.steps) - 1                                  # the 48-step rows
    scale = np.array([np.maximum(np.abs(fx.truth(fx.by_id[cs.case_id(spot, q, last)])[0]),
                                 np.asarray(fx.by_id[cs.case_id(spot, q, last)]["scales"])[:, None]) for q in sets])

    def move(rows, q):
        return float(np.max(np.abs(rows[q, last] - base[q, last]) / scale[q]))

    for k, name in enumerate(MUTATED["logsv"]):
        q = k % len(fx.sets)
        probe = 1e-9
        m0 = move(cs.oracle_rows(fx, W0, W1, spot, sets, restatement=True, scaled=(q, name, 1.0 + probe)), q)
        assert m0 > 0.0, name
        mutated = cs.oracle_rows(fx, W0, W1, spot, sets, restatement=True, scaled=(q, name, 1.0 + probe * MOVE / m0))
        assert 0.5 * MOVE <= move(mutated, q) <= 2.0 * MOVE, (name, move(mutated, q))
        merr, _ = fx.errors(spot, mutated)
        assert np.any(merr[q] > lim[q]), (name, q, merr[q].tolist(), lim[q].tolist())
        others = [s for s in sets if s != q]
        assert np.array_equal(mutated[others], base[others]) and np.all(merr[others] <= lim[others]), (name, q)
