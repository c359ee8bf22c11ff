"""
The host side of the four weighted conditional tails -- svmc_tilted_cond_payoff_chain, svmc_tilted_cond_greeks_chain,
svmc_cond_density_chain, svmc_jump_sets_payoff_chain -- replayed against tests/golden/cond_tails_host.json
(make_golden_cond_tails.py, recorded on the commit before the tails got one table walk, one quote check and one host driver in
csrc/svmc_tilted_cond.h): the four workspace size functions equal on the grid, and every call with one fault answered with the
recorded status.  No GPU: every call carries a workspace too small for it and is refused before anything is launched.
"""
import importlib.util
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_cond_tails", os.path.join(GOLDEN, "make_golden_cond_tails.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def _libraries():
    from stochvolmodels_amd import _lib
    return _lib.load_ext(), _lib.load_est()


def test_the_fixture_holds_every_size_and_every_case():
    gen = _generator()
    rec = json.load(open(gen.HOST_FIXTURE))
    sizes = np.array(rec["sizes"], dtype=np.uint64)
    assert sizes.shape == (4, 4, 4, 4) and (sizes > 0).all() and (sizes % 8 == 0).all()
    assert gen.SIZE_N == (1, 256, 257, 300000) and gen.SIZE_MK == ((1, 0), (1, 1), (3, 17), (16, 208)) and gen.SIZE_Z == (1, 4, 5, 16)
    want = [[entry, name] for entry in gen.SIGNATURES for name, _ in gen.defects(entry)]
    assert [r[:2] for r in rec["refusals"]] == want and len(gen.SIGNATURES) == 4
    by_entry = {entry: {n: s for e, n, s in rec["refusals"] if e == entry} for entry in gen.SIGNATURES}
    for entry, cases in by_entry.items():
        # each null pointer, each size, the offsets, a null row, the values, the workspace; the one status that is not "invalid argument"
        # but for the workspace's is the unknown type's, where the entry has types
        assert {"null_mu", "null_offsets", "null_gammas", "null_workspace", "null_row_mu", "n_path_0", "n_expiries_0", "n_z_0", "n_z_17",
                "offsets_start_1", "decreasing_offsets", "offset_above_2^30", "too_many_groups", "gamma_nan"} <= set(cases), entry
        assert cases["workspace_one_byte_short"] == gen.ERR_WORKSPACE
        other = {n: s for n, s in cases.items() if s not in (1, gen.ERR_WORKSPACE)}
        assert other == ({"type_2": 3, "type_-1": 3} if "types" in gen.SIGNATURES[entry] else {}), (entry, other)
    assert {"forward_0", "forward_inf", "forward_nan", "strike_nan", "shift_nan"} <= set(by_entry["svmc_tilted_cond_payoff_chain"])
    assert {"variance_negative", "variance_nan", "shift_nan"} <= set(by_entry["svmc_jump_sets_payoff_chain"])
    assert {"point_nan", "null_row_cv", "too_many_expiries"} <= set(by_entry["svmc_cond_density_chain"])


def test_the_sizes_replay():
    gen = _generator()
    rec = json.load(open(gen.HOST_FIXTURE))
    got, want = np.array(gen.run_sizes(*_libraries()), dtype=np.uint64), np.array(rec["sizes"], dtype=np.uint64)
    assert (got == want).all(), np.argwhere(got != want)[:6]


def test_every_single_fault_is_refused_with_the_recorded_status():
    gen = _generator()
    rec = json.load(open(gen.HOST_FIXTURE))
    now = gen.run_refusals(*_libraries())
    assert len(now) == len(rec["refusals"])
    differ = [(a, b) for a, b in zip(now, rec["refusals"]) if a != b]
    assert not differ, f"{len(differ)} of {len(now)} cases differ; the first (now, recorded): {differ[:5]}"
