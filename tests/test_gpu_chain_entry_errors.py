"""
The eight on-device-RNG chain entry points of svmc_chain.hip answer every bad argument -- alone, and two at once -- with the
status code and the svmc_last_error text recorded in tests/golden/chain_entry_errors.json (make_golden_chain_entry_errors.py, on
the commit before the entry points got their shared host helpers): the checks, their texts and their ORDER are part of the C ABI.
Every case fails before anything is launched: the test creates two small sessions and runs no kernel.
"""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_chain_entry_errors",
                                                  os.path.join(GOLDEN, "make_golden_chain_entry_errors.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_the_table_covers_the_eight_entry_points_and_every_pair():
    gen = _generator()
    recorded = json.load(open(gen.FIXTURE))
    assert [(e, n) for e, n, _, _ in recorded] == [(e, n) for e, n, _ in gen.cases()]
    assert {e for e, _, _, _ in recorded} == set(gen.SIGNATURES) and len(gen.SIGNATURES) == 8
    assert all(status != 0 and message for _, _, status, message in recorded)


@pytest.mark.gpu
def test_every_bad_argument_is_answered_as_recorded():
    gen = _generator()
    recorded = json.load(open(gen.FIXTURE))
    got = gen.run()
    assert len(got) == len(recorded)
    wrong = [(now, then) for now, then in zip(got, recorded) if now != then]
    assert not wrong, f"{len(wrong)} of {len(recorded)} cases differ; the first (now, recorded): {wrong[:5]}"
