"""
The engine's host layer against a recording of itself, no GPU: for every HipEngine route of tests/engine_routes.py the ordered C
calls -- scalars by value, pointers by what they point at to the length the headers document, device addresses as the stand-in
engine hands them out -- what the route returns from outputs the stand-in library fills, the kernel names it reports to the timer,
and the type and text of every refusal with the C calls made before it.  tests/golden/engine_call_args.json was recorded by
tests/golden/make_golden_engine_calls.py on the commit before the chain entries got one call path; a rewrite of that layer must
reproduce it exactly.
"""
import inspect
import json
import os

import pytest

import engine_routes
from stochvolmodels_amd import engine

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_call_args.json")))
CASES = [(group, name) for group, routes in GOLDEN.items() for name in routes]


@pytest.fixture(scope="module")
def recorded():
    return engine_routes.record_host()


def test_the_recording_covers_the_routes(recorded):
    assert {g: list(v) for g, v in recorded.items()} == {g: list(v) for g, v in GOLDEN.items()}
    assert len(GOLDEN["three"]) == len(engine_routes.ROUTES) >= 43 and len(GOLDEN["refusals"]) >= 30
    called = {c[0] for routes in GOLDEN.values() for r in routes.values() for c in r["calls"]}
    assert set(engine_routes.LENGTHS) <= called                 # every entry point with a documented length is reached


@pytest.mark.parametrize("group,name", CASES, ids=[f"{g}-{n}" for g, n in CASES])
def test_route_is_the_recorded_one(recorded, group, name):
    got, want = recorded[group][name], GOLDEN[group][name]
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        assert g == w
    assert got == want


def test_every_refusal_is_an_error_and_every_route_is_not():
    for group, routes in GOLDEN.items():
        for name, r in routes.items():
            assert ("error" in r) == (group == "refusals"), (group, name)
    unknown = [r["error"] for n, r in GOLDEN["refusals"].items() if n.endswith(("_sabr", "_hawkesjd"))]
    assert len(unknown) == 12 and all(t == "ValueError" and ": unknown model '" in text for t, text in unknown)


def test_the_many_route_names_its_models():
    assert '"hawkesjd"' in inspect.getsource(engine.HipEngine.price_chain_many_fused)
