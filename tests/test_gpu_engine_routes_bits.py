"""
Every chain route of the engine and every public pricer function over it, once, at the smallest sizes at which the host's
marshalling can still go wrong (1 000 paths: a multiple of neither 64 nor 256; three expiries with strikes of shape (2, 2), (3,) and
(1,) at ttms 1/12, 0.25, 0.5 and 12 steps a year; the chain cut to one expiry; fixed seeds), bit for bit against
tests/golden/engine_routes_bits.npz, and per route the kernel names the engine's timer reports.  The fixture was recorded by
tests/golden/make_golden_engine_calls.py on an MI355X on the commit before the chain entries got one call path (two runs of it
agreed in every bit); no kernel differs from that commit, so a difference here is a mistake of the host layer.  The chain with an
expiry without strikes is priced by that commit, so its results are held like the others.
"""
import json
import os

import numpy as np
import pytest

import engine_routes

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_routes_bits.npz"), allow_pickle=False)
NOTES = json.loads(str(GOLDEN["__notes__"]))


@pytest.fixture(scope="module")
def ran():
    """the routes run in the recording's order on one engine: later routes read the rows earlier ones left"""
    return engine_routes.run_gpu()


def test_the_same_routes_ran(ran):
    arrays, notes = ran
    assert list(notes) == list(NOTES) and len(NOTES) >= 87
    assert sorted(arrays) == sorted(k for k in GOLDEN.files if k != "__notes__")


@pytest.mark.parametrize("route", list(NOTES))
def test_route_bits_and_kernel_names(ran, route):
    arrays, notes = ran
    assert notes[route] == NOTES[route]                         # the timer's names, or the exception's type and text
    for k in (k for k in GOLDEN.files if k.startswith(route + "/")):
        got, want = arrays[k], GOLDEN[k]
        assert got.dtype == want.dtype and got.shape == want.shape, k
        assert got.tobytes() == want.tobytes(), (k, got, want)
