"""
The four payoff tails that work on a chain's quote table -- svmc_greeks_payoff_chain, svmc_cmc_payoff_chain, svmc_cmc_greeks_chain
and svmc_cmc_sens_chain -- replayed against tests/golden/quote_tails.npz (make_golden_quote_tails.py, recorded on the commit
before the tails got one quote check, one image builder and one workspace layout each): every output equal to the bit, the five
workspace size functions equal on the grid, and every chain with one fault answered with the recorded status and text, by the
tails and by the four fused drivers that make the same checks.
"""
import importlib.util
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_quote_tails", os.path.join(GOLDEN, "make_golden_quote_tails.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_the_fixture_holds_the_generators_inputs_and_every_case():
    gen = _generator()
    rec = np.load(gen.FIXTURE, allow_pickle=False)
    inputs = gen.make_inputs()
    assert {k[4:] for k in rec.files if k.startswith("in__")} == set(inputs)
    for name, arr in inputs.items():
        assert arr.dtype == rec["in__" + name].dtype and np.array_equal(arr.view(np.uint8), rec["in__" + name].view(np.uint8)), name
    assert rec["in__offsets"].tolist() == [0, 1, 1, 10, 18, 18] and rec["in__planted__mu"].shape == (5, 2 * 256 + 37)
    assert set(rec["in__types"][1:10].tolist()) == {0, 1} and set(rec["in__types"][10:18].tolist()) == {0, 1}
    errors = json.loads(str(rec["errors"]))
    assert [(e, n) for e, n, _, _ in errors] == [(e, n) for e, n, _ in gen.cases()]
    assert {e for e, _, _, _ in errors} == set(gen.SIGNATURES) and len(gen.SIGNATURES) == 8
    assert all(status != 0 and message for _, _, status, message in errors)
    assert rec["sizes"].shape == (4, 4, 3, 5) and (rec["sizes"] % 8 == 0).all()
    # the generator's self-check, on the recorded bits
    out = {k[5:]: rec[k].view(np.float64) for k in rec.files if k.startswith("out__")}
    assert len(out) == 3 * (2 * 6 + 2) and gen.self_check(out) == []
    lo, hi = 1, 10
    assert not np.isfinite(out["no_kept_path__cmc_payoff__r1__prices"][lo:hi]).any()


@pytest.mark.gpu
def test_the_tails_the_sizes_and_the_refusals_replay_to_the_bit():
    from stochvolmodels_amd import _lib
    gen = _generator()
    rec = np.load(gen.FIXTURE, allow_pickle=False)
    inputs = {k[4:]: rec[k] for k in rec.files if k.startswith("in__")}
    got, broken = gen.run(_lib.load(), inputs)
    assert broken == []
    assert set(got) == {k for k in rec.files if not k.startswith("in__")}
    wrong = [k for k in got if k.startswith("out__") and not (got[k].shape == rec[k].shape and (got[k] == rec[k]).all())]
    assert not wrong, f"{len(wrong)} outputs differ from the recorded bits: {wrong[:6]}"
    assert (got["sizes"] == rec["sizes"]).all(), np.argwhere(got["sizes"] != rec["sizes"])[:6]
    now, then = json.loads(str(got["errors"])), json.loads(str(rec["errors"]))
    assert len(now) == len(then)
    differ = [(a, b) for a, b in zip(now, then) if a != b]
    assert not differ, f"{len(differ)} of {len(then)} cases differ; the first (now, recorded): {differ[:5]}"
