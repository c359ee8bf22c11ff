"""
The four weighted conditional tails -- svmc_tilted_cond_payoff_chain (libsvmc_ext.so), svmc_tilted_cond_greeks_chain,
svmc_cond_density_chain and svmc_jump_sets_payoff_chain (libsvmc_est.so) -- replayed against tests/golden/cond_tails.npz
(make_golden_cond_tails.py, recorded on the commit before the tails got one payoff body, one finish body and one host driver in
csrc/svmc_tilted_cond.h): every price, error, Greek, density, statistic, corr and forward block equal to the bit.
"""
import importlib.util
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_cond_tails", os.path.join(GOLDEN, "make_golden_cond_tails.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_the_fixture_holds_the_generators_inputs_and_every_output():
    gen = _generator()
    rec = np.load(gen.FIXTURE, allow_pickle=False)
    assert os.path.getsize(gen.FIXTURE) < 1 << 20
    inputs = gen.make_inputs()
    assert {k[4:] for k in rec.files if k.startswith("in__")} == set(inputs)
    for name, arr in inputs.items():
        assert arr.dtype == rec["in__" + name].dtype and np.array_equal(arr.view(np.uint8), rec["in__" + name].view(np.uint8)), name
    assert rec["in__offsets"].tolist() == [0, 1, 1, 10, 18, 18] and rec["in__planted__mu"].shape == (5, 2 * 256 + 37)
    assert set(rec["in__types"][1:10].tolist()) == {0, 1} and rec["in__strikes"][3] < -0.4
    mu, cv = rec["in__planted__mu"], rec["in__planted__cv"]
    assert (cv[:, 5] == 0).all() and (cv[:, 17] < 0).all() and np.isnan(mu[:, 300]).all() and (mu[:, -1] == np.inf).all()
    assert (mu[:, 40] == -150.0).all() and np.isnan(rec["in__path0_dropped__mu"][:, 0]).all()
    assert not np.isfinite(rec["in__no_kept_path__mu"][gen.EMPTY_EXPIRY]).any() and gen.N_LARGE == 1024 * 256 + 3
    # per stored variant two recenterings of (4 + 2 + 4) outputs and two densities of 3; the large one a recentering and a density
    out = {k[5:]: rec[k].view(np.float64) for k in rec.files if k.startswith("out__")}
    assert len(out) == 3 * (2 * 10 + 2 * 3) + (10 + 3) and gen.self_check(out) == []
    lo, hi = 1, 10
    for name in ("payoff__r1__prices", "sets__r0__prices", "density__g3__pdf"):
        assert np.isnan(out["no_kept_path__" + name].reshape(-1, gen.K)[:, lo:hi]).all(), name
    for which, gammas in gen.CD_GAMMAS.items():
        pdf = out[f"planted__density__{which}__pdf"].reshape(gammas.size, gen.K)
        assert np.isnan(pdf[-1]).all() and np.isfinite(pdf[:-1]).all() and gammas[-1] == gen.DROP_GAMMA
    # the path whose weight overflows is dropped at gamma -3 alone: n_dropped of the statistics
    stats = out["planted__payoff__r0__stats"].reshape(gen.GAMMAS.size, gen.M, 8)
    assert (stats[-1, :, 6] == stats[0, :, 6] + 1).all() and (stats[1:-1, :, 6] == stats[0, :, 6]).all() and (stats[0, :, 6] == 3).all()


@pytest.mark.gpu
def test_the_four_tails_replay_to_the_bit():
    from stochvolmodels_amd import _lib
    gen = _generator()
    rec = np.load(gen.FIXTURE, allow_pickle=False)
    inputs = {k[4:]: rec[k] for k in rec.files if k.startswith("in__")}
    got, broken = gen.run((_lib.load(), _lib.load_ext(), _lib.load_est()), inputs)
    assert broken == []
    assert set(got) == {k for k in rec.files if k.startswith("out__")}
    wrong = [k for k in got if not (got[k].shape == rec[k].shape and (got[k] == rec[k]).all())]
    assert not wrong, f"{len(wrong)} of {len(got)} outputs differ from the recorded bits: {wrong[:6]}"
