"""
utils.funcs.chain_step_grid, the one per-expiry step grid of the host, against every copy of the formula it replaced -- frozen
below as they stood -- and against time_grid_steps, bit for bit: the grid decides which random numbers a path sees, and the
conditional routes promise the bits of the fused C drivers' grid (svmc_chain.hip expiry_grids).  No GPU.
"""
import numpy as np
import pytest

from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp, logsv_pricer as lp
from stochvolmodels_amd.utils.funcs import chain_step_grid, time_grid_steps


def frozen_cond_rows_grid(ttms, nb_steps_per_year):
    """the inline loop of HipEngine.step_hawkesjd_chain_cond_rows and the body of hawkes_jd_pricer.jump_step_grid"""
    if int(nb_steps_per_year) <= 0:
        raise ValueError("nb_steps_per_year must be positive")
    nbs, dts, t0 = [], [], 0.0
    for t in np.asarray(ttms, dtype=np.float64).ravel():
        d = float(t) - t0
        nb = int(d * float(int(nb_steps_per_year))) + 1
        nbs.append(nb)
        dts.append(d if nb == 1 else d / float(nb))
        t0 = float(t)
    return nbs, dts


def frozen_one_expiry_grid(ttm, nb_steps_per_year):
    """logsv_pricer.one_expiry_grid"""
    if int(nb_steps_per_year) <= 0:
        raise ValueError("nb_steps_per_year must be positive")
    nb = int(float(ttm) * float(int(nb_steps_per_year))) + 1
    return nb, (float(ttm) if nb == 1 else float(ttm) / float(nb))


def frozen_gap_loop(ttms, nb_steps_per_year):
    """the `for ttm in ttms: time_grid_steps(ttm - t0, ...)` loops of logsv_pricer.py and heston_pricer.py, time_grid_steps' body
    written out"""
    grids, t0 = [], 0.0
    for ttm in ttms:
        gap = ttm - t0
        nb_steps = int(gap * nb_steps_per_year) + 1
        grids.append((nb_steps, float(gap) / nb_steps))
        t0 = ttm
    return [g[0] for g in grids], [g[1] for g in grids]


CHAINS = {
    1: np.array([1.0 / 3.0]),
    # inexact products (1/12, 1/3), an exact multiple of every step (0.25 -> 0.5 after 1/3: a gap of 1/6; 1.0 -> 2.0: a gap of 1.0)
    4: np.array([1.0 / 12.0, 0.25, 1.0 / 3.0, 1.0]),
    # gaps shorter than one step of every grid (1e-4 year: nb == 1), equal neighbours' gaps, and long ones
    17: np.cumsum([1e-4, 1.0 / 12.0, 1e-4, 0.25 - 1.0 / 12.0 - 2e-4, 1.0 / 3.0 - 0.25, 1.0 / 360.0, 1.0 / 1800.0, 2.0 / 3.0 - 1.0 / 360.0
                   - 1.0 / 1800.0, 1.0, 5e-4, 0.5, 1.0 / 12.0, 1.0 / 12.0, 0.1, 0.7, 1.0 / 3.0, 2.0]),
}
SPYS = (1, 12, 360, 1800)


def bits(grid):
    nbs, dts = grid
    assert all(type(n) is int for n in nbs) and all(type(d) is float for d in dts)
    return list(nbs), [float(d).hex() for d in dts]


@pytest.mark.parametrize("m", list(CHAINS))
@pytest.mark.parametrize("spy", SPYS)
def test_one_grid_is_every_copy_it_replaced(m, spy):
    ttms = CHAINS[m]
    assert ttms.size == m and np.all(np.diff(ttms) > 0)
    want = bits(chain_step_grid(ttms, spy))
    assert want == bits(frozen_cond_rows_grid(ttms, spy))
    assert want == bits(frozen_gap_loop(ttms, spy)) == bits(frozen_gap_loop([float(t) for t in ttms], spy))
    assert want == bits(hp.jump_step_grid(ttms, spy)) == bits(chain_step_grid(list(ttms), spy))
    gaps = np.diff(np.concatenate([[0.0], ttms]))
    per_gap = [time_grid_steps(float(t) - (float(ttms[i - 1]) if i else 0.0), spy) for i, t in enumerate(ttms)]
    assert want == bits(([g[0] for g in per_gap], [g[1] for g in per_gap]))
    for t in ttms:                                              # one expiry from the origin
        one = frozen_one_expiry_grid(t, spy)
        assert lp.one_expiry_grid(t, spy) == one == time_grid_steps(float(t), spy)
        assert bits(chain_step_grid([t], spy)) == bits(([one[0]], [one[1]]))
    assert sum(want[0]) >= m and len(gaps) == m


def test_the_cases_the_grid_is_asked_about():
    nbs, dts = chain_step_grid(CHAINS[17], 12)
    assert nbs[0] == 1 and dts[0] == float(CHAINS[17][0])        # a gap shorter than a step: one step of the gap's length
    nbs, dts = chain_step_grid([0.25, 0.5], 12)                  # exact multiples of the step still take one step more
    assert nbs == [4, 4] and dts == [0.0625, 0.0625]
    assert chain_step_grid([1.0 / 12.0], 12)[0] == [2] and chain_step_grid([1.0], 360)[0] == [361]
    assert chain_step_grid([], 12) == ([], [])
    assert chain_step_grid([0.5], 12.9) == chain_step_grid([0.5], 12)      # the C drivers take an int


@pytest.mark.parametrize("spy", (0, -12))
def test_a_non_positive_step_count_is_refused(spy):
    for call in (lambda: chain_step_grid([0.1], spy), lambda: hp.jump_step_grid([0.1], spy), lambda: lp.one_expiry_grid(0.1, spy)):
        with pytest.raises(ValueError, match="^nb_steps_per_year must be positive$"):
            call()
