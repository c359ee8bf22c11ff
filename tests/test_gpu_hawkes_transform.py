"""
The Hawkes jump-diffusion's transform kernels against independent high-precision truth (tests/golden/hawkes_transform_odes.npz,
make_golden_hawkes_transform_odes.py: the coefficient ODEs of the reference's solve_ode_for_a solved twice in mpmath, agreeing
to 1e-16; tests/test_hawkes_transform_host.py shows that the fixture sees any single wrong term at 1e-5 or more):

  * hawkes_rhs / hawkes_dop853 / hawkes_mgf_grid_batch_kernel (svmc_hawkesjd_mgf_grid_batch, svmc_hawkesjd_mgf_grid): all three
    components and log E of every set (default, excited, asymmetric cross-excitation, decoupled, pure shift, no shift,
    kappa_m = 0, sigma = 0), ttm (1/365, 0.25, 2 years) and point (the pricer grid's ends and interior, and the real points of
    the forwards kernel), at rtol 1e-12 / atol 1e-14 and at the pricer's own 1e-10 / 1e-12; the decoupled set against its
    closed form; the a_t0 carry (a chained pair); points whose exact solution has a pole before the ttm come back NaN;
  * the launch shapes: n_grid of 1, 63, 64, 65 and 130 (HK_AB = 64 lanes a block, the last block partly empty), every tile of
    the points bit-equal to the first, nothing written past n_grid; 1, 2, 16 and 17 sets (HK_MAX_SETS = 16 a launch), each set
    on its own grid and parameters bit-equal to its single call and within the bound of mp for its own parameters;
  * the give-up: one point with a pole before the ttm returns NaN in all three components and its 63 neighbours in the wave
    stay within the bound;
  * hawkes_risk_forwards_kernel (svmc_hawkesjd_risk_forwards_batch): normalizers and gamma forwards against the same formed in
    mp from the stored real-phi solutions; 1, 2, 31, 32, 33 and 65 expiries (HK_RISK_MAX_TTMS = 32 lane pairs a launch) by 1, 16
    and 17 sets, every (expiry, set) entry at [expiry][set] and equal to its one-expiry, one-set call.

Errors are |dev - mp| / max(1, |mp|), the largest over a point's components and log E (relative errors for the forwards).
Each bound is four times the worst value measured on an MI355X (profiles/hawkes_transform_observed_tolerances.txt): the last
bits of an adaptive integrator move with the compiler's scheduling.  The ceilings asserted below are what keeps a wrong term
visible.
"""
import os

import mpmath as mp
import numpy as np
import pytest

from test_gpu_transform_odes import Dev, _check, _pf, ode_err, report

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HK_AB, HK_MAX_SETS, HK_RISK_MAX_TTMS = 64, 16, 32           # csrc/svmc_hawkes.hip
TIGHT = (1e-12, 1e-14)
# Measured worst on the MI355X: 1.212e-12 (sigma_zero, 2 years, Im phi = 475), x 4
ODE_BOUND = 4.9e-12
assert ODE_BOUND <= 1e-8
# at the pricer's own tolerances (1e-10 / 1e-12): measured worst 1.548e-10 (sigma_zero, 2 years, the last grid point), x 4
PRICER_BOUND = 6.2e-10
assert PRICER_BOUND <= 1e-6
# relative, normalizers and gamma forwards: measured worst 4.342e-14 (default set), x 4
FORWARDS_BOUND = 1.8e-13
assert FORWARDS_BOUND <= 1e-8
SENTINEL = complex(-7.25, 3.5)
PAD = 5                         # elements past the end of each output buffer


@pytest.fixture(scope="module")
def L():
    from stochvolmodels_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "hawkes_transform_odes.npz"))


def pricer_tolerances():
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp
    return hp.ODE_RTOL, hp.ODE_ATOL


def grid_batch(L, phi, ttm, rows, tol=TIGHT, a0=None, single=False):
    """svmc_hawkesjd_mgf_grid_batch (or, at one set with single=True, svmc_hawkesjd_mgf_grid) on [n_sets][n] grids at psi = 0:
    (a [n_sets][n][3], log E [n_sets][n]); both output buffers carry PAD sentinel elements past the end, checked here"""
    phi = np.ascontiguousarray(np.atleast_2d(phi), dtype=np.complex128)
    rows = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.float64)
    s, n = phi.shape
    assert rows.shape == (s, 16)
    a_host = np.full(3 * s * n + PAD, SENTINEL)
    a_host[:3 * s * n] = 0.0 if a0 is None else np.asarray(a0, dtype=np.complex128).ravel()
    a, lm = Dev(L, a_host), Dev(L, np.full(s * n + PAD, SENTINEL))
    dphi, dpsi = Dev(L, phi), Dev(L, np.zeros_like(phi))
    if single:
        assert s == 1
        _check(L.svmc_hawkesjd_mgf_grid(dphi.ptr, dpsi.ptr, n, float(ttm), _pf(rows), a.ptr, lm.ptr, tol[0], tol[1], None))
    else:
        _check(L.svmc_hawkesjd_mgf_grid_batch(dphi.ptr, dpsi.ptr, n, s, float(ttm), _pf(rows), a.ptr, lm.ptr, tol[0], tol[1], None))
    a_out, lm_out = a.get(3 * s * n + PAD, np.complex128), lm.get(s * n + PAD, np.complex128)
    assert np.all(a_out[3 * s * n:] == SENTINEL) and np.all(lm_out[s * n:] == SENTINEL), "written past n_grid"
    return a_out[:3 * s * n].reshape(s, n, 3), lm_out[:s * n].reshape(s, n)


def point_errors(a, lm, a_mp, lm_mp, defined, where):
    """the ODE metric per point; a point that is not defined (a pole before the ttm) must be NaN in all three components"""
    assert np.all(np.isnan(a[~defined].real) & np.isnan(a[~defined].imag)), ("a pole stepped over", where)
    assert np.all(np.isfinite(a[defined])) and np.all(np.isfinite(lm[defined])), ("a grid point given up", where)
    return ode_err(a[defined], lm[defined], a_mp[defined], lm_mp[defined])


# ---- every set, ttm and point against mp -----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tight", "pricer"])
def test_grid_kernel_vs_mp(L, fx, which):
    tol, bound = (TIGHT, ODE_BOUND) if which == "tight" else (pricer_tolerances(), PRICER_BOUND)
    assert np.max(fx["agree"]) <= 1e-16
    overall = 0.0
    for s, name in enumerate(fx["names"]):
        worst, where = 0.0, None
        for t, ttm in enumerate(fx["ttms"]):
            a, lm = grid_batch(L, fx["phi"][s], ttm, fx["params"][s], tol)
            e = point_errors(a[0], lm[0], fx["a"][s, t], fx["log_mgf"][s, t], fx["defined"][s, t], (str(name), float(ttm)))
            if e.size and e.max() > worst:
                worst, where = float(e.max()), (float(ttm), complex(fx["phi"][s][fx["defined"][s, t]][e.argmax()]))
        print(f"{name}: worst at (ttm, phi)", where)
        report(f"Hawkes grid vs mp, {which} tolerances, set {name}", worst, bound)
        overall = max(overall, worst)
    report(f"Hawkes grid vs mp, {which} tolerances, all sets", overall, bound)


def test_decoupled_set_vs_closed_form(L, fx):
    s = [str(n) for n in fx["names"]].index("decoupled")
    worst = 0.0
    for t, ttm in enumerate(fx["ttms"]):
        a, lm = grid_batch(L, fx["phi"][s], ttm, fx["params"][s])
        worst = max(worst, float(ode_err(a[0], lm[0], fx["closed_a"][t], fx["closed_log_mgf"][t]).max()))
    report("Hawkes grid vs the decoupled set's closed form", worst, ODE_BOUND)


def test_chained_pair_vs_mp(L, fx):
    """the a_t0 carry: 0.1 years from zero, then 0.15 more from the stored state of the first"""
    s = int(fx["chain_set"])
    assert np.max(fx["chain_agree"]) <= 1e-16
    t0, t1 = fx["chain_ttms"]
    phi, P = fx["phi"][s], fx["phi"].shape[1]
    a0, _ = grid_batch(L, phi, t0, fx["params"][s])
    first = float(ode_err(a0[0], np.zeros(P), fx["chain_a_first"], np.zeros(P)).max())
    a1, lm1 = grid_batch(L, phi, t1, fx["params"][s], a0=fx["chain_a_first"])
    second = float(ode_err(a1[0], lm1[0], fx["chain_a"], fx["chain_log_mgf"]).max())
    # and carried on the device, as the pricer does it: the first slice's own output in
    a2, lm2 = grid_batch(L, phi, t1, fx["params"][s], a0=a0)
    carried = float(ode_err(a2[0], lm2[0], fx["chain_a"], fx["chain_log_mgf"]).max())
    report("Hawkes chained pair, first slice vs mp", first, ODE_BOUND)
    report("Hawkes chained pair, second slice from the stored state vs mp", second, ODE_BOUND)
    report("Hawkes chained pair, second slice from the device's state vs mp", carried, 2 * ODE_BOUND)


# ---- launch shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_grid", [1, HK_AB - 1, HK_AB, HK_AB + 1, 2 * HK_AB + 2])
def test_grid_lengths_around_the_block(L, fx, n_grid):
    """one set and ttm suffice: the kernel's guard is `j >= n_grid` and a lane's work depends on its own point alone"""
    s, t = [str(n) for n in fx["names"]].index("asym"), 1
    P = fx["phi"].shape[1]
    idx = np.arange(n_grid) % P
    a, lm = grid_batch(L, fx["phi"][s][idx], fx["ttms"][t], fx["params"][s])
    a, lm = a[0], lm[0]
    assert np.array_equal(a, a[idx]) and np.array_equal(lm, lm[idx]), "a tile of the points differs from the first"
    worst = float(ode_err(a, lm, fx["a"][s, t][idx], fx["log_mgf"][s, t][idx]).max())
    report(f"Hawkes grid vs mp, n_grid {n_grid}", worst, ODE_BOUND)


def batch_order(fx, n_sets):
    """fixture set indices for a batch: neighbours differ, the 17th set is not the 1st"""
    S = len(fx["names"])
    return [(3 * i + i // S) % S for i in range(n_sets)]


@pytest.mark.parametrize("n_sets", [1, 2, HK_MAX_SETS, HK_MAX_SETS + 1])
def test_batch_of_sets(L, fx, n_sets):
    """each set on its own grid (its own vol_scaler) with its own parameters: bit-equal to its single call, and within the
    bound of mp for ITS parameters -- a set index applied to the grid but not to the constants fails the second"""
    t = 1
    order = batch_order(fx, n_sets)
    assert all(a != b for a, b in zip(order, order[1:]))
    a, lm = grid_batch(L, fx["phi"][order], fx["ttms"][t], fx["params"][order])
    worst = 0.0
    for i, s in enumerate(order):
        a1, lm1 = grid_batch(L, fx["phi"][s], fx["ttms"][t], fx["params"][s], single=True)
        assert np.array_equal(a[i], a1[0]) and np.array_equal(lm[i], lm1[0]), (n_sets, i, "differs from its single call")
        worst = max(worst, float(ode_err(a[i], lm[i], fx["a"][s, t], fx["log_mgf"][s, t]).max()))
    report(f"Hawkes grid vs mp, {n_sets} sets in a batch", worst, ODE_BOUND)


def test_give_up_is_one_lanes_own(L, fx):
    """one wave; lane 37 integrates towards a pole (1 + mean_p z_p -> 0 before the ttm) and gives up, the other 63 do not notice.
    The point and the ttm are those of the `failed` entries of hawkes_risk_premia.npz (gamma 4.8 at half a year: of the
    entry's two points it is phi = -gamma - 1 whose solution ends before the ttm)"""
    s = [str(n) for n in fx["names"]].index("default")
    P, at = fx["phi"].shape[1], 37
    idx = np.arange(HK_AB) % P
    phi = fx["phi"][s][idx].copy()
    phi[at] = complex(fx["giveup_phi"])                 # -gamma - 1 of the reference's failed entry
    a, lm = grid_batch(L, phi, fx["giveup_ttm"], fx["params"][s])
    a, lm = a[0], lm[0]
    assert np.all(np.isnan(a[at].real)) and np.all(np.isnan(a[at].imag)) and np.isnan(lm[at])
    keep = np.arange(HK_AB) != at
    assert np.all(np.isfinite(a[keep])) and np.all(np.isfinite(lm[keep]))
    assert np.max(fx["giveup_agree"]) <= 1e-16
    worst = float(ode_err(a[keep], lm[keep], fx["giveup_a"][idx][keep], fx["giveup_log_mgf"][idx][keep]).max())
    report("Hawkes grid vs mp, the 63 neighbours of a lane that gives up", worst, ODE_BOUND)


# ---- the risk-premia forwards ------------------------------------------------------------------------------------------------
FORWARD_SETS = ("default", "asym", "decoupled")


def forwards(L, rows, gammas, ttms, fwds, tol=TIGHT):
    """svmc_hawkesjd_risk_forwards_batch: (normalizers, gamma_forwards), each [n_ttms][n_sets]"""
    rows = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.float64)
    gammas, ttms, fwds = (np.ascontiguousarray(np.atleast_1d(v), dtype=np.float64) for v in (gammas, ttms, fwds))
    s, m = rows.shape[0], ttms.size
    assert gammas.size == s and fwds.size == m
    norm, gfwd = Dev(L, np.full(m * s + PAD, SENTINEL.real)), Dev(L, np.full(m * s + PAD, SENTINEL.real))
    _check(L.svmc_hawkesjd_risk_forwards_batch(_pf(rows), _pf(gammas), s, _pf(ttms), _pf(fwds), m, norm.ptr, gfwd.ptr, tol[0],
                                               tol[1], None))
    n_out, g_out = norm.get(m * s + PAD, np.float64), gfwd.get(m * s + PAD, np.float64)
    assert np.all(n_out[m * s:] == SENTINEL.real) and np.all(g_out[m * s:] == SENTINEL.real), "written past the last entry"
    return n_out[:m * s].reshape(m, s), g_out[:m * s].reshape(m, s)


def mp_forwards(fx, s, g, t, forward):
    """(normalizer, gamma_forward) in mp from the stored solutions at phi = -gamma and -gamma - 1"""
    n_grid = int(fx["n_grid_points"])
    assert fx["phi"][s, n_grid + 2 * g] == complex(-fx["gammas"][g]) and fx["phi"][s, n_grid + 2 * g + 1] == complex(-fx["gammas"][g] - 1)
    with mp.workdps(40):
        normalizer = mp.exp(-mp.mpf(float(fx["log_mgf"][s, t, n_grid + 2 * g].real)))
        return normalizer, mp.mpf(float(forward)) * mp.exp(mp.mpf(float(fx["log_mgf"][s, t, n_grid + 2 * g + 1].real))) * normalizer


def rel(dev, ref):
    with mp.workdps(40):
        return float(abs(mp.mpf(float(dev)) - ref) / abs(ref))


def test_forwards_vs_mp(L, fx):
    names = [str(n) for n in fx["names"]]
    fwds = np.array([1.07, 0.93, 1.31])
    worst = 0.0
    for name in FORWARD_SETS:
        s = names.index(name)
        norm, gfwd = forwards(L, np.tile(fx["params"][s], (3, 1)), fx["gammas"], fx["ttms"], fwds)
        here = 0.0
        for t in range(3):
            for g in range(3):
                n_mp, g_mp = mp_forwards(fx, s, g, t, fwds[t])
                here = max(here, rel(norm[t, g], n_mp), rel(gfwd[t, g], g_mp))
        report(f"Hawkes risk forwards vs mp, set {name}", here, FORWARDS_BOUND)
        worst = max(worst, here)
    report("Hawkes risk forwards vs mp, all sets", worst, FORWARDS_BOUND)


N_EXPIRIES = (1, 2, HK_RISK_MAX_TTMS - 1, HK_RISK_MAX_TTMS, HK_RISK_MAX_TTMS + 1, 2 * HK_RISK_MAX_TTMS + 1)
N_FORWARD_SETS = (1, HK_MAX_SETS, HK_MAX_SETS + 1)


def test_forwards_shapes(L, fx):
    """expiries across the 32 lane pairs of a launch, sets across the 16 of a launch: expiry e has ttm e % 3 of the stored
    three and its own forward, set i the parameters i % 3 of FORWARD_SETS and its own gamma"""
    names = [str(n) for n in fx["names"]]
    E, S = max(N_EXPIRIES), max(N_FORWARD_SETS)
    ttms = fx["ttms"][np.arange(E) % 3]
    fwds = 0.8 + 0.01 * np.arange(E)
    which = [names.index(FORWARD_SETS[i % 3]) for i in range(S)]
    rows = fx["params"][which]
    # the first three are the stored gammas; the later ones move inwards from them, away from the poles of large |phi|
    gammas = fx["gammas"][np.arange(S) % 3] + np.array([0.0625, 0.0625, -0.0625])[np.arange(S) % 3] * (np.arange(S) // 3)
    assert np.unique(gammas).size == S and np.unique(fwds).size == E
    # the one-expiry, one-set calls, once
    single_n, single_g = np.empty((E, S)), np.empty((E, S))
    for e in range(E):
        for i in range(S):
            n1, g1 = forwards(L, rows[i], gammas[i], ttms[e], fwds[e])
            single_n[e, i], single_g[e, i] = n1[0, 0], g1[0, 0]
    assert np.all(np.isfinite(single_n)) and np.all(np.isfinite(single_g))
    worst_mp = 0.0
    for e in range(3):
        for i in range(3):
            n_mp, g_mp = mp_forwards(fx, which[i], i, e, fwds[e])
            worst_mp = max(worst_mp, rel(single_n[e, i], n_mp), rel(single_g[e, i], g_mp))
    report("Hawkes risk forwards, one-expiry one-set calls vs mp", worst_mp, FORWARDS_BOUND)
    identical, worst = True, 0.0
    for m in N_EXPIRIES:
        for s in N_FORWARD_SETS:
            norm, gfwd = forwards(L, rows[:s], gammas[:s], ttms[:m], fwds[:m])
            identical &= bool(np.array_equal(norm, single_n[:m, :s]) and np.array_equal(gfwd, single_g[:m, :s]))
            worst = max(worst, float(np.max(np.abs(norm - single_n[:m, :s]) / single_n[:m, :s])),
                        float(np.max(np.abs(gfwd - single_g[:m, :s]) / single_g[:m, :s])))
    print("every (expiry, set) entry bit-identical to its one-expiry, one-set call:", identical)
    report("Hawkes risk forwards, batch entries vs their single calls", worst, ODE_BOUND)
