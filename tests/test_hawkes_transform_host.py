"""
tests/golden/hawkes_transform_odes.npz (make_golden_hawkes_transform_odes.py: the Hawkes coefficient ODEs of the reference's
solve_ode_for_a, solved twice in mpmath) can see a subtle error.  No device is needed:

  * a plain numpy double-precision RK4 of the same right-hand side, written here from the reference's formulas, reproduces
    every stored value (all sets, ttms, points, the three components and log E, and the chained pair) to 1e-9 in the ODE
    metric |x - mp| / max(1, |mp|), at a step count doubled until two runs agree to 1e-10;
  * the same RK4 with ONE term wrong -- each of MUTATIONS -- differs from the stored values by at least 1e-5 somewhere: an
    error of that kind in a kernel cannot pass the device tests' bound (tests/test_gpu_hawkes_transform.py, <= 1e-8);
  * the decoupled set's closed form, evaluated here in mpmath, equals its stored copy and the stored solves to 1e-15.

A stored point is `defined` unless the exact solution has a pole before the ttm (a real phi of the forwards kernel at two
years); those are left out here and must come back NaN from the device.
"""
import os

import mpmath as mp
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RK4_START_STEPS = 1000
RK4_SELF_AGREEMENT = 1e-10
RK4_BOUND = 1e-9
MUTATION_FLOOR = 1e-5
MUTATIONS = ("beta1_m <-> beta2_p", "comp_m from 1 + mean_m", "kappa_p <-> kappa_m in the decay terms", "kth_m dropped from a0'",
             "shift_m negated in the exponential", "h0 with phi (phi - 1)", "lambda_p <-> lambda_m in log E")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "hawkes_transform_odes.npz"))


def columns(fx):
    """the parameters as [S, 1] columns by name"""
    return {str(k): fx["params"][:, i:i + 1] for i, k in enumerate(fx["param_names"])}


def rhs(p, phi, a, mutation=None):
    """func_rhs of solve_ode_for_a (psi = 0) on a [3, S, P]; `mutation`: one of MUTATIONS, the single wrong term"""
    b1p, b2p, b1m, b2m = p["beta1_p"], p["beta2_p"], p["beta1_m"], p["beta2_m"]
    if mutation == MUTATIONS[0]:
        b1m, b2p = b2p, b1m
    comp_p = np.exp(p["shift_p"]) / (1.0 - p["mean_p"]) - 1.0
    comp_m = np.exp(p["shift_m"]) / ((1.0 + p["mean_m"]) if mutation == MUTATIONS[1] else (1.0 - p["mean_m"])) - 1.0
    kp, km = (p["kappa_m"], p["kappa_p"]) if mutation == MUTATIONS[2] else (p["kappa_p"], p["kappa_m"])
    z_p = phi - b1p * a[1] - b1m * a[2]
    z_m = phi - b2p * a[1] - b2m * a[2]
    j_p = np.exp(-p["shift_p"] * z_p) / (1.0 + p["mean_p"] * z_p) - 1.0
    j_m = np.exp((p["shift_m"] if mutation == MUTATIONS[4] else -p["shift_m"]) * z_m) / (1.0 + p["mean_m"] * z_m) - 1.0
    h0 = p["sigma"] ** 2 * (0.5 * ((phi - 1.0) if mutation == MUTATIONS[5] else (phi + 1.0)) * phi)
    kth_m = 0.0 if mutation == MUTATIONS[3] else p["kappa_m"] * p["theta_m"]
    return np.stack([p["kappa_p"] * p["theta_p"] * a[1] + kth_m * a[2] + h0, j_p - kp * a[1] + comp_p * phi,
                     j_m - km * a[2] + comp_m * phi])


def log_mgf(p, a, mutation=None):
    lp, lm = (p["lambda_m"], p["lambda_p"]) if mutation == MUTATIONS[6] else (p["lambda_p"], p["lambda_m"])
    return a[0] + a[1] * lp + a[2] * lm


def rk4(p, phi, a0, ttm, steps, mutation=None):
    h = ttm / steps
    a = np.array(a0, dtype=np.complex128)
    with np.errstate(all="ignore"):                        # a point past its pole overflows; those are masked by the caller
        for _ in range(steps):
            k1 = rhs(p, phi, a, mutation)
            k2 = rhs(p, phi, a + 0.5 * h * k1, mutation)
            k3 = rhs(p, phi, a + 0.5 * h * k2, mutation)
            k4 = rhs(p, phi, a + h * k3, mutation)
            a = a + (h / 6.0) * (k1 + 2.0 * (k2 + k3) + k4)
    return a


def metric(a, lm, a_mp, lm_mp, defined):
    """|x - mp| / max(1, |mp|), the largest over the components and log E, per point; 0 where the point is not defined"""
    with np.errstate(all="ignore"):
        e = np.abs(np.moveaxis(a, 0, -1) - a_mp) / np.maximum(1.0, np.abs(a_mp))
        e = np.maximum(e.max(axis=-1), np.abs(lm - lm_mp) / np.maximum(1.0, np.abs(lm_mp)))
    assert np.all(np.isfinite(e[defined]))
    return np.where(defined, e, 0.0)


@pytest.fixture(scope="module")
def converged(fx):
    """per ttm: (the step count at which RK4 agrees with itself at half the steps to 1e-10, its result [3, S, P])"""
    p, phi = columns(fx), fx["phi"]
    out = []
    for t, ttm in enumerate(fx["ttms"]):
        defined = fx["defined"][:, t]
        steps, prev = RK4_START_STEPS, rk4(p, phi, np.zeros((3,) + phi.shape), float(ttm), RK4_START_STEPS)
        while True:
            steps *= 2
            a = rk4(p, phi, np.zeros((3,) + phi.shape), float(ttm), steps)
            change = metric(a, log_mgf(p, a), np.moveaxis(prev, 0, -1), log_mgf(p, prev), defined).max()
            prev = a
            if change <= RK4_SELF_AGREEMENT:
                break
            assert steps < 200_000, (ttm, steps, change)
        out.append((steps, a))
    return out


def test_fixture_is_converged(fx):
    d = fx["defined"]
    assert np.max(fx["agree"][d]) <= 1e-16 and np.max(fx["chain_agree"]) <= 1e-16
    assert np.all(np.isfinite(fx["a"][d])) and np.all(np.isfinite(fx["log_mgf"][d]))
    assert np.all(np.isnan(fx["a"][~d].real))
    # what is not defined: real points at the longest ttm only, and never on the default or the decoupled set
    S, T, P = d.shape
    n_grid = int(fx["n_grid_points"])
    assert np.all(d[:, :T - 1]) and np.all(d[:, :, :n_grid])
    names = [str(n) for n in fx["names"]]
    assert np.all(d[names.index("default")]) and np.all(d[names.index("decoupled")]) and np.all(d[names.index("asym")])
    assert list(fx["param_names"]) == ["mu", "sigma", "shift_p", "mean_p", "shift_m", "mean_m", "lambda_p", "theta_p", "kappa_p",
                                       "beta1_p", "beta2_p", "lambda_m", "theta_m", "kappa_m", "beta1_m", "beta2_m"]


def test_rk4_reproduces_the_stored_values(fx, converged):
    p = columns(fx)
    worst = 0.0
    for t, (steps, a) in enumerate(converged):
        e = metric(a, log_mgf(p, a), fx["a"][:, t], fx["log_mgf"][:, t], fx["defined"][:, t])
        print(f"RK4 vs mp, ttm {float(fx['ttms'][t]):.4g}: {e.max():.3g} at {steps} steps")
        worst = max(worst, float(e.max()))
    # the chained pair: the second slice from the stored (rounded) state of the first
    s = int(fx["chain_set"])
    ps = {k: v[s:s + 1] for k, v in p.items()}
    phi = fx["phi"][s:s + 1]
    every = np.ones(phi.shape, dtype=bool)
    t0, t1 = (float(v) for v in fx["chain_ttms"])
    a_first = rk4(ps, phi, np.zeros((3,) + phi.shape), t0, converged[1][0])
    e0 = metric(a_first, np.zeros(phi.shape), fx["chain_a_first"][None], np.zeros(phi.shape), every).max()
    a_second = rk4(ps, phi, np.moveaxis(fx["chain_a_first"][None], -1, 0), t1, converged[1][0])
    e1 = metric(a_second, log_mgf(ps, a_second), fx["chain_a"][None], fx["chain_log_mgf"][None], every).max()
    print(f"RK4 vs mp, chained pair: {e0:.3g}, {e1:.3g}")
    assert max(worst, float(e0), float(e1)) <= RK4_BOUND


def test_every_single_term_mutation_is_seen(fx, converged):
    p, phi = columns(fx), fx["phi"]
    moved = {}
    for mutation in MUTATIONS:
        worst = 0.0
        for t, (steps, _) in enumerate(converged):
            a = rk4(p, phi, np.zeros((3,) + phi.shape), float(fx["ttms"][t]), steps, mutation)
            lm = log_mgf(p, a, mutation)
            with np.errstate(all="ignore"):
                e = np.abs(np.moveaxis(a, 0, -1) - fx["a"][:, t]) / np.maximum(1.0, np.abs(fx["a"][:, t]))
                e = np.maximum(e.max(axis=-1), np.abs(lm - fx["log_mgf"][:, t]) / np.maximum(1.0, np.abs(fx["log_mgf"][:, t])))
            e = e[fx["defined"][:, t]]
            # a mutated run may itself meet a pole: its non-finite points are left out, so only finite differences count
            worst = max(worst, float(np.max(e[np.isfinite(e)])))
        moved[mutation] = worst
    print("mutation: worst |x - mp| / max(1, |mp|) over all sets and points (floor %.0e)" % MUTATION_FLOOR)
    for mutation, v in moved.items():
        print(f"  {mutation:42s} {v:.3g}")
    for mutation, v in moved.items():
        assert v >= MUTATION_FLOOR, (mutation, v)


def closed_form_mp(params, phi, ttm):
    """[a0, a1, a2] of a set whose four betas are zero: a_i' = c_i - kappa_i a_i with c_i = j_i(phi) + comp_i phi constant"""
    q = {k: mp.mpf(float(v)) for k, v in params.items()}
    phi, t = mp.mpc(complex(phi)), mp.mpf(float(ttm))
    a, integral = [], []
    for s in ("p", "m"):
        comp = mp.exp(q["shift_" + s]) / (1 - q["mean_" + s]) - 1
        c = mp.exp(-q["shift_" + s] * phi) / (1 + q["mean_" + s] * phi) - 1 + comp * phi
        k = q["kappa_" + s]
        decay = -mp.expm1(-k * t) / k                                   # int_0^t exp(-k (t - s)) ds
        a.append(c * decay)
        integral.append(c * (t - decay) / k)
    a0 = q["sigma"] ** 2 * (phi + 1) * phi / 2 * t + q["kappa_p"] * q["theta_p"] * integral[0] + q["kappa_m"] * q["theta_m"] * integral[1]
    return [a0] + a


def test_decoupled_closed_form_equals_the_stored_values(fx):
    s = [str(n) for n in fx["names"]].index("decoupled")
    params = {str(k): fx["params"][s, i] for i, k in enumerate(fx["param_names"])}
    assert all(params[k] == 0.0 for k in ("beta1_p", "beta2_p", "beta1_m", "beta2_m"))
    worst = 0.0
    with mp.workdps(50):
        for t, ttm in enumerate(fx["ttms"]):
            for i, phi in enumerate(fx["phi"][s]):
                y = closed_form_mp(params, phi, ttm)
                y.append(y[0] + y[1] * mp.mpf(float(params["lambda_p"])) + y[2] * mp.mpf(float(params["lambda_m"])))
                for stored in ((*fx["a"][s, t, i], fx["log_mgf"][s, t, i]), (*fx["closed_a"][t, i], fx["closed_log_mgf"][t, i])):
                    for v, w in zip(y, stored):
                        worst = max(worst, float(abs(v - mp.mpc(complex(w))) / max(1, abs(v))))
    print(f"decoupled closed form vs the stored values: {worst:.3g}")
    assert worst <= 1e-15
