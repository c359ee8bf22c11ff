"""
Generate the Hawkes jump-diffusion golden vectors under tests/golden/ from the UNMODIFIED Python reference
(pricers/hawkes_jd_pricer.py).  Runs only in the build container, like make_golden.py (same _shims for numba):

    python tests/golden/make_golden_hawkes.py

  hawkes_mc.npz          hawkesjd_mc_chain_pricer on get_btc_test_chain_data() with default HawkesJDParams, 4096 paths, the
                         reference's 1800 steps per year (780 steps over the chain).  np.random.normal / uniform / exponential
                         are replaced by feeders that hand the reference the generator's own stream (tests/hawkes_twin.py), slice
                         by slice at chain-global step offsets -- the `feeder` idiom of make_golden.py's g_heston.  Stored: the
                         chain, the seed, prices, stderrs and the first 256 paths' (x, lambda_p, lambda_m) at every expiry.
  hawkes_mc_excited.npz  the same for a strongly self-exciting parameter set (clustered jumps, both sides in one step).
  hawkes_analytic.npz    hawkesjd_chain_pricer on the same chain at the reference's default solve_ivp tolerance and with the
                         solver tightened to rtol 1e-10 / atol 1e-12 (the g_analytic_tight idiom), plus the first expiry's
                         log_mgf on the transform grid (tightened).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "_shims"))
sys.path.insert(0, "/root/reference/src")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import stochvolmodels as svm  # noqa: E402
import stochvolmodels.pricers.hawkes_jd_pricer as hp  # noqa: E402
import stochvolmodels.utils.mgf_pricer as mgfp  # noqa: E402
from stochvolmodels.utils.config import VariableType  # noqa: E402
from stochvolmodels.utils.funcs import set_time_grid  # noqa: E402

import hawkes_twin as twin  # noqa: E402

N_PATH, KEEP, SEED = 4096, 256, 20251015
EXCITED = hp.HawkesJDParams(lambda_p=25.0, theta_p=15.0, kappa_p=30.0, beta1_p=150.0, beta2_p=-60.0,
                            lambda_m=30.0, theta_m=20.0, kappa_m=40.0, beta1_m=120.0, beta2_m=-200.0)


def save(name, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")


def chain_arrays(chain):
    out = dict(ttms=np.asarray(chain.ttms, dtype=np.float64), forwards=np.asarray(chain.forwards, dtype=np.float64),
               discfactors=np.asarray(chain.discfactors, dtype=np.float64))
    for i, (k, t) in enumerate(zip(chain.strikes_ttms, chain.optiontypes_ttms)):
        out[f"strikes_{i}"], out[f"types_{i}"] = np.asarray(k, dtype=np.float64), np.asarray(t)
    return out


def params_vec(p):
    return np.array([getattr(p, k) for k in twin.PARAM_NAMES])


def g_mc(name, params):
    chain = svm.get_btc_test_chain_data()
    n = N_PATH
    orig = (np.random.normal, np.random.uniform, np.random.exponential, hp.simulate_hawkesjd_terminal)
    state = dict(step0=0, states=[])

    def simulate(ttm, x0, lambda_p0, lambda_m0, nb_path, **kw):
        nb, dt, _ = set_time_grid(ttm=ttm, nb_steps_per_year=5 * 360)
        d = twin.hawkes_draws(SEED, 0, 0, n, state["step0"], nb)
        normals = iter([d["z"]])
        uniforms = iter([d["u_p"], d["u_m"]])
        exps = iter([d["e_p"], d["e_m"]])

        def normal(loc, scale, size):
            assert (loc, scale) == (0, 1) and tuple(size) == (nb, n)
            return next(normals)

        def uniform(low, high, size):
            assert tuple(size) == (nb, n)
            return next(uniforms)

        def exponential(scale, size):
            assert tuple(size) == (nb, n)
            return scale * next(exps)

        np.random.normal, np.random.uniform, np.random.exponential = normal, uniform, exponential
        try:
            out = orig[3](ttm=ttm, x0=x0, lambda_p0=lambda_p0, lambda_m0=lambda_m0, nb_path=nb_path, **kw)
        finally:
            np.random.normal, np.random.uniform, np.random.exponential = orig[:3]
        state["step0"] += nb
        state["states"].append(np.stack([a[:KEEP] for a in out]))
        return out

    hp.simulate_hawkesjd_terminal = simulate
    try:
        pr, sd = hp.hawkesjd_mc_chain_pricer(ttms=chain.ttms, forwards=chain.forwards, discfactors=chain.discfactors,
                                             strikes_ttms=chain.strikes_ttms, optiontypes_ttms=chain.optiontypes_ttms,
                                             nb_path=n, **params.to_dict())
    finally:
        hp.simulate_hawkesjd_terminal = orig[3]
    stats = {}
    twin.mc_chain(chain.ttms, chain.forwards, chain.discfactors, chain.strikes_ttms, chain.optiontypes_ttms,
                  {k: getattr(params, k) for k in twin.PARAM_NAMES}, n, SEED, stats=stats)
    print(name, "steps", state["step0"], "jumps", stats)
    save(name, **chain_arrays(chain), params=params_vec(params), seed=SEED, n_path=n, nb_steps_total=state["step0"],
         prices=np.concatenate([np.asarray(a) for a in pr]), stderrs=np.concatenate([np.asarray(a) for a in sd]),
         states=np.stack(state["states"]), jumps_p=stats["jumps_p"], jumps_m=stats["jumps_m"], jumps_both=stats["both"])


def g_analytic():
    chain = svm.get_btc_test_chain_data()
    p = hp.HawkesJDParams()
    kw = dict(model_params=p, ttms=chain.ttms, forwards=chain.forwards, discfactors=chain.discfactors,
              strikes_ttms=chain.strikes_ttms, optiontypes_ttms=chain.optiontypes_ttms)
    default = hp.hawkesjd_chain_pricer(**kw)
    orig = hp.solve_ivp

    def tight(*a, **k):
        k.setdefault("rtol", 1e-10)
        k.setdefault("atol", 1e-12)
        return orig(*a, **k)

    hp.solve_ivp = tight
    try:
        tight_prices = hp.hawkesjd_chain_pricer(**kw)
        vol_scaler = hp.set_vol_scaler(sigma0=p.sigma, ttm=np.min(chain.ttms))
        phi, psi, theta = mgfp.get_transform_var_grid(variable_type=VariableType.LOG_RETURN, max_phi=hp.MAX_PHI,
                                                      vol_scaler=vol_scaler)
        a1, lm1 = hp.compute_hawkes_a_mgf_grid(ttm=chain.ttms[0], phi_grid=phi, psi_grid=psi, model_params=p)
    finally:
        hp.solve_ivp = orig
    save("hawkes_analytic", **chain_arrays(chain), params=params_vec(p),
         prices_default=np.concatenate([np.asarray(a) for a in default]),
         prices_tight=np.concatenate([np.asarray(a) for a in tight_prices]), phi=phi, a1_tight=a1, log_mgf1_tight=lm1,
         compensators=np.array([p.compensator_p, p.compensator_m]), conds=np.array([p.jump1_cond, p.jump2_cond]),
         excited_params=params_vec(EXCITED), excited_compensators=np.array([EXCITED.compensator_p, EXCITED.compensator_m]),
         excited_conds=np.array([EXCITED.jump1_cond, EXCITED.jump2_cond]))


if __name__ == "__main__":
    g_mc("hawkes_mc", hp.HawkesJDParams())
    g_mc("hawkes_mc_excited", EXCITED)
    g_analytic()
