"""Shared by tests/test_gpu_cmc.py and its child process: the conditional stepping kernels driven through the C ABI
(svmc_logsv_chain_cmc / svmc_heston_chain_cmc) on the cases of tests/golden/cmc_steps.npz.

As a program it is the worker of tests/test_gpu_cmc.py::test_full_launch_form: the test starts it with SVMC_FEW_WAVES_MAX_PATHS=0
(read once per process), so that the launches run the FULL-LAUNCH kernels at the fixture's 130 and 64 paths, and it writes the
terminal states of every case to the .npz named on its command line:  python tests/cmc_steps_worker.py OUT.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cmc_twin as ct  # noqa: E402
import mc_steps_worker as mw  # noqa: E402


def step_chain(eng, case, nb_steps, offset):
    """the case's model through one chain call of len(nb_steps) slices from the engine's resident state"""
    p, dt, seed = case["params"], case["dt"], case["seed"]
    m = len(nb_steps)
    if case["gen"] == "logsv":
        eng.logsv_chain_cmc(nb_steps, [dt] * m, [case["eta"]] * m, p["theta"], p["kappa1"], p["kappa2"], p["beta"], p["volvol"],
                            case["spot"], seed, 0, offset)
    else:
        eng.heston_chain_cmc(nb_steps, [dt] * m, p["theta"], p["kappa"], p["rho"], p["volvol"], seed, 0, offset)


def device_state(eng, fx, case):
    """[4][n]: (mu, cv, state, qvar) after the case's steps"""
    eng.set_state_cmc(*fx.start(case))
    step_chain(eng, case, [case["steps"]], case["offset"])
    return np.stack(eng.get_state_cmc())


def run_cases(fx, cases):
    from stochvolmodels_amd.engine import HipEngine
    engines, out = {}, {}
    try:
        for case in cases:
            eng = engines.get(case["n"])
            if eng is None:
                eng = engines[case["n"]] = HipEngine(case["n"])
            out[case["id"]] = device_state(eng, fx, case)
    finally:
        for eng in engines.values():
            eng.close()
    return out


def main():
    assert os.environ.get("SVMC_FEW_WAVES_MAX_PATHS") == "0"
    fx = mw.Fixture(ct.FIXTURE)
    np.savez(sys.argv[1], **run_cases(fx, fx.cases))
    return 0


if __name__ == "__main__":
    sys.exit(main())
