"""Shared by tests/test_gpu_cmc_sens.py and its child process: the many-job conditional stepping kernels (svmc_logsv_chain_cmc_many /
svmc_heston_chain_cmc_many) and, per job, the single uniform-start call they must equal bit for bit.

As a program it is the worker of tests/test_gpu_cmc_sens.py::test_many_job_stepping_full_launch_form: the test starts it with
SVMC_FEW_WAVES_MAX_PATHS=0 (read once per process), so that every launch runs the FULL-LAUNCH kernels, and it writes the many-job
rows and the single calls' rows of both models to the .npz named on its command line:
    python tests/cmc_many_worker.py OUT.npz N_PATH"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# four slices of 3, 5, 8 and 6 steps: the first three of one dt (joined boundaries, and Philox calls of four steps straddled), the
# fourth of another
NB_STEPS = [3, 5, 8, 6]
DTS = [1.0 / 360.0, 1.0 / 360.0, 1.0 / 360.0, 1.0 / 300.0]
M = len(NB_STEPS)

# (parameter row, seed, call id): two jobs on one (seed, call id) with other parameters -- for LogSV also an eta != 1, which cuts that
# job's joined stretch --, jobs of equal parameters on other seeds, and the zero-noise set
LOGSV_A = [0.2, 0.22, 3.0, 12.0, -0.3, 0.4, 1.0, 1.0, 1.0, 1.0]
LOGSV_B = [0.35, 0.3, 2.0, 5.0, 0.2, 0.9, 1.0, 1.1, 1.0, 1.0]
LOGSV_ZERO = [0.3, 0.25, 1.5, 2.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0]
HESTON_A = [0.04, 0.04, 4.0, -0.5, 0.4]
HESTON_B = [0.09, 0.06, 2.0, 0.3, 0.8]
HESTON_ZERO = [0.05, 0.04, 3.0, 0.0, 0.0]          # volvol = 0 and rho = 0: the return has no noise of the driver either
JOBS = {"logsv": [(LOGSV_A, 11, 3), (LOGSV_B, 11, 3), (LOGSV_A, 12, 0), (LOGSV_A, 13, 0), (LOGSV_ZERO, 14, 1)],
        "heston": [(HESTON_A, 11, 3), (HESTON_B, 11, 3), (HESTON_A, 12, 0), (HESTON_A, 13, 0), (HESTON_ZERO, 14, 1)]}


def many_rows(eng, model, jobs):
    """[2][J][M][n]: every job's mu and cv rows from ONE many-job launch"""
    J, n = len(jobs), eng.n_path
    eng.chain_cmc_many(model, NB_STEPS, DTS, np.array([row for row, _, _ in jobs]), [s for _, s, _ in jobs], [c for _, _, c in jobs], 1)
    return eng.download(eng.snapshot_ptr(0), 2 * J * M * n).reshape(2, J, M, n)


def single_rows(eng, model, job):
    """[2][M][n]: the job alone through svmc_*_chain_cmc from the uniform start (0, 0, vol0, 0)"""
    row, seed, call_id = job
    n = eng.n_path
    eng.set_state_cmc(np.zeros(n), np.zeros(n), np.full(n, row[0]), np.zeros(n))
    if model == "logsv":
        eng.logsv_chain_cmc(NB_STEPS, DTS, row[6:], row[1], row[2], row[3], row[4], row[5], True, seed, call_id, 0)
    else:
        eng.heston_chain_cmc(NB_STEPS, DTS, row[1], row[2], row[3], row[4], seed, call_id, 0)
    return eng.download(eng.snapshot_ptr(0), 2 * M * n).reshape(2, M, n)


def run(n):
    """{model + "_many": [2][J][M][n], model + "_single": [J][2][M][n]}"""
    from stochvolmodels_amd.engine import HipEngine
    out = {}
    eng = HipEngine(n)
    try:
        for model, jobs in JOBS.items():
            out[model + "_many"] = many_rows(eng, model, jobs)
            out[model + "_single"] = np.stack([single_rows(eng, model, job) for job in jobs])
    finally:
        eng.close()
    return out


def main():
    assert os.environ.get("SVMC_FEW_WAVES_MAX_PATHS") == "0"
    np.savez(sys.argv[1], **run(int(sys.argv[2])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
