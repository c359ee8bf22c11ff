"""the routes of tests/test_gpu_clock_probe.py, and its worker: every launcher that passes the calling thread's armed clock probe
(svmc_clock_probe_arm / _read) to its kernel, driven through the engine and pricer calls.  The test runs stamps() in its own
process -- at these sizes the few-waves forms of the generators -- and starts this file with SVMC_FEW_WAVES_MAX_PATHS=0 (read
once per process) for the full-launch forms; as a program it prints one JSON line {route: [8 stamps]} plus the status and
message of a read after the final disarm."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import stochvolmodels_amd as sv  # noqa: E402
from stochvolmodels_amd import _lib  # noqa: E402
from stochvolmodels_amd.engine import get_engine, marshalled_chain, option_type_codes  # noqa: E402

N = 4096                               # 16 blocks of the few-waves forms, 8 of logsv_rng_kernel, 16 / 4 of the volatility paths
N_CHAIN_BLOCK = 8192                   # the 1024-thread whole-chain kernels (full-launch chain and many-job routes): 8 blocks
STEPS = 8                              # per expiry
SPY = 75                               # int(0.1 * 75) + 1 = 8 steps for each of the two expiries
TTMS = np.array([0.1, 0.2])
FW, DF = np.array([1.0, 1.01]), np.array([0.99, 0.98])
STRIKES = [np.array([0.9, 1.0, 1.1])] * 2
TYPES = [np.array(["P", "C", "C"])] * 2


def routes(full_launch: bool):
    """{route: (launch, stream getter)}: launch() queues (or runs) the route's stepping launch once"""
    P = sv.LOGSV_BTC_PARAMS
    n_chain = N_CHAIN_BLOCK if full_launch else N
    model = (P.theta, P.kappa1, P.kappa2, P.beta, P.volvol)
    codes = [option_type_codes(t) for t in TYPES]

    def slice_rng():
        eng = get_engine(N)
        eng.fill_state(0.0, P.sigma0, 0.0)
        eng.logsv_rng(STEPS, 0.1 / STEPS, *model, 1.0, True, 11, 0, 0)
        return eng.stream

    def chain_rng():
        eng = get_engine(n_chain)
        eng.reserve_snapshots(4)
        spot, _keep = eng.alloc_sums(4, "clock_probe_spot")
        eng.logsv_chain_rng([STEPS, STEPS], [0.1 / STEPS] * 2, [1.0, 1.0], FW, *model, True, 11, 0, 0, True, spot,
                            start=(0.0, P.sigma0, 0.0))
        return eng.stream

    def chain_rng_sets():
        res = sv.draw_fixed_randoms_on_device(TTMS, nb_path=N, nb_steps_per_year=SPY, seed=11)
        try:                           # un-replayed: a captured launch never carries the probe
            res.price_logsv_chain(TTMS, FW, DF, STRIKES, codes, P.sigma0, *model, np.ones(2), True, 1, use_graph=False)
        finally:
            res.free()
        return None

    def vol_paths(supplied: bool):
        eng = get_engine(N)
        b = np.random.default_rng(3).standard_normal((STEPS, N)) * np.sqrt(0.1 / STEPS) if supplied else None
        eng.logsv_vol_paths(STEPS, 0.1 / STEPS, P.sigma0, *model, True, 11, 0, brownians=b)
        return eng.stream

    def chain_rng_many(n_jobs: int):
        eng = get_engine(n_chain)
        ch = marshalled_chain(TTMS, FW, DF, STRIKES, codes)
        # the many-job grid is (path blocks, jobs) and a block stamps by its blockIdx.x alone (csrc/svmc_block.h): ONE job gives each
        # slot one writer, and entry and exit can be compared; with two jobs a slot has two writers on different XCDs, whose cycle
        # counters are not comparable, so that route is only held to having stamped (TWO_JOBS in the test)
        rows = np.array([[(1.0 + 0.1 * j) * P.sigma0, *model, 1.0, 1.0] for j in range(n_jobs)])
        eng.price_chain_many_fused(ch, "logsv", rows, [11 + j for j in range(n_jobs)], [0] * n_jobs, 1, SPY, 1)
        return eng.stream

    return {"logsv_rng_launch": slice_rng, "logsv_chain_rng_impl": chain_rng, "logsv_chain_rng_sets": chain_rng_sets,
            "svmc_logsv_vol_paths_drawn": lambda: vol_paths(False), "svmc_logsv_vol_paths_supplied": lambda: vol_paths(True),
            "logsv_chain_rng_many": lambda: chain_rng_many(1), "logsv_chain_rng_many_two_jobs": lambda: chain_rng_many(2)}


def stamps(full_launch: bool) -> dict:
    """per route: arm (a fresh zeroed buffer), launch, read the 8 stamps, disarm"""
    L = _lib.load()
    out = {}
    for name, launch in routes(full_launch).items():
        _lib.check(L.svmc_clock_probe_arm(1))
        try:
            stream = launch()
            st = (C.c_uint64 * 8)()
            _lib.check(L.svmc_clock_probe_read(st, stream))
            out[name] = [int(v) for v in st]
        finally:
            _lib.check(L.svmc_clock_probe_arm(0))
    return out


def read_after_disarm():
    """(status, message) of svmc_clock_probe_read on a thread whose probe is not armed"""
    L = _lib.load()
    st = (C.c_uint64 * 8)()
    rc = L.svmc_clock_probe_read(st, None)
    return int(rc), L.svmc_last_error().decode("utf-8", "replace")


def main():
    assert os.environ.get("SVMC_FEW_WAVES_MAX_PATHS") == "0"
    out = {"stamps": stamps(True)}
    out["read_after_disarm"] = list(read_after_disarm())
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
