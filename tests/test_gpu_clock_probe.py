"""
The in-kernel clock probe (svmc_clock_probe_arm / _read; bench.py's clock_mhz_in_kernel) on every launch route that passes it:
logsv_rng_launch, logsv_chain_rng_impl, logsv_chain_rng_sets (un-replayed), svmc_logsv_vol_paths (drawn and supplied) and
logsv_chain_rng_many (one job, and two jobs) -- the few-waves forms in this process, the full-launch forms in a child started with
SVMC_FEW_WAVES_MAX_PATHS=0 (tests/clock_probe_worker.py).  The probe's buffer belongs to the calling host thread and a launcher
hands it to its kernel as an argument: a launcher that looked at another copy of that per-thread state would pass null, nothing
would fail, and the bench would read zero stamps.  So per route: arm (a fresh, zeroed buffer), launch, read -- the first and the
last block must both have stamped a later exit than entry -- and disarm.
4096 paths, 8 steps per expiry, 2 expiries: more than one block in every form (8192 paths for the 1024-thread whole-chain kernels).
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROUTES = ["logsv_chain_rng_impl", "logsv_chain_rng_many", "logsv_chain_rng_many_two_jobs", "logsv_chain_rng_sets", "logsv_rng_launch",
          "svmc_logsv_vol_paths_drawn", "svmc_logsv_vol_paths_supplied"]
# the many-job launch with two jobs: each slot has two writers whose cycle counters are not comparable (csrc/svmc_block.h,
# clock_probe_stamp), so entry and exit of a slot are not ordered; the route is held to having stamped at that grid shape
TWO_JOBS = "logsv_chain_rng_many_two_jobs"
NOT_ARMED = "svmc_clock_probe_read: this thread has not armed the probe (svmc_clock_probe_arm)"


def check_stamps(got: dict) -> None:
    assert sorted(got) == ROUTES
    for route, st in got.items():
        assert len(st) == 8, route
        for which, (t_entry, r_entry, t_exit, r_exit) in (("first block", st[0:4]), ("last block", st[4:8])):
            print(route, which, t_entry, r_entry, t_exit, r_exit)
            assert t_entry != 0 and r_entry != 0 and t_exit != 0 and r_exit != 0, (route, which, st)
            if route != TWO_JOBS:
                assert t_exit > t_entry, (route, which, st)
                assert r_exit >= r_entry, (route, which, st)


def test_every_probed_route_stamps_first_and_last_block_few_waves_forms():
    import clock_probe_worker as w
    from stochvolmodels_amd import _lib
    check_stamps(w.stamps(False))
    rc, msg = w.read_after_disarm()
    assert rc == _lib.ERR_INVALID_ARGUMENT and msg == NOT_ARMED, (rc, msg)


def test_every_probed_route_stamps_first_and_last_block_full_launch_forms():
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "clock_probe_worker.py")
    r = subprocess.run([sys.executable, worker], env=dict(os.environ, SVMC_FEW_WAVES_MAX_PATHS="0"), capture_output=True, text=True,
                       timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, (r.returncode, r.stderr[-2000:])
    got = json.loads(lines[-1])
    check_stamps(got["stamps"])
    assert got["read_after_disarm"] == [1, NOT_ARMED], got["read_after_disarm"]
