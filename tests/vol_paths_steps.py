"""Shared by tests/golden/make_golden_vol_paths_steps.py, tests/test_vol_paths_steps_host.py and
tests/test_gpu_vol_paths_steps.py: the case table of tests/golden/vol_paths_steps.npz, the increments of a case, the fixture's
reader, the fp64 oracle on a case, and the C-ABI driver of svmc_logsv_vol_paths (any ld / ldb, supplied increments or the device
draw).  checksum, measure, bound and ULP are tests/mc_steps_worker.py's."""
import ctypes as C
import json
import os

import numpy as np

import mc_steps_worker as mw
from oracle import oracle

FIXTURE = os.path.join(mw.HERE, "golden", "vol_paths_steps.npz")
DT = 1.0 / 360.0
N, LONG_N = 130, 64                                       # two waves and two lanes; one wave
SHORT_STEPS = (1, 2, 3, 7)                                # every row stored
ROWS_64 = (1, 2, 3, 4, 8, 16, 32, 63, 64)
LONG_STEPS = 1029                                         # 1030 rows: both loop forms end in a ragged tail (1029 = 4 x 257 + 1)
ROWS_LONG = (1, 2, 1023, 1024, 1025, 1026, 1027, 1028, 1029)
SEEDS = dict(ordinary=20271, long=20272, far=20273)
FAR_STARTS = {"div50": 1.0 / 50.0, "div1000": 1.0 / 1000.0, "x30": 30.0, "x300": 300.0}   # v0 / theta
STEP_CONSTANTS = ("kappa1", "kappa2", "theta", "beta", "volvol", "dt")
BOUND_GEN = dict(ordinary="logsv", long="logsv", far="far")    # whose MARGIN / FLOOR_ULPS of mc_steps_worker.py a group is held to


def plan(sets):
    """the table of the cases, as dicts without truth, for the generator; sets = make_golden_mc_steps.LOGSV_SETS (the tests read the
    cases from the file)"""
    out = []

    def add(group, sname, p, v0, spot, n, steps, rows, tag):
        out.append(dict(id=f"vp-{tag}-s{steps}", group=group, set=sname, params={k: p[k] for k in STEP_CONSTANTS[:-1]}, v0=v0,
                        spot=spot, n=n, steps=steps, dt=DT, seed=SEEDS[group], rows=list(rows)))

    for sname, spot in (("btc", True), ("btc", False), ("test", True)):
        p = sets[sname]
        for s in SHORT_STEPS:
            add("ordinary", sname, p, p["sigma0"], spot, N, s, range(1, s + 1), f"{sname}-{'spot' if spot else 'inv'}")
        add("ordinary", sname, p, p["sigma0"], spot, N, 64, ROWS_64, f"{sname}-{'spot' if spot else 'inv'}")
    p = sets["btc"]
    add("long", "btc", p, p["sigma0"], True, LONG_N, LONG_STEPS, ROWS_LONG, "btc-spot")
    for tag, f in FAR_STARTS.items():
        for s in SHORT_STEPS:
            add("far", "btc", p, p["theta"] * f, True, N, s, range(1, s + 1), f"far-{tag}")
    return out


def expected_ids():
    ids = [f"vp-{t}-s{s}" for t in ("btc-spot", "btc-inv", "test-spot") for s in SHORT_STEPS + (64,)]
    ids.append(f"vp-btc-spot-s{LONG_STEPS}")
    return ids, {tag: [f"vp-far-{tag}-s{s}" for s in SHORT_STEPS] for tag in FAR_STARTS}


def increments(case):
    """w[t][p] = fl(sqrt(dt) z[t][p]), z the stream-2 normal the device-draw route consumes at step t (word t & 3 of call t >> 2):
    the oracle's stream-2 pair of index t >> 1 holds words 2 (t >> 1 & 1), + 1 of that call, so z[t] is component t & 1 of it"""
    steps, n = case["steps"], case["n"]
    z0, z1 = oracle.fill_normals(case["seed"], n, (steps + 1) // 2, call_id=0, stream=2)
    z = np.empty((2 * z0.shape[0], n))
    z[0::2], z[1::2] = z0, z1
    return np.ascontiguousarray(np.sqrt(case["dt"]) * z[:steps])


def oracle_rows(case, w, scaled=None):
    """the case's stored rows [len(rows)][n] from the fp64 oracle on the increments w; scaled = (name, factor): that one step
    constant multiplied by factor (the mutation of tests/test_vol_paths_steps_host.py)"""
    p, dt = dict(case["params"]), case["dt"]
    if scaled is not None:
        name, f = scaled
        if name == "dt":
            dt = dt * f
        else:
            p[name] = p[name] * f
    with np.errstate(all="ignore"):
        sig = oracle.logsv_vol_paths(case["steps"], dt, case["v0"], p["theta"], p["kappa1"], p["kappa2"], p["beta"], p["volvol"],
                                     case["n"], is_spot_measure=case["spot"], brownians=w)
    return sig[case["rows"]]


class Fixture:
    def __init__(self, path=FIXTURE):
        g = np.load(path, allow_pickle=False)
        self.meta = json.loads(str(g["meta"]))
        self.cases = self.meta["cases"]
        self.by_id = {c["id"]: c for c in self.cases}
        self.hi = g["hi"]
        self.lo = g["lo_rel"].astype(np.float64) * np.abs(self.hi)      # the truth is the double pair hi + lo

    def truth(self, case):
        """(hi, lo), each [len(rows)][n]"""
        nr, n, off = len(case["rows"]), case["n"], case["off"]
        sl = slice(off, off + nr * n)
        return self.hi[sl].reshape(nr, n), self.lo[sl].reshape(nr, n)

    def error(self, case, rows):
        """|d / truth - 1|, the largest over the paths, per stored row (sigma > 0: no scale under the truth, no fragile paths)"""
        hi, lo = self.truth(case)
        return np.array(mw.measure(np.asarray(rows, dtype=np.float64), hi, lo, np.zeros(case["n"], dtype=bool), np.zeros(len(hi))))

    def bound(self, case):
        return mw.bound(case["oracle_err"], BOUND_GEN[case["group"]])


# ---- svmc_logsv_vol_paths through the C ABI -----------------------------------------------------------------------------------------
def upload(host):
    """a DeviceBuffer holding the doubles of `host`"""
    from stochvolmodels_amd import _lib
    from stochvolmodels_amd.engine import DeviceBuffer
    host = np.ascontiguousarray(host, dtype=np.float64)
    buf = DeviceBuffer(max(host.size, 1))
    _lib.check(_lib.load().svmc_memcpy_h2d(buf.ptr, host.ctypes.data, host.nbytes, None))
    _lib.check(_lib.load().svmc_stream_synchronize(None))
    return buf


def download(buf, n):
    from stochvolmodels_amd import _lib
    out = np.empty(int(n))
    _lib.check(_lib.load().svmc_memcpy_d2h(out.ctypes.data, buf.ptr, out.nbytes, None))
    _lib.check(_lib.load().svmc_stream_synchronize(None))
    return out


SENTINEL = -7.25


def device_vol_paths(n, steps, dt, v0, p, spot, w=None, seed=0, call_id=0, path_offset=0, ld=None, ldb=None):
    """svmc_logsv_vol_paths into a buffer prefilled with SENTINEL: the whole [(steps + 1)][ld] array as the device left it.
    w: the increments [steps][n] (uploaded with leading dimension ldb, its padding SENTINEL too), None: the device draw"""
    from stochvolmodels_amd import _lib
    ld = n if ld is None else ld
    ldb = n if ldb is None else ldb
    out = upload(np.full((steps + 1) * ld, SENTINEL))
    wb = None
    try:
        if w is not None:
            padded = np.full((steps, ldb), SENTINEL)
            padded[:, :n] = w
            wb = upload(padded)
        _lib.check(_lib.load().svmc_logsv_vol_paths(out.ptr, ld, n, steps, dt, v0, p["theta"], p["kappa1"], p["kappa2"], p["beta"],
                                                    p["volvol"], int(spot), None if wb is None else C.c_void_p(wb.ptr), ldb, seed,
                                                    call_id, path_offset, None))
        return download(out, (steps + 1) * ld).reshape(steps + 1, ld)
    finally:
        out.free()
        if wb is not None:
            wb.free()


def device_rows(case, form, w=None):
    """the case's stored rows from the device: form "w" on the uploaded increments, "rng" on the device draw at the case's seed"""
    sig = device_vol_paths(case["n"], case["steps"], case["dt"], case["v0"], case["params"], case["spot"],
                           w=w if form == "w" else None, seed=case["seed"])
    assert np.all(sig[0] == case["v0"])
    return sig[case["rows"]]
