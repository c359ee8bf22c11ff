"""
Generate tests/golden/vol_paths_steps.npz: the LogSV volatility paths of simulate_vol_paths in extended precision, the truth that
tests/test_vol_paths_steps_host.py holds the fp64 CPU oracle to and tests/test_gpu_vol_paths_steps.py logsv_vol_paths_kernel in both
of its loop forms.  CPU only, by hand:

    python tests/golden/make_golden_vol_paths_steps.py

What is evaluated is the REFERENCE's recursion as oracle/svmc_oracle.c:svo_logsv_vol_paths states it
(pricers/logsv_pricer.py:930-945), in mpmath at PREC = 256 bits from the double parameters and the double increments w (converted
exactly) -- not the kernel's regrouping (ln sigma in units of ln 2 / 256, four FMAs on host-scaled constants, Newton reciprocal,
table exponential):

    L = ln v0 once;  L += (k1 theta / s - k1 + k2 (theta - s) + adj s - vartheta^2 / 2) dt + vartheta w;  s = exp(L)
    adj = 0 (spot measure) | beta (inverse measure), vartheta = sqrt(beta^2 + volvol^2)

The increments are the product's own stream (version RNG_STREAM_VERSION, recorded): for a case with seed S, w[t] = fl(sqrt(dt) z[t])
with z the stream-2 normal the oracle's device-draw route consumes at step t (word t & 3 of call t >> 2).  One truth then serves
both forms of the kernel: these arrays uploaded as `brownians`, and the device draw at seed S.  The device draw multiplies z by the
UNROUNDED vartheta sqrt(dt) K where the truth's input is the rounded product w: the two differ by that one rounding of w (2^-53 of
vartheta w, a term of about 0.1 in ln sigma -- 1e-17 per step), which the bound's floor covers many times over.

Cases (tests/vol_paths_steps.py:plan; dt = 1/360):
    ordinary   btc spot, btc inverse, test spot of LOGSV_SETS; 130 paths (two waves and two lanes); 1, 2, 3, 7 steps with every
               row stored, 64 steps with rows 1, 2, 3, 4, 8, 16, 32, 63, 64
    long       btc spot, 64 paths, 1029 steps (1030 rows: the drawing loop ends in a partial call, the supplied-increments loop in
               a ragged tail), rows 1, 2, 1023 .. 1029
    far        btc spot from the scalar v0 = theta / 50, theta / 1000, 30 theta, 300 theta (this kernel starts every path from
               v0); 130 paths; 1, 2, 3, 7 steps, every row.  A far start whose truth is not finite in double is dropped, with a
               line in the output.

File layout (make_golden_mc_steps.py's):
    meta          JSON: rng_stream_version, prec, and `cases`: per case id, group, set, params, v0, spot, n, steps, dt, seed, rows
                  (the stored time indices), off (offset of the case's len(rows) x n block in hi / lo_rel), checksum (sha256 of
                  the increments) and oracle_err [len(rows)]
    hi, lo_rel    the truth as the double pair hi + lo: hi the nearest double, lo = truth - hi = lo_rel |hi|, lo_rel in float32

oracle_err is the yardstick: the fp64 oracle's own relative error |d / truth - 1| against the truth, the largest over the paths,
per stored row.  sigma > 0, and the scheme has no discrete decision: no scale under the truth, no fragile paths.
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vol_paths_steps as vp  # noqa: E402  (shared with the tests)
from make_golden_mc_steps import LOGSV_SETS, MAX_BYTES, PREC, RNG_STREAM_VERSION  # noqa: E402
from mc_steps_worker import checksum, measure  # noqa: E402
from oracle import oracle  # noqa: E402

mp.mp.prec = PREC
F = mp.mpf


def truth_vol_paths(case, w):
    """rows 1 .. steps of every path: [steps][n] of mpf"""
    p = case["params"]
    dt = F(case["dt"])
    theta, k1, k2, beta, volvol = (F(p[k]) for k in ("theta", "kappa1", "kappa2", "beta", "volvol"))
    adj = F(0) if case["spot"] else beta
    vartheta2 = beta * beta + volvol * volvol
    vartheta = mp.sqrt(vartheta2)
    steps, n = w.shape
    out = [[None] * n for _ in range(steps)]
    for j in range(n):
        s = F(case["v0"])
        L = mp.log(s)
        for t in range(steps):
            L = L + (k1 * theta / s - k1 + k2 * (theta - s) + adj * s - vartheta2 / 2) * dt + vartheta * F(float(w[t, j]))
            s = mp.exp(L)
            out[t][j] = s
    return out


def main():
    oracle.build()
    cases, his, los, off = [], [], [], 0
    memo = {}                                               # the 1-, 2-, 3-, 7-step cases are prefixes of their 64-step run
    for case in vp.plan(LOGSV_SETS):
        w = vp.increments(case)
        # the increments ARE the device-draw route's: the oracle on them equals the oracle drawing for itself, bit for bit
        p = case["params"]
        drawn = oracle.logsv_vol_paths(case["steps"], case["dt"], case["v0"], p["theta"], p["kappa1"], p["kappa2"], p["beta"],
                                       p["volvol"], case["n"], is_spot_measure=case["spot"], seed=case["seed"])
        assert np.array_equal(drawn[case["rows"]], vp.oracle_rows(case, w)), case["id"]
        key = (case["set"], case["spot"], case["v0"], case["n"], case["seed"])
        if key not in memo or len(memo[key]) < case["steps"]:
            try:
                memo[key] = truth_vol_paths(case, w)
            except OverflowError:
                memo[key] = None
        tr = memo[key]
        rows = None if tr is None else [tr[t - 1] for t in case["rows"]]
        hi = None if rows is None else np.array([[float(v) for v in r] for r in rows])
        if hi is None or not (np.all(np.isfinite(hi)) and np.all(hi > 0.0)):
            assert case["group"] == "far", case["id"]       # every other truth is finite in double
            print("DROPPED", case["id"], "its truth is not finite in double", flush=True)
            continue
        lo = np.array([[float(v - F(float(h))) for v, h in zip(r, hr)] for r, hr in zip(rows, hi)])
        lo32 = (lo / np.abs(hi)).astype(np.float32)
        lo = lo32.astype(np.float64) * np.abs(hi)           # as the Fixture rebuilds it
        err = measure(vp.oracle_rows(case, w), hi, lo, np.zeros(case["n"], dtype=bool), np.zeros(len(hi)))
        assert np.all(np.isfinite(err)), case["id"]
        cases.append(dict(case, off=off, checksum=checksum(w), oracle_err=err))
        his.append(hi.ravel()), los.append(lo32.ravel())
        off += hi.size
        print(case["id"], "oracle_err", " ".join("%.2e" % e for e in err), flush=True)
    meta = dict(rng_stream_version=RNG_STREAM_VERSION, prec=PREC, cases=cases)
    np.savez_compressed(vp.FIXTURE, meta=np.array(json.dumps(meta)), hi=np.concatenate(his), lo_rel=np.concatenate(los))
    size = os.path.getsize(vp.FIXTURE)
    print(len(cases), "cases,", size, "bytes")
    assert size < MAX_BYTES, size


if __name__ == "__main__":
    main()
