"""
Generate tests/golden/cmc_steps.npz: the terminal states (mu, cv, sigma | v, qvar) of the conditional Monte Carlo step recursions
in extended precision, the truth that tests/test_cmc_host.py holds the NumPy restatement to and tests/test_gpu_cmc.py the stepping
kernels of csrc/svmc_cmc.hip.  CPU only, by hand:

    python tests/golden/make_golden_cmc.py

Everything is evaluated in mpmath at 256 bits (tests/cmc_twin.py mp_logsv / mp_heston: the REFERENCE's step as the reference writes
it, with the volatility's driver substituted) on the product's own random stream, tag 8 (cmc_twin.normals: one normal per step,
word step & 3 of Philox call step >> 2).

Cases: LogSV sets "btc" and "test" and Heston sets "base" and "btc" of make_golden_mc_steps.py, a LogSV set with beta = volvol = 0
and a Heston set with rho = -1; N = 130 paths (two waves and two lanes), step counts 1, 2, 3, 4, 5, 7, 8, 9, 64 at step offsets 0,
1, 2, 3 (every phase of the four-steps-per-call layout at a slice's start, and every phase at its end), and one 1024-step case on
64 paths per model.  Spot measure, eta = 1, dt = 1 / 360, start (0, 0, sigma0 | v0, 0).

File layout: that of mc_steps.npz (make_golden_mc_steps.py: meta / hi / lo_rel / fragile); nq = 4 quantities per case in the order
mu, cv, state, qvar.  `oracle_err` is the NumPy restatement's (cmc_twin.np_logsv / np_heston) own error against the truth in
mc_steps_worker.measure's measure, the yardstick of the device bound.  Scales: 1 for mu; theta^2 T (LogSV) / theta T (Heston) for
cv and qvar; sigma0 / theta for the state.  Heston paths whose new variance comes within 1e-9 relative of the floor at some step
are fragile and left out; at most 1 % of a case's paths may be (asserted here).
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
sys.path.insert(0, HERE)

import cmc_twin as ct  # noqa: E402
from make_golden_mc_steps import (FRAGILE_REL, HESTON_SETS, LOGSV_SETS, MAX_BYTES, MAX_FRAGILE_SHARE, PREC, RNG_STREAM_VERSION,  # noqa: E402
                                  Book)
from mc_steps_worker import checksum  # noqa: E402

mp.mp.prec = PREC
N = 130
STEPS = (1, 2, 3, 4, 5, 7, 8, 9, 64)
OFFSETS = (0, 1, 2, 3)
LONG_STEPS, LONG_N = 1024, 64
DT = 1.0 / 360.0
SEEDS = dict(logsv=20271, heston=20272)
LOGSV = dict(LOGSV_SETS, zero=dict(LOGSV_SETS["test"], beta=0.0, volvol=0.0))
HESTON = dict(HESTON_SETS, rho_m1=dict(HESTON_SETS["base"], rho=-1.0))
LONG_SET = dict(logsv="btc", heston="btc")


def plan(sname, gen):
    runs = [(N, off, STEPS) for off in OFFSETS]
    if sname == LONG_SET[gen]:
        runs.append((LONG_N, 0, (LONG_STEPS,)))
    return runs


def build():
    book = Book()
    for gen, sets in (("logsv", LOGSV), ("heston", HESTON)):
        seed = SEEDS[gen]
        for sname, p in sets.items():
            vol0 = p["sigma0"] if gen == "logsv" else p["v0"]
            for n, off, snaps in plan(sname, gen):
                B = ct.normals(seed, n, max(snaps), off)
                st = [np.zeros(n), np.zeros(n), np.full(n, vol0), np.zeros(n)]
                if gen == "logsv":
                    tr, fr = ct.mp_logsv(mp, st, DT, p, 1.0, True, B, snaps)
                else:
                    tr, fr = ct.mp_heston(mp, st, DT, p, B, snaps, FRAGILE_REL)
                for s in snaps:
                    T = s * DT
                    if gen == "logsv":
                        o = ct.np_logsv(st, DT, p, 1.0, True, B[:s])
                        scales = [1.0, p["theta"] ** 2 * T, p["sigma0"], p["theta"] ** 2 * T]
                    else:
                        o = ct.np_heston(st, DT, p, B[:s])
                        scales = [1.0, p["theta"] * T, p["theta"], p["theta"] * T]
                    book.add(dict(id=f"{gen}-{sname}-s{s}-o{off}", gen=gen, set=sname, params=p, eta=1.0, spot=True, steps=s, dt=DT,
                                  offset=off, seed=seed, start=[0.0, 0.0, vol0, 0.0], scales=scales, checksum=checksum(B[:s])),
                             tr[s], (fr > 0) & (fr <= s), np.stack(o))
    return book


def main():
    book = build()
    meta = dict(rng_stream_version=RNG_STREAM_VERSION, stream_tag=ct.TAG, prec=PREC, fragile_rel=FRAGILE_REL,
                max_fragile_share=MAX_FRAGILE_SHARE, cases=book.cases)
    path = os.path.join(HERE, "cmc_steps.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), hi=np.concatenate(book.hi), lo_rel=np.concatenate(book.lo),
                        fragile=np.packbits(np.concatenate(book.frag)))
    size = os.path.getsize(path)
    print(len(book.cases), "cases,", size, "bytes")
    assert size < MAX_BYTES, size


if __name__ == "__main__":
    main()
