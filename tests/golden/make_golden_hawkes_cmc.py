"""
Generate tests/golden/hawkes_cmc_steps.npz: the conditional Monte Carlo step recursion of the Hawkes jump-diffusion (DESIGN.md
row f16) in extended precision, the truth that tests/test_hawkes_cmc_host.py holds the NumPy twin to and that a device test is to
hold a stepping kernel to.  CPU only, by hand (about two minutes):

    python tests/golden/make_golden_hawkes_cmc.py

Everything is evaluated in mpmath at PREC = 256 bits from the double parameters and the twin's draws on streams 9 and 10
(hawkes_cmc_twin.draws, converted exactly), as make_golden_mc_steps.py does for the plain Hawkes step.

A run is (parameter set, step offset): ONE chain of six slices of 1, 2, 3, 7, 64 and 451 steps -- odd and even counts, so that
slice boundaries fall both on and inside a Philox call of stream 9, which carries two steps -- on 700 paths from the origin
(0, lambda_p, lambda_m).  A case is (run, expiry); the path counts 1, 63, 64, 65, 513, 700 are prefixes of the run's paths (a path's
draws depend on its index alone), and the twin's error is stored for each.

File layout (tests/mc_steps_worker.py Fixture reads it):
    meta          JSON: rng_stream_version, stream_tags, prec, path_counts, steps, dts, and `cases`: per case id, set, params, offset,
                  expiry, steps (of its slice), end (chain-local steps up to it), n = 700, nq = 3, scales, off / foff (offsets of its
                  3 x n block in hi / lo_rel and of its n flags in `fragile`), checksum (sha256 of the run's draws), and per path
                  count: oracle_err_n [3] (the twin's error over the first n paths), jumped_n [2] (paths among the first n that
                  jumped on each side within the slice), fragile_n (fragile paths among the first n)
    hi, lo_rel    the truth (mu, lambda_p, lambda_m) as the double pair hi + lo, lo = lo_rel |hi| with lo_rel in float32
    fragile       per path: a jump test came within FRAGILE_REL relative of its threshold at some step up to the expiry; such
                  paths are left out of every comparison

Enforced here and recorded: every case of at least 64 paths whose slice has at least 64 steps has jumps on both sides; at most one
path of a case is fragile (none is expected).
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

import hawkes_cmc_twin as hc  # noqa: E402
import hawkes_twin as ht  # noqa: E402
from mc_steps_worker import checksum, measure  # noqa: E402

PREC = 256
mp.mp.prec = PREC
RNG_STREAM_VERSION = 4
FRAGILE_REL = 1e-9
SEED = 20267
N = 700
PATH_COUNTS = (1, 63, 64, 65, 513, 700)
STEPS = (1, 2, 3, 7, 64, 451)
DTS = (0.02, 0.015, 0.02, 0.01, 0.02, 0.02)
OFFSETS = (0, 1)
SETS = ("hawkes_mc", "hawkes_mc_excited")
MAX_BYTES = 1_000_000


def main():
    cases, his, los, frags = [], [], [], []
    off = foff = 0
    for sname in SETS:
        p = dict(zip(ht.PARAM_NAMES, (float(v) for v in np.load(os.path.join(HERE, sname + ".npz"))["params"])))
        scales = [1.0, p["theta_p"], p["theta_m"]]
        for offset in OFFSETS:
            truth, fragile, jumps = hc.mp_chain(mp, p, SEED, N, STEPS, DTS, offset, FRAGILE_REL)
            twin = hc.np_chain(p, SEED, N, STEPS, DTS, offset)
            d = hc.draws(SEED, N, sum(STEPS), offset)
            cs = checksum(*[d[k] for k in ("u_p", "u_m", "v_p", "v_m")])
            for i, steps in enumerate(STEPS):
                hi = np.array([[float(v) for v in row] for row in truth[i]])
                lo = np.array([[float(v - mp.mpf(float(h))) for v, h in zip(row, hrow)] for row, hrow in zip(truth[i], hi)])
                assert np.all(np.isfinite(hi))
                with np.errstate(all="ignore"):
                    lo32 = np.where(hi != 0.0, lo / np.abs(hi), 0.0).astype(np.float32)
                assert np.all(lo[hi == 0.0] == 0.0)
                lo = lo32.astype(np.float64) * np.abs(hi)                     # as the Fixture rebuilds it
                state = np.stack(twin[i])
                meta = dict(id=f"{sname}-o{offset}-e{i}", gen="hawkes", set=sname, params=p, offset=offset, expiry=i, steps=steps,
                            end=int(sum(STEPS[:i + 1])), n=N, nq=3, scales=scales, off=off, foff=foff, seed=SEED, checksum=cs,
                            fragile_paths=int(fragile[i].sum()), oracle_err_n={}, jumped_n={}, fragile_n={})
                assert meta["fragile_paths"] <= 1, (meta["id"], meta["fragile_paths"])
                for n in PATH_COUNTS:
                    meta["oracle_err_n"][str(n)] = measure(state[:, :n], hi[:, :n], lo[:, :n], fragile[i, :n], scales)
                    jumped = [int(np.count_nonzero(jumps[i, k, :n])) for k in (0, 1)]
                    meta["jumped_n"][str(n)] = jumped
                    meta["fragile_n"][str(n)] = int(fragile[i, :n].sum())
                    assert n < 64 or steps < 64 or min(jumped) >= 1, (meta["id"], n, jumped)
                meta["oracle_err"] = meta["oracle_err_n"][str(N)]
                cases.append(meta)
                his.append(hi.ravel()), los.append(lo32.ravel()), frags.append(fragile[i].copy())
                off += 3 * N
                foff += N
                print(meta["id"], "fragile", meta["fragile_paths"], "jumped", meta["jumped_n"][str(N)], "twin err",
                      ["%.2e" % e for e in meta["oracle_err"]], flush=True)
    meta = dict(rng_stream_version=RNG_STREAM_VERSION, stream_tags=[hc.UNIFORM_TAG, hc.JUMP_TAG], prec=PREC, fragile_rel=FRAGILE_REL,
                max_fragile_paths=1, path_counts=list(PATH_COUNTS), steps=list(STEPS), dts=list(DTS), offsets=list(OFFSETS), cases=cases)
    np.savez_compressed(hc.FIXTURE, meta=np.array(json.dumps(meta)), hi=np.concatenate(his), lo_rel=np.concatenate(los),
                        fragile=np.packbits(np.concatenate(frags)))
    size = os.path.getsize(hc.FIXTURE)
    print(len(cases), "cases,", size, "bytes")
    assert size < MAX_BYTES, size


if __name__ == "__main__":
    main()
