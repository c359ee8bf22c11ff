"""
Generate tests/golden/chain_sets_steps.npz: what the multi-set LogSV stepping kernels (logsv_chain_w_sets_kernel<P>,
logsv_chain_rng_sets_kernel<P>) leave in their snapshot rows -- x and qvar of every (set, expiry) -- in extended precision.
tests/test_chain_sets_widths_host.py holds the fp64 oracle to it, tests/test_gpu_chain_sets_steps.py the kernels.  CPU only, by hand:

    python tests/golden/make_golden_chain_sets_steps.py

The recursion is make_golden_mc_steps.truth_logsv (the reference's, 256-bit mpmath) and the random inputs are mc_steps_worker.normals
on the product's stream (seed, call 0), both imported; tests/golden/mc_steps.npz and its generator are not touched.  The chain and
the sets are those of tests/chain_sets_steps.py (its docstring says why every slice has the same dt and every set one eta: the
chain of a set is then one recursion and no state is rounded between the slices).  Each set starts where the sets entry starts it:
x = 0, qvar = 0, its own sigma0.

One case per (measure, set, slice): the cumulative x and qvar after that slice, in the file layout of mc_steps.npz (meta, hi,
lo_rel, fragile: make_golden_mc_steps.py's docstring), written by that generator's Book, so that mc_steps_worker.Fixture reads
it.  oracle_err is the fp64 C oracle's error against the truth, stepped slice by slice as an fp64 chain driver does; numpy_err its
NumPy restatement's.  The LogSV recursion takes no discrete decision: no path is fragile.  meta also records the random stream
version, the seed, the path count, the grid (nb_steps_per_year, ttms, steps, dt), the sets and the widths the device test runs.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_mc_steps as mk  # noqa: E402  (the recursion, the bookkeeping, the stream version)
import chain_sets_steps as cs  # noqa: E402
import mc_steps_worker as mw  # noqa: E402
from oracle import oracle  # noqa: E402

MAX_BYTES = 1_000_000


def main():
    oracle.build()
    from stochvolmodels_amd.utils.funcs import chain_step_grid
    nbs, dts = chain_step_grid(cs.TTMS, cs.SPY)
    assert tuple(nbs) == cs.STEPS and all(d == cs.DT for d in dts), (nbs, dts)
    sets = [cs.param_set(j) for j in range(cs.N_SETS)]
    W0, W1 = mw.normals(cs.SEED, cs.N, sum(cs.STEPS), 0, 0)
    snaps = tuple(int(s) for s in np.cumsum(cs.STEPS))
    book = mk.Book()

    class Grid:                                            # what chain_sets_steps.oracle_rows reads of a fixture
        steps, dt = cs.STEPS, cs.DT
    Grid.sets = sets

    for spot in (True, False):
        o = cs.oracle_rows(Grid, W0, W1, spot, range(cs.N_SETS))
        o2 = cs.oracle_rows(Grid, W0, W1, spot, range(cs.N_SETS), restatement=True)
        for q, p in enumerate(sets):
            start = mk.const_start(cs.N, 0.0, p["sigma0"], 0.0)
            tr, fr = mk.truth_logsv(start, cs.DT, p, p["eta"], spot, W0, W1, snaps)
            for i, s in enumerate(snaps):
                book.add(dict(id=cs.case_id(spot, q, i), gen="logsv", set=q, slice=i, spot=spot, steps=s, dt=cs.DT, eta=p["eta"],
                              seed=cs.SEED, scales=[1.0, p["theta"] ** 2 * s * cs.DT]),
                         [tr[s][0], tr[s][2]], (fr > 0) & (fr <= s), o[q, i], o2[q, i])
    meta = dict(rng_stream_version=mk.RNG_STREAM_VERSION, prec=mk.PREC, seed=cs.SEED, n=cs.N, spy=cs.SPY, ttms=list(cs.TTMS),
                steps=list(cs.STEPS), dt=cs.DT, sets=sets, widths=list(cs.WIDTHS), checksum=mw.checksum(W0, W1), cases=book.cases)
    np.savez_compressed(cs.FIXTURE, meta=np.array(json.dumps(meta)), hi=np.concatenate(book.hi), lo_rel=np.concatenate(book.lo),
                        fragile=np.packbits(np.concatenate(book.frag)))
    size = os.path.getsize(cs.FIXTURE)
    print(len(book.cases), "cases,", size, "bytes")
    assert size < MAX_BYTES, size


if __name__ == "__main__":
    main()
