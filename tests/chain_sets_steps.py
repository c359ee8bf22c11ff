"""Shared by tests/golden/make_golden_chain_sets_steps.py, tests/test_chain_sets_widths_host.py, tests/test_gpu_chain_sets_steps.py
and tests/test_gpu_chain_sets_widths.py: the cases of tests/golden/chain_sets_steps.npz (the multi-set LogSV stepping kernels'
snapshot rows in 256-bit arithmetic), the fp64 oracle on them, and the read-only helper that finds the snapshot rows of a C-ABI
session.

The chain.  Slices of 1, 2, 5 and 40 steps at nb_steps_per_year = 505 with expiries at 1, 3, 8 and 48 times 2^-9: every gap is
a multiple of 2^-9 that the drivers' rule int(gap x 505) + 1 cuts into that many steps, and gap / steps is 2^-9 EXACTLY for every
slice.  One dt and one vol-backbone eta per set make the chain of a set ONE recursion of 48 steps whose states after 1, 3, 8 and
48 steps are the snapshot rows -- which is what make_golden_mc_steps.truth_logsv evaluates, with no state rounded to a double
between the slices.  (Constants that differ from slice to slice are the bit contracts' business: tests/test_gpu_chain_sets_widths.py.)

The sets.  Eight parameter sets that differ in all six model parameters; the odd ones carry a backbone eta off 1.  The truth of a
set does not depend on its company, so a width-w case is the sets 0 .. w - 1 and the widths 4, 7 and 8 share their truths.
"""
import ctypes as C
import os

import numpy as np

import mc_steps_worker as mw

FIXTURE = os.path.join(mw.HERE, "golden", "chain_sets_steps.npz")
SEED = 20267
N = 130
SPY = 505
STEPS = (1, 2, 5, 40)
DT = 2.0 ** -9
TTMS = tuple(float(s) * DT for s in np.cumsum(STEPS))
WIDTHS = (4, 7, 8)
N_SETS = 8
PARAM_NAMES = ("sigma0", "theta", "kappa1", "kappa2", "beta", "volvol")


def param_set(j):
    """set j of the family the bit contracts of tests/test_gpu_parity.py use, with a constant backbone eta on the odd sets"""
    return dict(sigma0=0.8 + 0.02 * j, theta=1.0 + 0.01 * j, kappa1=3.0 + 0.1 * j, kappa2=3.0 - 0.1 * j, beta=0.15 - 0.03 * j,
                volvol=1.8 - 0.05 * j, eta=1.0 if j % 2 == 0 else 0.7 + 0.05 * j)


def case_id(spot, q, i):
    return f"{'spot' if spot else 'inv'}-set{q}-slice{i}"


class Fixture(mw.Fixture):
    def __init__(self, path=FIXTURE):
        super().__init__(path)
        m = self.meta
        self.sets, self.steps, self.ttms, self.dt, self.spy, self.seed, self.n = (m[k] for k in ("sets", "steps", "ttms", "dt", "spy",
                                                                                                 "seed", "n"))

    def normals(self):
        """(W0, W1) [48][n] of the stream (seed, call 0) and their checksum"""
        W0, W1 = mw.normals(self.seed, self.n, sum(self.steps), 0, 0)
        return W0, W1, mw.checksum(W0, W1)

    def errors(self, spot, rows, sets=None):
        """rows [P][m][2][n] (x, qvar of set q after slice i) -> (gpu_err [P][m][2], oracle_err [P][m][2]) in mc_steps_worker.measure"""
        sets = range(len(rows)) if sets is None else sets
        cases = [[self.by_id[case_id(spot, q, i)] for i in range(len(self.steps))] for q in sets]
        err = np.array([[self.error(c, r) for c, r in zip(cs, rs)] for cs, rs in zip(cases, rows)])
        return err, np.array([[c["oracle_err"] for c in cs] for cs in cases])


def oracle_rows(fx, W0, W1, spot, sets, restatement=False, scaled=None):
    """the snapshot rows [len(sets)][m][2][n] from the fp64 oracle (restatement=True: its NumPy restatement), slice by slice from
    the sets entry's start state (0, sigma0, 0) as an fp64 chain driver carries it.  scaled = (q, name, factor): that one step
    constant of set q multiplied by factor (name: a model parameter, "eta" or "dt")"""
    from oracle import oracle
    fn = oracle.np_logsv_terminal_w if restatement else oracle.logsv_terminal_w
    n = W0.shape[1]
    out = np.empty((len(sets), len(fx.steps), 2, n))
    for k, q in enumerate(sets):
        p = dict(fx.sets[q])
        dt = fx.dt
        if scaled is not None and scaled[0] == q:
            if scaled[1] == "dt":
                dt = dt * scaled[2]
            else:
                p[scaled[1]] = p[scaled[1]] * scaled[2]
        x, s, v = np.zeros(n), np.full(n, p["sigma0"]), np.zeros(n)
        t0 = 0
        for i, nb in enumerate(fx.steps):
            with np.errstate(all="ignore"):
                x, s, v = fn(x, s, v, dt, p["theta"], p["kappa1"], p["kappa2"], p["beta"], p["volvol"], W0[t0:t0 + nb], W1[t0:t0 + nb],
                             eta=p["eta"], is_spot_measure=spot)
            out[k, i, 0], out[k, i, 1] = x, v
            t0 += nb
    return out


# ---- where a session keeps its snapshot rows ------------------------------------------------------------------------------------
SESSION_SCAN_BYTES = 1536


def session_snapshot_ptr(session, n_path, max_expiries, max_strikes):
    """the device address of the snapshot rows of a svmc_session_t that was created for (n_path, max_expiries, max_strikes).

    READ-ONLY, and for tests alone.  The C ABI keeps a session opaque and hands out its results, not its rows; the multi-set
    drivers leave x (and qvar) of every (set, expiry) in those rows and nowhere else.  The session object (struct Session of
    csrc/svmc_chain.hip) holds the three sizes it was created with side by side -- size_t n_path, int max_expiries, size_t
    max_strikes -- followed by the device pointers x, vol, qvar, snap.  The head of the object is searched for that triple, which
    must occur exactly once; a layout that no longer has it fails here, loudly, and not in a kernel."""
    addr = session.value if isinstance(session, C.c_void_p) else int(session)
    assert addr
    w = np.frombuffer(C.string_at(addr, SESSION_SCAN_BYTES), dtype=np.uint64)
    hits = [k for k in range(w.size - 6) if int(w[k]) == int(n_path) and int(w[k + 1]) & 0xFFFFFFFF == int(max_expiries)
            and int(w[k + 2]) == int(max_strikes)]
    assert len(hits) == 1, f"struct Session: (n_path, max_expiries, max_strikes) found {len(hits)} times in the object's head"
    x, vol, qvar, snap = (int(v) for v in w[hits[0] + 3:hits[0] + 7])
    assert len({x, vol, qvar, snap}) == 4 and all((x, vol, qvar, snap)), "struct Session: the pointers after the sizes are not four"
    return snap, (x, vol, qvar)


def session_rows(eng, session, n_path, max_expiries, max_strikes, n_sets, m, with_qvar):
    """the rows a sets launch of n_sets sets and m expiries left in the session: x [n_sets][m][n_path] and, with_qvar, qvar of the
    same shape (set-major; the qvar rows follow the n_sets m rows of x), downloaded through the engine `eng`"""
    snap, _ = session_snapshot_ptr(session, n_path, max_expiries, max_strikes)
    assert (2 if with_qvar else 1) * n_sets * m <= 2 * max_expiries
    count = n_sets * m * n_path
    x = eng.download(snap, count).reshape(n_sets, m, n_path)
    if not with_qvar:
        return x, None
    return x, eng.download(snap + 8 * count, count).reshape(n_sets, m, n_path)
