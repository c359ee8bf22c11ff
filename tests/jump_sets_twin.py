"""
CPU twin of the many-sets estimator on one set of jump rows (include/svmc_est.h svmc_jump_sets_payoff_chain),
shared by tests/test_jump_sets_host.py and tests/test_gpu_jump_sets.py.

No new arithmetic: with x | a ~ N(a - v / 2, v), v the same on every path, the estimator IS tests/tilted_cond_twin.estimator on the
rows mu = longdouble(a) - longdouble(v) / 2, cv = v at the set's gamma.  Only the recentring is taken where the device takes it: on
the rows (a, 0), that twin's corr_of(a, 0) -- it depends on neither v nor gamma.

TwinEngine stands where engine.HipEngine stands for the Python routes on a machine without a GPU: the rows by
tests/hawkes_cmc_twin.np_chain at sigma = 0, the tail by this twin, "pointers" raw host addresses as tests/fake_engine.py has them.
"""
import ctypes as C

import numpy as np

import hawkes_cmc_twin as hc
import tilted_cond_twin as tc
from fake_engine import FakeEngine

LD = np.longdouble
STAT_ORDER = tc.STATS


def rows_of(a, v):
    """(mu, cv) the tilted twin is fed: mu = a - v / 2 in long double, cv = v on every path"""
    a = np.asarray(a, dtype=np.float64).ravel()
    return a.astype(LD) - LD(v) / 2, np.full(a.size, float(v))


def corr_of(a, forward, recenter):
    a = np.asarray(a, dtype=np.float64).ravel()
    return tc.corr_of(a, np.zeros(a.size), forward, recenter)


def estimator(a, v, forward, strikes, types, gamma, recenter=False):
    """(prices [K], stderrs [K], stats dict of tilted_cond_twin.STATS and "corr") of one (set, expiry)"""
    mu, cv = rows_of(a, v)
    corr = corr_of(a, forward, recenter)
    saved = tc.corr_of
    tc.corr_of = lambda *_: corr                # the recentring of the rows (a, 0), whatever (mu, cv) are
    try:
        return tc.estimator(mu, cv, forward, strikes, types, gamma, recenter)
    finally:
        tc.corr_of = saved


def chain(a_rows, variances, gammas, forwards, strikes, types, recenter=False):
    """every (set, expiry): (prices [Q][m] -> [K_i], stderrs the same, stats [Q, m, 8] in STAT_ORDER, corr [m]), in double"""
    Q, m = len(gammas), len(a_rows)
    prices, errs, stats = [], [], np.empty((Q, m, len(STAT_ORDER)))
    for q in range(Q):
        pq, eq = [], []
        for i in range(m):
            p, e, st = estimator(a_rows[i], variances[q][i], forwards[i], strikes[i], types[i], gammas[q], recenter)
            pq.append(p.astype(np.float64).reshape(np.shape(strikes[i])))
            eq.append(e.astype(np.float64).reshape(np.shape(strikes[i])))
            stats[q, i] = [float(st[k]) for k in STAT_ORDER]
        prices.append(pq)
        errs.append(eq)
    corr = np.array([float(corr_of(a_rows[i], forwards[i], recenter)) for i in range(m)])
    return prices, errs, stats, corr


class HostBuffer:
    """engine.DeviceBuffer on host memory"""

    def __init__(self, n):
        self.n = int(n)
        self.array = np.zeros(self.n)
        self.ptr = self.array.ctypes.data

    def offset(self, n_doubles):
        return self.ptr + 8 * int(n_doubles)

    def free(self):
        pass


def _view(ptr, n):
    return np.ctypeslib.as_array((C.c_double * n).from_address(ptr))


class TwinEngine(FakeEngine):
    """FakeEngine with the two engine methods of row f20 by the twins; counts what it is asked for"""
    stream = None

    def __init__(self, n_path):
        super().__init__(n_path)
        self.stepping_calls, self.tail_calls, self.sets_per_call = 0, 0, []
        self.x = HostBuffer(n_path)                 # (the state array as a buffer: the host-array route uploads into it)

    def upload(self, ptr, host):
        host = np.ascontiguousarray(host, dtype=np.float64)
        C.memmove(ptr, host.ctypes.data, host.nbytes)

    def step_hawkesjd_jump_rows(self, ch, params, nb_steps_per_year, seed, call_id):
        from stochvolmodels_amd.pricers.hawkes_jd_pricer import PARAM_NAMES, jump_step_grid
        assert float(params[1]) == 0.0
        p = dict(zip(PARAM_NAMES, (float(x) for x in params)))
        nbs, dts = jump_step_grid(ch["ttms"], nb_steps_per_year)
        m = len(nbs)
        self.reserve_snapshots(2 * m)
        for i, st in enumerate(hc.np_chain(p, seed, self.n_path, nbs, dts, call_id=call_id)):
            self._snap[i] = st[0]
            self._snap[m + i] = 0.0
        self.stepping_calls += 1

    def copy_rows(self, dst_ptr, src_ptr, n_doubles):
        _view(dst_ptr, n_doubles)[:] = _view(src_ptr, n_doubles)

    def jump_sets_payoffs(self, forwards, strikes, codes, variances, gammas, recenter=False, a_rows=None, shifts=None, a_ptrs=None):
        ptrs = list(a_ptrs) if a_ptrs is not None else ([self.x.ptr] if a_rows is None else [self.snapshot_ptr(r) for r in a_rows])
        rows = [_view(p, self.n_path).copy() for p in ptrs]
        types = [np.where(np.asarray(c).ravel() == 0, "C", "P") for c in codes]
        self.tail_calls += 1
        self.sets_per_call.append(len(gammas))
        assert len(gammas) <= 16
        return chain(rows, np.asarray(variances), list(gammas), list(forwards), strikes, types, recenter)
