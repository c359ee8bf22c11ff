"""
The analytic pricers' host side without a device: the one chain loop (analytic.chain_sums) against a recording stand-in of
the grid -- offsets, the zero-strike expiry, every [set][expiry] slice -- the single and batch wrappers' given-up bookkeeping,
and AnalyticGrid's pool and one-set-only methods on a stubbed library handle.
"""
import numpy as np
import pytest

import stochvolmodels_amd as sv
from stochvolmodels_amd import _lib, analytic
from stochvolmodels_amd.pricers import logsv_pricer as lp

KS = (3, 0, 2)                                  # strikes per expiry: the middle expiry takes no space
TTMS, FORWARDS = np.array([0.1, 0.25, 0.5]), np.array([1.0, 1.01, 1.02])
STRIKES = [np.linspace(0.9, 1.1, k) for k in KS]
TYPES = [np.full(k, "C") for k in KS]


def marked(expiry, n_sets, k):
    """what RecordingGrid writes for one expiry: [n_sets][k] values that name their set, expiry and strike"""
    return np.array([[0.001 * (100 * s + 10 * expiry + j + 1) for j in range(k)] for s in range(n_sets)])


class RecordingGrid:
    """AnalyticGrid stand-in: records the chain loop's calls; an inversion writes marked() into the result buffer where the
    device would write the sums; the second set of a batch has 7 given-up points"""
    made = []

    @classmethod
    def acquire(cls, phis, psis, n_coef):
        obj = cls(len(phis))
        obj.n = len(phis[0])
        cls.made.append(obj)
        return obj

    def __init__(self, n_sets):
        self.n_sets, self.n, self.calls, self.buf = n_sets, 0, [], None

    def reserve_results(self, n):
        self.calls.append(("reserve", n))
        self.buf = np.full(n, np.nan)

    def logsv_advance(self, dt, rows, is_spot_measure, order, rtol=None, atol=None):
        self.calls.append(("advance", float(dt), np.array(rows)))

    def queue_capped_sums(self, forward, strikes, offset):
        expiry = sum(c[0] == "queue" for c in self.calls)
        self.calls.append(("queue", forward, offset))
        k = np.size(strikes)
        self.buf[offset:offset + self.n_sets * k] = marked(expiry, self.n_sets, k).ravel()

    def download_results(self, n):
        self.calls.append(("download", n))
        self.last_given_up = np.array([0, 7][:self.n_sets])
        return self.buf[:n].copy()

    def release(self):
        self.calls.append(("release",))


def test_chain_loop_offsets_and_slices():
    grid = RecordingGrid(2)
    advances = []
    sums = analytic.chain_sums(grid, TTMS, FORWARDS, STRIKES, lambda i, dt: advances.append((i, dt)))
    assert [c[1] for c in grid.calls if c[0] == "reserve"] == [10]
    assert [c[2] for c in grid.calls if c[0] == "queue"] == [0, 6, 6]
    assert [c[1] for c in grid.calls if c[0] == "download"] == [10]
    assert [c[0] for c in grid.calls] == ["reserve", "queue", "queue", "queue", "download"]
    assert [a[0] for a in advances] == [0, 1, 2]
    np.testing.assert_array_equal([a[1] for a in advances], np.diff(np.concatenate([[0.0], TTMS])))
    assert len(sums) == 2 and all(len(s) == 3 for s in sums)
    for s in range(2):
        for i, k in enumerate(KS):
            assert sums[s][i].shape == (k,)
            np.testing.assert_array_equal(sums[s][i], marked(i, 2, k)[s])
    # ... and the prices keep the [set][expiry] layout: every slice from its own sums
    prices = analytic.chain_prices_from_sums(sums, "vanilla", TTMS, FORWARDS, np.ones(3), STRIKES, TYPES, True)
    for s in range(2):
        for i, k in enumerate(KS):
            np.testing.assert_array_equal(prices[s][i], analytic.vanilla_prices_from_capped(
                marked(i, 2, k)[s], FORWARDS[i], STRIKES[i], TYPES[i], 1.0, True))


def test_single_wrapper_notes_an_int_and_the_batch_an_array(monkeypatch):
    monkeypatch.setattr(lp, "AnalyticGrid", RecordingGrid)
    RecordingGrid.made = []
    kw = dict(ttms=TTMS, forwards=FORWARDS, discfactors=np.ones(3), strikes_ttms=STRIKES, optiontypes_ttms=TYPES)
    single = lp.logsv_chain_pricer(params=sv.LOGSV_BTC_PARAMS, **kw)
    assert type(lp.LAST_ANALYTIC_GIVEN_UP) is int and lp.LAST_ANALYTIC_GIVEN_UP == 0
    assert [p.shape for p in single] == [(3,), (0,), (2,)]
    with pytest.warns(RuntimeWarning, match=r"given up on \[0, 7\] of 1000") as rec:
        batch = lp.logsv_chain_pricer_batch(params_list=[sv.LOGSV_BTC_PARAMS, sv.LOGSV_BTC_PARAMS], **kw)
    assert rec[0].filename == __file__                      # the warning points at the caller's line
    assert isinstance(lp.LAST_ANALYTIC_GIVEN_UP, np.ndarray) and lp.LAST_ANALYTIC_GIVEN_UP.tolist() == [0, 7]
    one, two = RecordingGrid.made
    assert (one.n_sets, two.n_sets) == (1, 2)
    assert [c[0] for c in one.calls] == ["reserve"] + ["advance", "queue"] * 3 + ["download", "release"]
    assert [c[2] for c in one.calls if c[0] == "queue"] == [0, 3, 3]
    assert [c[2] for c in two.calls if c[0] == "queue"] == [0, 6, 6]
    for a, b in zip(one.calls, two.calls):                  # one set is the batch at one set: the same advances, row for row
        if a[0] == "advance":
            assert a[1] == b[1] and a[2].shape == (1, 8) and b[2].shape == (2, 8)
            np.testing.assert_array_equal(a[2][0], b[2][0])
    for a, b in zip(single, batch[0]):
        np.testing.assert_array_equal(a, b)
    monkeypatch.setattr(lp, "LAST_ANALYTIC_GIVEN_UP", 0)


class StubLib:
    """libsvmc stand-in: every call succeeds and is recorded; svmc_malloc hands out distinct addresses nothing dereferences"""

    def __init__(self):
        self.calls, self.next_ptr = [], 1 << 20

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            if name == "svmc_malloc":
                args[0]._obj.value, self.next_ptr = self.next_ptr, self.next_ptr + (1 << 30)
            elif name == "svmc_device_count":
                args[0]._obj.value = 1
            elif name == "svmc_get_device":
                args[0]._obj.value = 0
            return 0
        return call


@pytest.fixture
def stub():
    lib = StubLib()
    with pytest.MonkeyPatch.context() as m:
        m.setattr(_lib, "load", lambda: lib)
        m.setattr(analytic, "_POOL", {})
        yield lib
        for g in list(analytic._POOL.values()):             # while the stub still answers svmc_free
            g.close()


def test_pool_is_keyed_by_sets_and_sizes(stub):
    phi = -0.5 + 1j * np.linspace(0.0, 10.0, 50)
    psi = np.zeros_like(phi)
    g1 = analytic.AnalyticGrid.acquire(phi, psi, 3)
    assert (g1.n_sets, g1.n, g1.n_coef) == (1, 50, 3) and g1.last_given_up.tolist() == [0]
    g1.release()
    uploads = stub.calls.count("svmc_memcpy_h2d")
    again = analytic.AnalyticGrid.acquire(phi, psi, 3)
    assert again is g1 and stub.calls.count("svmc_memcpy_h2d") == uploads           # the same grids: nothing re-uploaded
    g2 = analytic.AnalyticGrid.acquire([phi, 2.0 * phi], [psi, psi], 3)             # two sets of the same length
    assert g2 is not g1 and (g2.n_sets, g2.n) == (2, 50) and g2.last_given_up.tolist() == [0, 0]
    private = analytic.AnalyticGrid.acquire(phi, psi, 3)                            # g1 is out: a second acquire builds its own
    assert private is not g1
    private.close()
    again.release()
    stacked = analytic.AnalyticGrid.acquire(phi[None, :], psi[None, :], 3)          # [1][n] is the 1-D grid's key
    assert stacked is g1
    stacked.release()
    uploads = stub.calls.count("svmc_memcpy_h2d")
    changed = analytic.AnalyticGrid.acquire(phi + 1.0, psi, 3)                      # other bytes: phi alone goes up again
    assert changed is g1 and stub.calls.count("svmc_memcpy_h2d") == uploads + 1
    np.testing.assert_array_equal(changed.phi_host, (phi + 1.0)[None, :])
    changed.release()
    wider = analytic.AnalyticGrid.acquire(phi, psi, 5)                              # another coefficient count, another key
    assert wider is not g1
    wider.release()
    g2.release()
    assert analytic.AnalyticGrid.acquire([phi, phi], [psi, psi], 3) is g2
    g2.release()
    assert len(analytic._POOL) == 3


def test_one_set_only_methods_refuse_a_batch(stub):
    phi = -0.5 + 1j * np.linspace(0.0, 10.0, 50)
    two = analytic.AnalyticGrid([phi, phi], [0 * phi, 0 * phi], 1)
    two.reserve_results(8)
    launches = len(stub.calls)
    with pytest.raises(AssertionError):
        two.heston_advance(0.1, 0.04, 0.04, 1.0, 0.5, -0.5, True)
    with pytest.raises(AssertionError):
        two.queue_qvar_sums(0.1, np.array([0.04]), 0)
    with pytest.raises(AssertionError):                      # ... and through the chain loop
        analytic.chain_sums(two, TTMS, FORWARDS, STRIKES, lambda i, dt: None, "qvar")
    assert stub.calls[launches:].count("svmc_mgf_qvar_slice") == 0 and "svmc_heston_mgf_grid" not in stub.calls
    two.close()
    one = analytic.AnalyticGrid(phi, 0 * phi, 1)
    one.reserve_results(8)
    one.heston_advance(0.1, 0.04, 0.04, 1.0, 0.5, -0.5, True)
    one.queue_qvar_sums(0.1, np.array([0.04]), 0)
    assert stub.calls[-2:] == ["svmc_heston_mgf_grid", "svmc_mgf_qvar_slice"]
    one.close()
