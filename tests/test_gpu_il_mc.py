"""
The Monte Carlo side of the impermanent-loss pricer on the device: svmc_il_payoff on uploaded log-returns
against tests/il_twin.py's long-double brute force of the estimator include/svmc.h states (keep and indicator decisions in
double on the host), over path counts around the wave, the block and the grid-stride loop, case counts around the kernel's
group of four, planted NaN and +-inf paths and a path whose recentred spot is negative; a case in company bit-equal to the case
alone; the Python routes against the C ABI; model_mc_il_payoff at the fixture's seed against the CPU twin's recorded results;
and the statistical test, |Fourier - Monte Carlo| <= 4 standard errors in all six (maturity, case) pairs at 400 000 paths.

The deviation measure is test_gpu_tilted.py's, |got - want| / max(|want|, 1e-4 scale), the scale per quantity in scales().  The bounds in TOL are measured: ten
times the largest deviation seen on the MI355X, rounded up to one digit (profiles/il_observed_tolerances.txt), none above the
project's 1e-12.  Every comparison prints its deviation (run with -s).
"""
import ctypes as C
import os

import numpy as np
import pytest

import il_twin
from test_gpu_tilted import deviation

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = 4                                  # IL_G of csrc/svmc_kernels.hip: cases per block
# value: 8.909e-13 observed, at ONE path (pay(p1) = 0.0247 formed from terms of +-92: one ulp of a term); ten times that is above
# the project's bound, so the bound is the project's 1e-12 itself
TOL = dict(value=1e-12, stderr=3e-13, square_root=4e-15, linear=3e-15, put=7e-14, call=4e-14, digital_put=9e-16, digital_call=9e-16)
assert max(TOL.values()) <= 1e-12      # the project's parity bound for prices and states: no bound here may exceed it
SEEN = {}
P0, NOTIONAL = 2200.0, 1e6
# nine cases: 2 G + 1
CASES = np.array([[2200.0, P0, 2000.0, 2400.0], [2050.0, P0, 2000.0, 2400.0], [2500.0, P0, 1800.0, 2600.0], [2200.0, P0, 2150.0, 2250.0],
                  [1900.0, P0, 2000.0, 2400.0], [2600.0, P0, 2100.0, 2300.0], [2200.0, P0, 1000.0, 4000.0], [2300.0, P0, 2199.0, 2201.0],
                  [2100.0, P0, 1500.0, 2205.0]])


@pytest.fixture(scope="module", autouse=True)
def largest_deviations():
    yield
    for k in il_twin.FIELDS:
        print(f"\nlargest il mc {k} deviation: {SEEN.get(k, float('nan')):.3e}  bound {TOL[k]:.0e}", end="")
    print()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "il_payoff.npz"))


def note(field, dev, what):
    SEEN[field] = max(SEEN.get(field, 0.0), dev)
    print(f"{what}: {field} deviation {dev:.3e} (bound {TOL[field]:.0e})")
    assert dev <= TOL[field], (what, field, dev)


def scales(p1, p0, pa, pb, notional):
    """the size of the numbers each quantity is formed from, as the forward is for an option's payoff spot - K: a piece's own
    size, and for the value and its error notional0 notional times the size of the terms pay is a difference of, 2 sqrt(S) and
    sqrt(p0) (S / p0 + 1) ~ 4 sqrt(p0) together.  IL is a difference of pieces up to a thousand times its size (narrow ranges
    most of all: over [2199, 2201] pay is 1e-5 of its terms), so an error of one ulp of a term is 1e-11 of the value; measured
    against notional0 notional alone the narrow case showed 9.3e-12 on the MI355X"""
    s = notional / (2 * np.sqrt(p0) - p0 / np.sqrt(pb) - np.sqrt(pa)) * 4 * np.sqrt(p0)
    return dict(value=s, stderr=s, square_root=np.sqrt(pb), linear=2 * np.sqrt(p0), put=pa, call=pb, digital_put=1.0, digital_call=1.0)


def il_payoff_cabi(x, cases, notional=NOTIONAL):
    """svmc_il_payoff on x uploaded to a private buffer -> [n_cases][10]"""
    from stochvolmodels_amd import _lib
    from stochvolmodels_amd.engine import DeviceBuffer
    L = _lib.load()
    x = np.ascontiguousarray(x, dtype=np.float64)
    table = np.ascontiguousarray(np.column_stack([cases, np.full(len(cases), notional)]))
    nbytes = C.c_size_t(0)
    _lib.check(L.svmc_il_payoff_workspace_bytes(x.size, len(table), C.byref(nbytes)))
    dx, ws = DeviceBuffer(x.size), DeviceBuffer((nbytes.value + 7) // 8)
    try:
        _lib.check(L.svmc_memcpy_h2d(dx.ptr, x.ctypes.data, x.nbytes, None))
        _lib.check(L.svmc_stream_synchronize(None))
        out = np.empty((len(table), 10))
        dp = C.POINTER(C.c_double)
        _lib.check(L.svmc_il_payoff(dx.ptr, x.size, table.ctypes.data_as(dp), len(table), out.ctypes.data_as(dp), ws.ptr, nbytes.value, None))
        return out
    finally:
        dx.free()
        ws.free()


def check_against_brute(out, x, cases, what, guard=True):
    for c, (p1, p0, pa, pb) in enumerate(cases):
        if guard:                                                   # a one-ulp difference in exp must not flip an indicator piece
            assert il_twin.nearest_boundary(x, p1, pa, pb) > 1e-9, (what, c)
        want, n_kept, n_dropped = il_twin.brute(x, p1, p0, pa, pb, NOTIONAL)
        assert (out[c, 8], out[c, 9]) == (n_kept, n_dropped), (what, c, out[c, 8:], n_kept, n_dropped)
        sc = scales(p1, p0, pa, pb, NOTIONAL)
        for i, k in enumerate(il_twin.FIELDS):
            note(k, deviation([out[c, i]], [want[k]], sc[k]), f"{what} case={c} n={x.size}")


def sample(n, seed, vol=0.1):
    return vol * np.random.default_rng(seed).standard_normal(n) + 0.02


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 100003])
def test_arithmetic_against_long_double(n):
    """4097: two path blocks and a ragged one; 100 003: 49 blocks, the moment rows summed by every block"""
    x = sample(n, 300 + n)
    for k in (1, G, G + 1, 2 * G + 1):
        check_against_brute(il_payoff_cabi(x, CASES[:k]), x, CASES[:k], f"paths k={k}")


def test_keep_rule_and_a_negative_spot():
    """NaN and +-inf paths are dropped and counted; a far path up lifts the mean of exp(x), so the far path down is recentred below zero"""
    x = sample(300, 9)
    x[[3, 70, 130, 299]] = [np.nan, np.inf, -np.inf, np.nan]
    x[200], x[250] = 3.0, -5.0                # a far path up lifts the mean of exp(x): the far path down has a negative recentred spot
    assert il_twin.host_spots(x, 2200.0)[1].min() < 0.0
    out = il_payoff_cabi(x, CASES)
    assert out[0, 8] == 296 and out[0, 9] == 4
    check_against_brute(out, x, CASES, "keep rule")
    none = il_payoff_cabi(np.array([np.nan, np.inf]), CASES[:1])           # no kept path: 0/0, and the counts say so
    assert none[0, 8] == 0 and none[0, 9] == 2 and np.isnan(none[0, 0])


def test_company_does_not_change_bits():
    x = sample(4097, 21)
    together = il_payoff_cabi(x, CASES)
    for c in range(len(CASES)):
        assert np.array_equal(il_payoff_cabi(x, CASES[c:c + 1])[0], together[c]), c
    assert np.array_equal(il_payoff_cabi(x, CASES[3:8]), together[3:8])


def test_python_routes_equal_the_c_abi():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.engine import get_engine
    x = sample(1000, 5)
    want = il_payoff_cabi(x, CASES)
    p1, p0, pa, pb = CASES.T
    value, stderr, extra = sv.compute_mc_il_payoff(x, p1, p0, pa, pb, notional=NOTIONAL, return_pieces=True)
    assert np.array_equal(value, want[:, 0]) and np.array_equal(stderr, want[:, 1])
    for i, k in enumerate(il_twin.FIELDS[2:]):
        assert np.array_equal(extra[k], want[:, 2 + i]), k
    assert (extra["n_kept"], extra["n_dropped"]) == (1000, 0)
    v1, e1 = sv.compute_mc_il_payoff(x, 2050.0, P0, 2000.0, 2400.0)        # scalars in, scalars out
    assert isinstance(v1, float) and (v1, e1) == (want[1, 0], want[1, 1])
    eng = get_engine(1000)
    eng.reserve_snapshots(2)
    eng.upload(eng.snapshot_ptr(1), x)
    v2, e2 = eng.il_payoffs(p1.reshape(3, 3), P0, pa.reshape(3, 3), pb.reshape(3, 3), NOTIONAL, snap_row=1)
    assert v2.shape == (3, 3) and np.array_equal(v2.ravel(), want[:, 0]) and np.array_equal(e2.ravel(), want[:, 1])


@pytest.fixture(scope="module")
def model_runs(fx):
    """model_mc_il_payoff of the candidate set at the fixture's seed and path count, per maturity: (value, stderr, extra)"""
    import stochvolmodels_amd as sv
    params = sv.LogSvParams(**dict(zip(("sigma0", "theta", "kappa1", "kappa2", "beta", "volvol"), map(float, fx["cand_params"]))))
    pa, pb, p1 = fx["cases"].T
    runs = [sv.LogSVPricer().model_mc_il_payoff(params, float(ttm), p1, float(fx["p0"]), pa, pb, nb_path=int(fx["mc_paths"]),
                                                seed=int(fx["mc_seed"]), notional=float(fx["notional"]), return_pieces=True)
            for ttm in fx["ttms"]]
    return params, runs


def test_model_mc_il_payoff_equals_the_twins_record(fx, model_runs):
    """the device's paths are the CPU twin's to rounding, and so are the value, its error and the pieces"""
    assert tuple(fx["mc_fields"]) == il_twin.FIELDS
    pa, pb, p1 = fx["cases"].T
    for t, (value, stderr, extra) in enumerate(model_runs[1]):
        assert (extra["n_kept"], extra["n_dropped"]) == (int(fx["mc_paths"]), 0)
        got = np.column_stack([value, stderr] + [extra[k] for k in il_twin.FIELDS[2:]])
        for c in range(3):
            sc = scales(p1[c], float(fx["p0"]), pa[c], pb[c], float(fx["notional"]))
            for i, k in enumerate(il_twin.FIELDS):
                note(k, deviation([got[c, i]], [fx[f"mc_{t}_twin"][c, i]], sc[k]), f"twin ttm={float(fx['ttms'][t]):.4f} case={c}")


def test_fourier_and_monte_carlo_agree_within_four_standard_errors(fx, model_runs):
    """the reference's own analytic-against-MC criterion, no case left out"""
    import stochvolmodels_amd as sv
    params, runs = model_runs
    pa, pb, p1 = fx["cases"].T
    for t, ttm in enumerate(fx["ttms"]):
        fourier = sv.logsv_il_pricer(params, float(ttm), p1, float(fx["p0"]), pa, pb, notional=float(fx["notional"]))
        value, stderr, _ = runs[t]
        z = (fourier - value) / stderr
        print(f"il z-scores ttm {float(ttm):.4f}: {z}  (twin: {fx[f'mc_{t}_z']})")
        assert np.all(np.abs(fourier - value) <= 4.0 * stderr), (float(ttm), z)


@pytest.mark.parametrize("which", ["heston", "hawkes"])
def test_other_models_price_on_their_resident_state(which):
    """HestonPricer / HawkesJDPricer.model_mc_il_payoff: the reduction on whatever the generator left, against the brute force of
    the state downloaded from the same engine"""
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.engine import get_engine
    n = 20000
    if which == "heston":
        pricer, params = sv.HestonPricer(), sv.BTC_HESTON_PARAMS
    else:
        pricer, params = sv.HawkesJDPricer(), sv.HawkesJDParams()
    p1, p0, pa, pb = CASES[:3].T
    value, stderr, extra = pricer.model_mc_il_payoff(params, 0.1, p1, p0, pa, pb, nb_path=n, seed=77, notional=NOTIONAL, return_pieces=True)
    x = get_engine(n).get_state()[0]
    out = np.column_stack([value, stderr] + [extra[k] for k in il_twin.FIELDS[2:]] + [np.full(3, extra["n_kept"]), np.full(3, extra["n_dropped"])])
    assert extra["n_kept"] == n
    check_against_brute(out, x, CASES[:3], which, guard=False)
    for c, (a, b, c1, d) in enumerate(CASES[:3]):
        assert il_twin.nearest_boundary(x, a, c1, d) > 1e-12
