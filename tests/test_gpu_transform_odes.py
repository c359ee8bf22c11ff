"""
The analytic route's device kernels against independent high-precision truth:

  * the LogSV coefficient ODE, both kernel forms -- logsv_mgf_grid_kernel (one 16-lane row per grid point) and
    logsv_mgf_grid_lane_kernel (one lane per grid point, taken beyond 8192 points) -- against the Taylor-series solutions
    of tests/golden/transform_odes.npz (make_golden_transform_odes.py: two independent fixed-point solves agreeing to
    1e-18), every component A_k and log E, both measures, both expansion orders, 1/365 to 5 years, and a chained pair of
    slices with different vol_backbone_eta (the a_t0 carry);
  * the batch contract of logsv_chain_pricer_batch across the row / lane switch (8, 9, 16 and 17 sets);
  * the single C entry points svmc_logsv_mgf_grid / svmc_mgf_vanilla_slice against their batch forms at one set, bit for bit;
  * the inversion kernels (mgf_vanilla_slice_kernel, mgf_qvar_slice_kernel, mgf_gamma_slice_kernel) against the same
    Simpson-weighted sum evaluated in mpmath from the same doubles, at grid lengths and strike counts around the kernels'
    256-thread and 32-strike boundaries, and the nansum contract (NaN terms dropped, inf kept, a -inf log E a zero term);
  * the density slices (mgf_pdf_slice_kernel, mgf_digital_slice_kernel of csrc/svmc_density.hip) against the sums of the
    reference's pdf_with_mgf_grid and digital_slice_pricer_with_mgf_grid in mpmath, under the same error model: the
    256-thread stride loop at 255, 256 and 257 points, both branches of legacy_weight (Simpson, and the local-step weights on
    a geometrically stretched grid), both arms of the digital kernel's Smith division (|Re phi| >= |Im phi| at the first
    grid points only), both contours, the 64-set launch boundary of the pdf entry (64, 65 and 129 sets, each bit-equal to its
    single call), the 32-strike chunks of the digital entry, a negative scale, and the nansum contract of both;
  * all five slice kernels against the bits recorded in tests/golden/mgf_slice_bits.npz (make_golden_mgf_slice_bits.py) before
    they came to share one sum loop (csrc/svmc_mgf_slice.h): the loop's trip counts, the strike chunk and the pdf launch
    boundary, every weight rule and contour, and non-finite log E entries.

Errors of the ODE are |dev - mp| / max(1, |mp|), the largest over a point's components and log E; every report() line
prints the measured worst value against its bound.
"""
import ctypes as C
import json
import math
import os

import mpmath as mp
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROW_MAX = 8192                 # csrc/svmc_analytic.hip: rows while one set's grid has at most this many points
# The ODE kernels run here at rtol 1e-12 / atol 1e-14, a hundred times tighter than the pricers' 1e-10 / 1e-12 (where the
# worst measured error is 4.4e-9: DOP853's global error, beta_neg, inverse measure, order 2, 0.25 years), so that the bound
# has room under the hard ceiling of 1e-8, which keeps a wrong term of relative weight 1e-7 visible.
# Measured worst: 4.1e-11 (rows: kappa2_zero, inverse measure, order 2, 0.25 years), 1.3e-11 (lanes), 4.1e-11 between the
# two forms; x 4 headroom.
ODE_RTOL, ODE_ATOL = 1e-12, 1e-14
ODE_BOUND = 1.7e-10
assert ODE_BOUND <= 1e-8
EPS = 2.0 ** -53


def report(name, value, bound):
    print(f"DEVICE-MAX {name}: {value:.4g} (bound {bound:.4g})")
    assert value <= bound, (name, value, bound)


@pytest.fixture(scope="module")
def L():
    from stochvolmodels_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "transform_odes.npz"))


class Dev:
    """a device copy of a host array (complex128, float64 or int32 contents), freed with the object"""

    def __init__(self, L, host=None, n_doubles=None):
        from stochvolmodels_amd.engine import DeviceBuffer
        self.L = L
        nd = n_doubles if host is None else np.ascontiguousarray(host).nbytes // 8
        self.buf = DeviceBuffer(max(int(nd), 1))
        if host is not None:
            h = np.ascontiguousarray(host)
            _check(L.svmc_memcpy_h2d(self.buf.ptr, h.ctypes.data, h.nbytes, None))
            _check(L.svmc_stream_synchronize(None))

    @property
    def ptr(self):
        return self.buf.ptr

    def get(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        _check(self.L.svmc_memcpy_d2h(out.ctypes.data, self.buf.ptr, out.nbytes, None))
        _check(self.L.svmc_stream_synchronize(None))
        return out


def _check(rc):
    from stochvolmodels_amd import _lib
    _lib.check(rc)


def _pf(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def mgf_grid(L, phi, psi, ttm, rows, spot, order, a0=None):
    """svmc_logsv_mgf_grid_batch on [n_sets][n] grids: (A [n_sets][n][n_coef], log E [n_sets][n])"""
    phi = np.ascontiguousarray(np.atleast_2d(phi), dtype=np.complex128)
    psi = np.ascontiguousarray(np.atleast_2d(psi), dtype=np.complex128)
    rows = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.float64)
    s, n = phi.shape
    nc = 5 if order == 2 else 3
    a = Dev(L, np.zeros((s, n, nc), dtype=np.complex128) if a0 is None else np.asarray(a0, dtype=np.complex128))
    lm = Dev(L, n_doubles=2 * s * n)
    dphi, dpsi = Dev(L, phi), Dev(L, psi)
    _check(L.svmc_logsv_mgf_grid_batch(dphi.ptr, dpsi.ptr, n, s, float(ttm), _pf(rows), int(spot), int(order), a.ptr, lm.ptr,
                                       ODE_RTOL, ODE_ATOL, None))
    return a.get((s, n, nc), np.complex128), lm.get((s, n), np.complex128)


def set_row(params, eta=1.0):
    return np.array([*params, eta, 0.0])


def ode_err(A, lm, A_mp, lm_mp):
    """|dev - mp| / max(1, |mp|) per point, the largest over the components and log E"""
    nc = A.shape[-1]
    e = np.abs(A - A_mp[..., :nc]) / np.maximum(1.0, np.abs(A_mp[..., :nc]))
    return np.maximum(e.max(axis=-1), np.abs(lm - lm_mp) / np.maximum(1.0, np.abs(lm_mp)))


def cases(fx):
    """(set index, measure index, order index, ttm index) of every fixture block"""
    S, T = fx["logsv_params"].shape[0], fx["logsv_ttms"].size
    return [(s, m, o, t) for s in range(S) for m in range(2) for o in range(2) for t in range(T)]


# ---- a, b, c: the LogSV coefficient ODE, row and lane form, against mp -----------------------------------------------------
@pytest.fixture(scope="module")
def row_lane(L, fx):
    """both forms' results on every fixture block, the lane form from the points tiled past ROW_MAX"""
    out = {}
    P = fx["logsv_phi"].shape[-1]
    reps = ROW_MAX // P + 1
    for s, m, o, t in cases(fx):
        params, spot, order, ttm = fx["logsv_params"][s], m == 0, o + 1, fx["logsv_ttms"][t]
        phi, psi = fx["logsv_phi"][s, m], fx["logsv_psi"][s, m]
        row = mgf_grid(L, phi, psi, ttm, set_row(params), spot, order)
        lane = mgf_grid(L, np.tile(phi, reps), np.tile(psi, reps), ttm, set_row(params), spot, order)
        out[s, m, o, t] = (row[0][0], row[1][0], lane[0][0].reshape(reps, P, -1), lane[1][0].reshape(reps, P))
    return out


def test_logsv_row_form_vs_mp(fx, row_lane):
    assert np.max(fx["logsv_agree"]) <= 1e-18
    worst, where = 0.0, None
    for (s, m, o, t), (A, lm, _, _) in row_lane.items():
        assert np.all(np.isfinite(A)) and np.all(np.isfinite(lm)), ("a grid point given up", s, m, o, t)
        e = ode_err(A, lm, fx["logsv_A"][s, m, o, t], fx["logsv_log_mgf"][s, m, o, t])
        if e.max() > worst:
            worst, where = float(e.max()), (str(fx["logsv_names"][s]), m, o + 1, float(fx["logsv_ttms"][t]), int(e.argmax()))
    print("row form worst at (set, measure, order, ttm, point)", where)
    report("LogSV row form vs mp", worst, ODE_BOUND)


def test_logsv_lane_form_vs_mp(fx, row_lane):
    worst = 0.0
    for (s, m, o, t), (_, _, A, lm) in row_lane.items():
        # every copy of a point the same bits as its first: no lane reads a neighbour's state
        assert np.array_equal(A, np.broadcast_to(A[:1], A.shape)) and np.array_equal(lm, np.broadcast_to(lm[:1], lm.shape)), \
            ("lane copies differ", s, m, o, t)
        assert np.all(np.isfinite(A)) and np.all(np.isfinite(lm)), ("a grid point given up", s, m, o, t)
        e = ode_err(A[0], lm[0], fx["logsv_A"][s, m, o, t], fx["logsv_log_mgf"][s, m, o, t])
        worst = max(worst, float(e.max()))
    report("LogSV lane form vs mp", worst, ODE_BOUND)


def test_logsv_row_vs_lane(fx, row_lane):
    worst, identical = 0.0, True
    for (s, m, o, t), (A, lm, Al, lml) in row_lane.items():
        identical &= bool(np.array_equal(A, Al[0]) and np.array_equal(lm, lml[0]))
        worst = max(worst, float(ode_err(A, lm, Al[0], lml[0]).max()))
    print("row and lane forms bit-identical:", identical)
    report("LogSV row form vs lane form", worst, ODE_BOUND)


def test_logsv_chained_slices_vs_mp(L, fx):
    """the a_t0 carry: a slice to chain_ttms[0] at eta_0, then the next over the difference at eta_1, from the first's A"""
    s = int(fx["chain_set"])
    params, (t0, t1), (e0, e1) = fx["logsv_params"][s], fx["chain_ttms"], fx["chain_etas"]
    assert np.max(fx["chain_agree"]) <= 1e-18
    P = fx["logsv_phi"].shape[-1]
    reps = ROW_MAX // P + 1
    worst = {}
    for m in range(2):
        phi, psi = fx["logsv_phi"][s, m], fx["logsv_psi"][s, m]
        for form, k in (("row", 1), ("lane", reps)):
            A0, _ = mgf_grid(L, np.tile(phi, k), np.tile(psi, k), t0, set_row(params, e0), m == 0, 2)
            A1, lm1 = mgf_grid(L, np.tile(phi, k), np.tile(psi, k), float(t1 - t0), set_row(params, e1), m == 0, 2, a0=A0)
            A0, A1, lm1 = A0[0, :P], A1[0, :P], lm1[0, :P]
            e = max(float(ode_err(A0, np.zeros(P), fx["chain_A_first"][m], np.zeros(P)).max()),
                    float(ode_err(A1, lm1, fx["chain_A"][m], fx["chain_log_mgf"][m]).max()))
            worst[form] = max(worst.get(form, 0.0), e)
    for form, e in worst.items():
        report(f"LogSV chained slices ({form} form) vs mp", e, ODE_BOUND)


# ---- d: the batch contract across the form switch --------------------------------------------------------------------------
def test_logsv_batch_bit_identical_across_form_switch():
    """logsv_chain_pricer_batch promises the bits of one logsv_chain_pricer call per set.  At the pricers' 1000-point grid, 8
    sets fill 8000 points of a launch and 9 or more would cross 8192: a set's form (and so its rounding) must not follow the
    number of sets sharing its launch"""
    import stochvolmodels_amd as sv
    g = np.load(os.path.join(HERE, "golden", "analytic.npz"))
    kk, types, ttms = g["strikes"], g["types"], g["ttms"]
    chain = sv.OptionChain(ttms=ttms, forwards=np.ones(4), strikes_ttms=(kk,) * 4, optiontypes_ttms=(types,) * 4, ids=None)
    pricer = sv.LogSVPricer()
    base = [[float(a) for a in g[f"logsv_{t}_params"]] for t in ("btc", "readme", "quick", "test", "fig3")]
    sets = []
    for i in range(17):
        v = list(base[i % 5])
        bump = 1.0 + 0.01 * (i // 5)                 # distinct sets: theta and volvol bumped per round of the five
        v[1] *= bump
        v[5] *= bump
        sets.append(sv.LogSvParams(sigma0=v[0], theta=v[1], kappa1=v[2], kappa2=v[3], beta=v[4], volvol=v[5]))
    for spot in (True, False):
        single = [np.stack(pricer.price_chain(chain, p, is_spot_measure=spot)) for p in sets]
        for n in (8, 9, 16, 17):
            batch = pricer.price_chain_batch(chain, sets[:n], is_spot_measure=spot)
            for i, (a, b) in enumerate(zip(batch, single[:n])):
                np.testing.assert_array_equal(np.stack(a), b, err_msg=f"{n} sets, set {i}, spot {spot}")


@pytest.mark.parametrize("order", [1, 2])
def test_single_entry_points_are_their_batch_forms_at_one_set(L, order):
    """svmc_logsv_mgf_grid and svmc_mgf_vanilla_slice, which the Python package no longer calls, against
    svmc_logsv_mgf_grid_batch and svmc_mgf_vanilla_slice_batch at n_sets = 1: a 50-point grid (a partial last block of the row
    form), two chained expiries, 3 strikes -- A, log E and the sums bit for bit"""
    n, nc = 50, 5 if order == 2 else 3
    phi = -0.5 + 1j * np.linspace(0.0, 5.6 / 0.16, n)
    psi = np.zeros(n, dtype=np.complex128)
    params = (0.8376, 1.0413, 3.1844, 3.058, 0.1514, 1.8458)
    forward, strikes = 1.02, np.array([0.8, 1.0, 1.3])
    dphi, dpsi = Dev(L, phi), Dev(L, psi)
    single = [Dev(L, np.zeros((n, nc), dtype=np.complex128)), Dev(L, n_doubles=2 * n), Dev(L, n_doubles=3)]
    batch = [Dev(L, np.zeros((n, nc), dtype=np.complex128)), Dev(L, n_doubles=2 * n), Dev(L, n_doubles=3)]
    for dt, eta in ((0.1, 1.0), (0.15, 1.1)):
        _check(L.svmc_logsv_mgf_grid(dphi.ptr, dpsi.ptr, n, dt, *params, 1, order, eta, single[0].ptr, single[1].ptr,
                                     ODE_RTOL, ODE_ATOL, None))
        _check(L.svmc_mgf_vanilla_slice(dphi.ptr, single[1].ptr, n, forward, _pf(strikes), 3, single[2].ptr, None))
        _check(L.svmc_logsv_mgf_grid_batch(dphi.ptr, dpsi.ptr, n, 1, dt, _pf(set_row(params, eta)), 1, order, batch[0].ptr,
                                           batch[1].ptr, ODE_RTOL, ODE_ATOL, None))
        _check(L.svmc_mgf_vanilla_slice_batch(dphi.ptr, batch[1].ptr, n, 1, forward, _pf(strikes), 3, batch[2].ptr, None))
        for a, b, shape, dtype in zip(single, batch, ((n, nc), n, 3), (np.complex128, np.complex128, np.float64)):
            got = a.get(shape, dtype)
            assert np.all(np.isfinite(got.view(np.float64)))
            np.testing.assert_array_equal(got, b.get(shape, dtype))


# ---- g: the inversion kernels against the exact Simpson-weighted sum ------------------------------------------------------
# The reference is the same sum in mpmath from the same doubles (the grid, log E, x or K ttm, the weights' h), the exponent's
# argument included.  Bound: |dev - ref| <= 2^-53 (C_SUM n sum_j |t_j| + 2 sum_j |t_j| a_j), C_SUM = 8.
#   C_SUM n: a term carries at most ~12 roundings of its own (cexp_ <= 5e-16, the weight's division and products, the
#   complex weight's division under the gamma kernel), and the sum at most ceil(n / 256) serial additions per thread, six
#   shuffle levels and three LDS additions, each relative to a partial sum <= sum |t_j|: 12 + n / 256 + 9 <= 8 n for n >= 3.
#   2 a_j: the kernel forms the argument of cexp_ in double, a product and a sum per part (fused or not), an absolute error
#   <= 2^-53 a_j with a_j = |Re log E_j| + |Im log E_j| + |x| (|Re phi_j| + |Im phi_j|) per part, and an absolute error d
#   of the argument is a relative error d of the term.
C_SUM = 8.0


def checked_strikes(k):
    """the strikes held to the mp sum: both ends of every 32-strike chunk (the rest are held to the float64 sum below)"""
    return sorted({i for c in range(0, k, 32) for i in (c, min(c + 31, k - 1))})


def np_sum_check(name, got, ref):
    """every strike against the same sum in float64 (numpy), to 1e-12 of its sum of |term| -- catches a strike chunk mixed up"""
    val, absum = ref
    assert np.all(np.abs(got - val) <= 1e-12 * absum), (name, np.max(np.abs(got - val) / absum))


def legacy_weight(j, n):
    """utils/mgf_pricer.py:158-171: 1, 4, 2, 4, ..., the last index 1 -- or 4 where it is odd"""
    w = 1.0 if j in (0, n - 1) else 2.0
    return 4.0 if j & 1 else w


def mp_sum(terms):
    """(nansum of the terms, sum |t_j|, sum |t_j| a_j over the finite ones): NaN dropped, inf kept"""
    with mp.workdps(50):
        keep = [(t, a) for t, a in terms if not mp.isnan(t)]
        fin = [(t, a) for t, a in keep if mp.isfinite(t)]
        return mp.fsum(t for t, _ in keep), mp.fsum(abs(t) for t, _ in fin), mp.fsum(abs(t) * a for t, a in fin)


def _term(w, lm, x, z):
    """(Re[w exp(log E - x z)] in mp, a_j); inf / NaN as IEEE arithmetic gives them.  At Re log E = +inf the exponential is
    (inf cos, inf sin) of the phase -- (inf, 0) at a phase of exactly 0, as C99's cexp and NumPy's -- and the real part of the
    product is Re[w] inf cos - Im[w] inf sin: that infinity, or NaN where the two are infinities of opposite sign"""
    a = abs(lm.real) + abs(lm.imag) + abs(x) * (abs(z.real) + abs(z.imag))
    if math.isnan(lm.real) or math.isnan(lm.imag):
        return mp.nan, a
    if lm.real == -math.inf:
        return mp.mpf(0), 0.0
    arg = mp.mpc(lm) - mp.mpf(x) * mp.mpc(z)
    if lm.real == math.inf:
        parts = {mp.sign(v) for v in (w.real * mp.cos(arg.imag), -w.imag * mp.sin(arg.imag))} - {0}
        return (mp.inf * parts.pop() if len(parts) == 1 else mp.nan), a
    return (w * mp.exp(arg)).real, a


def vanilla_ref(phi, lm, x):
    n = phi.size
    h = phi[1].imag - phi[0].imag
    terms = []
    with mp.workdps(50):
        for j in range(n):
            p = mp.mpf(phi[j].imag)
            pw = (mp.mpf(h) / 3 * legacy_weight(j, n) / mp.pi) / (p * p + mp.mpf(1) / 4)
            terms.append(_term(mp.mpc(pw), lm[j], x, phi[j]))
    return mp_sum(terms)


def simpson_weights(n):
    return np.array([legacy_weight(j, n) for j in range(n)])


def vanilla_np(phi, lm, x):
    h = phi[1].imag - phi[0].imag
    pw = (h / 3 * simpson_weights(phi.size) / np.pi) / (phi.imag ** 2 + 0.25)
    t = (pw * np.exp(lm[None, :] - x[:, None] * phi[None, :])).real
    return t.sum(axis=1), np.abs(t).sum(axis=1)


def synthetic_grid(n, vol_scaler, spot=True, seed=0):
    """the pricer's phi grid shape at n points, and a smooth decaying log E with a phase"""
    p = np.linspace(0, 5.6 / vol_scaler, n)
    phi = (-0.5 if spot else 0.5) + 1j * p
    rng = np.random.default_rng(seed)
    lm = -0.5 * (vol_scaler * p) ** 2 * (1 + 0.1 * rng.uniform(size=n)) + 1j * 0.3 * p * rng.uniform(size=n)
    return phi, lm


def check_sum(name, dev, ref, n):
    val, absum, absum_a = ref
    if mp.isinf(val):
        assert dev == float(val), (name, dev, val)
        return 0.0
    err = abs(mp.mpf(dev) - val)
    bound = EPS * (C_SUM * n * absum + 2 * absum_a)
    assert err <= bound, (name, float(err), float(bound))
    return float(err / bound) if bound > 0 else 0.0


@pytest.mark.parametrize("n", [3, 4, 255, 256, 257, 1000, 1001])
def test_vanilla_slice_kernel_vs_exact_sum(L, n):
    """several sets (each its own grid spacing) and strike counts across the 32-strike chunk boundary"""
    scalers = (0.16, 0.05, 0.3)
    grids = [synthetic_grid(n, v, seed=i) for i, v in enumerate(scalers)]
    phi = np.stack([g[0] for g in grids])
    lm = np.stack([g[1] for g in grids])
    dphi, dlm = Dev(L, phi), Dev(L, lm)
    forward = 1.3
    worst = 0.0
    for k in (1, 32, 33, 65):
        strikes = forward * np.exp(np.linspace(-0.6, 0.6, k))
        out = Dev(L, n_doubles=3 * k)
        _check(L.svmc_mgf_vanilla_slice_batch(dphi.ptr, dlm.ptr, n, 3, forward, _pf(strikes), k, out.ptr, None))
        got = out.get((3, k), np.float64)
        for s in range(3):
            x = np.array([math.log(forward / float(K)) for K in strikes])
            np_sum_check(f"vanilla n={n} k={k} set={s}", got[s], vanilla_np(phi[s], lm[s], x))
            for i in checked_strikes(k):
                worst = max(worst, check_sum(f"vanilla n={n} k={k} set={s} strike={i}", got[s, i],
                                             vanilla_ref(phi[s], lm[s], x[i]), n))
    report(f"vanilla slice n={n} error / bound", worst, 1.0)


def test_vanilla_slice_kernel_nansum_contract(L):
    n = 257
    phi, lm = synthetic_grid(n, 0.16)
    forward, strikes = 1.0, np.array([1.0, 0.8])                 # x = 0 first: the inf term's phase is exactly 0
    cases_ = {"nan": {5: complex(np.nan, 0.0)}, "neg_inf": {5: complex(-np.inf, 0.0), 200: complex(-np.inf, 0.0)},
              "pos_inf": {7: complex(np.inf, 0.0)}}
    for name, edits in cases_.items():
        z = lm.copy()
        for j, v in edits.items():
            z[j] = v
        out = Dev(L, n_doubles=2)
        dphi, dlm = Dev(L, phi), Dev(L, z)
        _check(L.svmc_mgf_vanilla_slice_batch(dphi.ptr, dlm.ptr, n, 1, forward, _pf(strikes), 2, out.ptr, None))
        got = out.get(2, np.float64)
        for i, K in enumerate(strikes):
            ref = vanilla_ref(phi, z, math.log(forward / float(K)))
            if name == "pos_inf" and i == 0:
                assert got[i] == np.inf, got
            elif name == "pos_inf":
                assert np.isinf(got[i]) and got[i] == float(ref[0]), (got[i], ref[0])
            else:
                assert np.isfinite(got[i]), (name, got[i])
                check_sum(f"vanilla {name} strike {i}", got[i], ref, n)


def qvar_ref(psi, lm, kt):
    n = psi.size
    h = psi[1].imag - psi[0].imag
    terms = []
    with mp.workdps(50):
        for j in range(n):
            w = (mp.mpf(h) / 3 * legacy_weight(j, n) / mp.pi) / (mp.mpc(psi[j]) ** 2)
            terms.append(_term(w, lm[j], -kt, psi[j]))              # exp(K ttm psi + log E)
    return mp_sum(terms)


@pytest.mark.parametrize("n", [3, 4, 255, 256, 257, 1000, 1001])
def test_qvar_slice_kernel_vs_exact_sum(L, n):
    psi = -0.5 + 1j * np.linspace(0, 400.0, n)
    rng = np.random.default_rng(n)
    lm = -0.01 * np.abs(psi) * (1 + 0.1 * rng.uniform(size=n)) + 1j * 0.05 * psi.imag
    if n > 8:
        lm[3] = complex(np.nan, 0.0)                               # dropped
        lm[n - 2] = complex(-np.inf, 0.0)                          # a zero term
    dpsi, dlm = Dev(L, psi), Dev(L, lm)
    ttm, worst = 0.5, 0.0
    for k in (1, 32, 33, 65):
        strikes = np.linspace(0.05, 2.0, k)
        out = Dev(L, n_doubles=k)
        _check(L.svmc_mgf_qvar_slice(dpsi.ptr, dlm.ptr, n, ttm, _pf(strikes), k, out.ptr, None))
        got = out.get(k, np.float64)
        kt = strikes * ttm
        h = psi[1].imag - psi[0].imag
        fin = ~np.isnan(lm.real)
        w = (h / 3 * simpson_weights(n) / np.pi) / psi ** 2
        t = (w[None, fin] * np.exp(kt[:, None] * psi[None, fin] + lm[None, fin])).real
        np_sum_check(f"qvar n={n} k={k}", got, (t.sum(axis=1), np.abs(t).sum(axis=1)))
        for i in checked_strikes(k):
            worst = max(worst, check_sum(f"qvar n={n} k={k} strike={i}", got[i], qvar_ref(psi, lm, float(kt[i])), n))
    report(f"qvar slice n={n} error / bound", worst, 1.0)


def gamma_ref(phi, lm, x, gamma, shortcut):
    n = phi.size
    h = phi[1].imag - phi[0].imag
    terms = []
    with mp.workdps(50):
        for j in range(n):
            dp_pi = mp.mpf(h) / 3 * legacy_weight(j, n) / mp.pi
            if shortcut:
                p = mp.mpf(phi[j].imag)
                w = mp.mpc(dp_pi / (p * p + mp.mpf(1) / 4))
            else:
                pg = mp.mpc(phi[j]) + mp.mpf(gamma)
                w = -dp_pi / ((pg + 1) * pg)
            terms.append(_term(w, lm[j], x, phi[j]))
    return mp_sum(terms)


@pytest.mark.parametrize("n", [3, 4, 255, 256, 257, 1000, 1001])
def test_gamma_slice_kernel_vs_exact_sum(L, n):
    """three sets with their own grid spacing and gamma: the real shortcut (Re phi = 0.5 + gamma) and the complex weight;
    type 'C' with normalizer 1 and gamma forward 0 gives the price -K^(1 + gamma) cap"""
    gammas = np.array([-1.0, 0.7, -0.2])
    shortcut = np.array([1, 0, 0], dtype=np.int32)
    phis, lms = [], []
    for s, v in enumerate((0.16, 0.05, 0.3)):
        phi, lm = synthetic_grid(n, v, seed=10 + s)
        phis.append((0.5 + gammas[s]) + 1j * phi.imag if shortcut[s] else (-0.5 + 0.1 * s) + 1j * phi.imag)
        lms.append(lm)
    phi, lm = np.stack(phis), np.stack(lms)
    dphi, dlm = Dev(L, phi), Dev(L, lm)
    norm, gfwd = Dev(L, np.ones(3)), Dev(L, np.zeros(3))
    forward, worst = 1.1, 0.0
    for k in (1, 32, 33, 65):
        strikes = forward * np.exp(np.linspace(-0.5, 0.5, k))
        codes = np.zeros(k, dtype=np.int32)
        out = Dev(L, n_doubles=3 * k)
        _check(L.svmc_mgf_gamma_slice_batch(dphi.ptr, dlm.ptr, n, 3, _pf(gammas), shortcut.ctypes.data_as(C.POINTER(C.c_int)),
                                            norm.ptr, gfwd.ptr, 0, forward, _pf(strikes),
                                            codes.ctypes.data_as(C.POINTER(C.c_int)), k, out.ptr, None))
        got = out.get((3, k), np.float64)
        for s in range(3):
            x_all = np.array([math.log(forward / float(K)) for K in strikes])
            h = phi[s, 1].imag - phi[s, 0].imag
            dp = h / 3 * simpson_weights(n) / np.pi
            w = dp / (phi[s].imag ** 2 + 0.25) if shortcut[s] else -dp / ((phi[s] + gammas[s] + 1) * (phi[s] + gammas[s]))
            t = (w[None, :] * np.exp(lm[s][None, :] - x_all[:, None] * phi[s][None, :])).real
            kg_np = strikes ** (1 + gammas[s])
            np_sum_check(f"gamma n={n} k={k} set={s}", -got[s] / kg_np, (t.sum(axis=1), np.abs(t).sum(axis=1)))
            for i in checked_strikes(k):
                K = strikes[i]
                x = x_all[i]
                val, absum, absum_a = gamma_ref(phi[s], lm[s], x, gammas[s], bool(shortcut[s]))
                with mp.workdps(50):
                    kg = mp.mpf(float(K)) ** (1 + mp.mpf(gammas[s]))
                    err = abs(mp.mpf(got[s, i]) + kg * val)
                    # the price's pow and product: a few more roundings of |K^(1 + gamma) cap|
                    bound = kg * (EPS * (C_SUM * n * absum + 2 * absum_a) + 4 * EPS * abs(val))
                assert err <= bound, (n, k, s, i, float(err), float(bound))
                worst = max(worst, float(err / bound))
    report(f"gamma slice n={n} error / bound", worst, 1.0)


# ---- the density slices against the exact sum ----------------------------------------------------------------------------
# The sums are written from the reference: utils/mgf_pricer.py:375-383 (pdf_with_mgf_grid: dx nansum Re[(dp / pi) exp(z u +
# log E)], z = (space - shift) / scale) and :244-253 (digital_slice_pricer_with_mgf_grid: nansum Re[-+(dp / pi) / phi
# exp(-x phi + log E)]), dp the legacy weights of :157-171 -- Simpson's, or 0.5 (p_1 - p_0) on the first point and p_j - p_(j-1)
# on the others.  The same error model as above, unchanged; the density's final product with dx is one more rounding of the
# result.
MAX_PDF_SETS = 64              # csrc/svmc_density.hip


def density_grid(n, vol_scaler, spot, seed, is_simpson):
    """synthetic_grid, its spacing stretched geometrically (the last step e^2 times the first) for the local-step weights"""
    phi, lm = synthetic_grid(n, vol_scaler, spot=spot, seed=seed)
    if is_simpson:
        return phi, lm
    p = phi.imag[-1] * np.expm1(2.0 * np.linspace(0.0, 1.0, n)) / math.expm1(2.0)
    rng = np.random.default_rng(seed)
    lm = -0.5 * (vol_scaler * p) ** 2 * (1 + 0.1 * rng.uniform(size=n)) + 1j * 0.3 * p * rng.uniform(size=n)
    return phi.real + 1j * p, lm


def dp_mp(grid, j, is_simpson):
    """the legacy weight dp_j in mp from the grid's doubles (the Simpson step h as the double the reference forms)"""
    n, p = grid.size, grid.imag
    if is_simpson:
        return mp.mpf(p[1] - p[0]) / 3 * legacy_weight(j, n)
    return (mp.mpf(p[1]) - mp.mpf(p[0])) / 2 if j == 0 else mp.mpf(p[j]) - mp.mpf(p[j - 1])


def dp_np(grid, is_simpson):
    p = grid.imag
    if is_simpson:
        return (p[1] - p[0]) / 3 * simpson_weights(grid.size)
    return np.append(0.5 * (p[1] - p[0]), p[1:] - p[:-1])


def pdf_ref(u, lm, z, is_simpson):
    """the sum of :381 at one z (a double, formed as the reference forms it), before the product with dx"""
    with mp.workdps(50):
        return mp_sum([_term(mp.mpc(dp_mp(u, j, is_simpson) / mp.pi), lm[j], -z, u[j]) for j in range(u.size)])


def pdf_np(u, lm, z, is_simpson):
    t = (dp_np(u, is_simpson)[None, :] / np.pi * np.exp(z[:, None] * u[None, :] + lm[None, :])).real
    return t.sum(axis=1), np.abs(t).sum(axis=1)


def check_pdf(name, dev, ref, dx, n):
    """check_sum for dx * sum: the bound scaled by |dx|, plus the product's own rounding"""
    val, absum, absum_a = ref
    if mp.isinf(val):
        assert dev == float(val) * math.copysign(1.0, dx), (name, dev, val)
        return 0.0
    with mp.workdps(50):
        err = abs(mp.mpf(dev) - mp.mpf(dx) * val)
        bound = abs(mp.mpf(dx)) * (EPS * (C_SUM * n * absum + 2 * absum_a) + EPS * abs(val))
    assert err <= bound, (name, float(err), float(bound))
    return float(err / bound) if bound > 0 else 0.0


def pdf_batch(L, u, lm, space, shifts, scales, is_simpson):
    """svmc_mgf_pdf_slice_batch on [n_sets][n_grid] grids and [n_sets][n_space] space grids -> [n_sets][n_space]"""
    u, lm, space = (np.ascontiguousarray(np.atleast_2d(v)) for v in (u, lm, space))
    shifts, scales = (np.ascontiguousarray(np.atleast_1d(v), dtype=np.float64) for v in (shifts, scales))
    s, n = u.shape
    du, dlm, dsp, out = Dev(L, u), Dev(L, lm), Dev(L, space), Dev(L, n_doubles=space.size)
    _check(L.svmc_mgf_pdf_slice_batch(du.ptr, dlm.ptr, n, s, dsp.ptr, space.shape[1], _pf(shifts), _pf(scales), int(is_simpson),
                                      out.ptr, None))
    return out.get(space.shape, np.float64)


def pdf_set(n, i, is_simpson, n_space):
    """set i of a pdf batch: its own grid, space grid, shift and scale (every third scale negative)"""
    v = (0.16, 0.05, 0.3)[i % 3] * (1.0 + 0.03 * (i // 3))
    u, lm = density_grid(n, v, spot=bool(i % 2), seed=100 + i, is_simpson=is_simpson)
    scale = (-1.0 if i % 3 == 1 else 1.0) * v * (1.5 + 0.1 * (i % 5))
    shift = 0.01 * (i % 7) - 0.02
    space = shift + abs(scale) * np.linspace(-2.5 + 0.1 * (i % 4), 2.0, n_space)
    return u, lm, space, shift, scale


@pytest.mark.parametrize("is_simpson", [1, 0])
@pytest.mark.parametrize("n", [3, 4, 255, 256, 257, 1000, 1001])
def test_pdf_slice_kernel_vs_exact_sum(L, n, is_simpson):
    """three sets, each its own grid, space grid, shift and scale (one scale negative); 2 and 33 space points"""
    worst = 0.0
    for n_space in (2, 33):
        sets = [pdf_set(n, i, is_simpson, n_space) for i in range(3)]
        assert any(s[4] < 0 for s in sets)
        got = pdf_batch(L, *(np.stack([s[k] for s in sets]) for k in range(3)), [s[3] for s in sets], [s[4] for s in sets],
                        is_simpson)
        for i, (u, lm, space, shift, scale) in enumerate(sets):
            z = (space - shift) / scale                                   # :379, in double as the reference
            dx = space[1] - space[0]
            val, absum = pdf_np(u, lm, z, is_simpson)
            np_sum_check(f"pdf n={n} simpson={is_simpson} n_space={n_space} set={i}", got[i], (dx * val, abs(dx) * absum))
            for k in (0, n_space - 1):
                worst = max(worst, check_pdf(f"pdf n={n} simpson={is_simpson} n_space={n_space} set={i} point={k}", got[i, k],
                                             pdf_ref(u, lm, float(z[k]), is_simpson), float(dx), n))
    report(f"pdf slice n={n} simpson={is_simpson} error / bound", worst, 1.0)


@pytest.mark.parametrize("n_sets", [MAX_PDF_SETS, MAX_PDF_SETS + 1, 2 * MAX_PDF_SETS + 1])
def test_pdf_slice_sets_across_the_launch_boundary(L, n_sets):
    """64 sets a launch: set s of the batch equals its single call bit for bit; the first and the last set against mp"""
    n, n_space, worst = 4, 3, 0.0
    for is_simpson in (1, 0):
        sets = [pdf_set(n, i, is_simpson, n_space) for i in range(n_sets)]
        got = pdf_batch(L, *(np.stack([s[k] for s in sets]) for k in range(3)), [s[3] for s in sets], [s[4] for s in sets],
                        is_simpson)
        for i, (u, lm, space, shift, scale) in enumerate(sets):
            np.testing.assert_array_equal(got[i], pdf_batch(L, u, lm, space, shift, scale, is_simpson)[0],
                                          err_msg=f"{n_sets} sets, set {i}, simpson {is_simpson}")
        for i in (0, n_sets - 1):
            u, lm, space, shift, scale = sets[i]
            z = (space - shift) / scale
            for k in range(n_space):
                worst = max(worst, check_pdf(f"pdf {n_sets} sets, set {i}, point {k}", got[i, k],
                                             pdf_ref(u, lm, float(z[k]), is_simpson), float(space[1] - space[0]), n))
    report(f"pdf slice, {n_sets} sets, error / bound", worst, 1.0)


def digital_ref(phi, lm, x, negative_contour, is_simpson):
    """the sum of :253 for one x, with the payoff transform of :244 (calls, Re phi < 0) or :247 (puts)"""
    with mp.workdps(50):
        sign = -1 if negative_contour else 1
        return mp_sum([_term(sign * (dp_mp(phi, j, is_simpson) / mp.pi) / mp.mpc(phi[j]), lm[j], x, phi[j])
                       for j in range(phi.size)])


def digital_np(phi, lm, x, negative_contour, is_simpson):
    pw = (-1.0 if negative_contour else 1.0) * (dp_np(phi, is_simpson) / np.pi) / phi
    t = (pw[None, :] * np.exp(lm[None, :] - x[:, None] * phi[None, :])).real
    return t.sum(axis=1), np.abs(t).sum(axis=1)


def digital_batch(L, phi, lm, forward, strikes, negative_contour, is_simpson):
    """svmc_mgf_digital_slice_batch: phi, log E [n_sets][n_grid], the same strikes and forward for every set -> [n_sets][k]"""
    phi, lm = np.ascontiguousarray(np.atleast_2d(phi)), np.ascontiguousarray(np.atleast_2d(lm))
    strikes = np.ascontiguousarray(strikes, dtype=np.float64)
    s, n = phi.shape
    dphi, dlm, out = Dev(L, phi), Dev(L, lm), Dev(L, n_doubles=s * strikes.size)
    _check(L.svmc_mgf_digital_slice_batch(dphi.ptr, dlm.ptr, n, s, float(forward), _pf(strikes), strikes.size,
                                          int(negative_contour), int(is_simpson), out.ptr, None))
    return out.get((s, strikes.size), np.float64)


@pytest.mark.parametrize("is_simpson", [1, 0])
@pytest.mark.parametrize("spot", [True, False])
@pytest.mark.parametrize("n", [3, 4, 255, 256, 257, 1000, 1001])
def test_digital_slice_kernel_vs_exact_sum(L, n, spot, is_simpson):
    """three sets on grids of different spacing, Re phi = -0.5 (the calls' contour) or +0.5 (the puts'), Im phi from 0: the
    first points have |Re phi| >= |Im phi| and the rest do not, so both arms of the Smith division are taken"""
    grids = [density_grid(n, v, spot, 20 + i, is_simpson) for i, v in enumerate((0.16, 0.05, 0.3))]
    phi, lm = np.stack([g[0] for g in grids]), np.stack([g[1] for g in grids])
    first_arm = np.abs(phi.real) >= np.abs(phi.imag)
    assert np.all(first_arm.any(axis=1)) and np.all((~first_arm).any(axis=1)), "one arm of the Smith division is not taken"
    negative_contour = bool(np.all(phi.real < 0.0))                       # :242
    assert negative_contour == spot
    forward, worst = 1.3, 0.0
    for k in (1, 32, 33, 65):
        strikes = forward * np.exp(np.linspace(-0.6, 0.6, k))
        got = digital_batch(L, phi, lm, forward, strikes, negative_contour, is_simpson)
        x = np.array([math.log(forward / float(K)) for K in strikes])
        for s in range(3):
            name = f"digital n={n} spot={spot} simpson={is_simpson} k={k} set={s}"
            np_sum_check(name, got[s], digital_np(phi[s], lm[s], x, negative_contour, is_simpson))
            for i in checked_strikes(k):
                worst = max(worst, check_sum(f"{name} strike={i}", got[s, i],
                                             digital_ref(phi[s], lm[s], x[i], negative_contour, is_simpson), n))
    report(f"digital slice n={n} spot={spot} simpson={is_simpson} error / bound", worst, 1.0)


NANSUM_EDITS = {"nan": {5: complex(np.nan, 0.0)}, "neg_inf": {5: complex(-np.inf, 0.0), 200: complex(-np.inf, 0.0)},
                "pos_inf": {7: complex(np.inf, 0.0)}}


@pytest.mark.parametrize("is_simpson", [1, 0])
def test_pdf_slice_kernel_nansum_contract(L, is_simpson):
    """NaN terms dropped, +inf kept, a -inf log E a zero term.  z = 0 first: the inf term's phase is exactly 0"""
    n = 257
    u, lm = density_grid(n, 0.16, True, 0, is_simpson)
    shift, scale = 0.05, 0.2
    space = np.array([shift, shift + 0.07, shift - 0.11])
    z = (space - shift) / scale
    assert z[0] == 0.0
    dx = float(space[1] - space[0])
    for name, edits in NANSUM_EDITS.items():
        e = lm.copy()
        for j, v in edits.items():
            e[j] = v
        got = pdf_batch(L, u, e, space, shift, scale, is_simpson)[0]
        for i in range(space.size):
            ref = pdf_ref(u, e, float(z[i]), is_simpson)
            if name == "pos_inf":
                assert np.isinf(got[i]) and got[i] == float(ref[0]), (i, got[i], ref[0])
                assert i > 0 or got[i] == np.inf
            else:
                assert np.isfinite(got[i]), (name, got[i])
                check_pdf(f"pdf {name} point {i}", got[i], ref, dx, n)


@pytest.mark.parametrize("is_simpson", [1, 0])
@pytest.mark.parametrize("spot", [True, False])
def test_digital_slice_kernel_nansum_contract(L, spot, is_simpson):
    """as above.  The weight p = -+(dp / pi) / phi is complex here: Re p > 0 on both contours, Im p > 0 for the calls (Re phi
    < 0) and < 0 for the puts.  A +inf log E at point 7 gives Re[p] inf cos(theta) - Im[p] inf sin(theta) with the phase theta
    = -x Im phi_7, as NumPy's product.  The strikes, in order:
      strike == forward, x = 0: theta is exactly 0, the exponential is (inf, 0) and the sum +inf (the sign of Re p);
      theta = -+0.7 and +-2.4: both parts have the same sign, the sum is +inf and -inf;
      0.8: theta < 0 in the fourth quadrant -- the parts agree for the calls (+inf) and are inf - inf = NaN for the puts, a term
      that nansum drops: the sum of the other terms"""
    n = 257
    phi, lm = density_grid(n, 0.16, spot, 0, is_simpson)
    forward = 1.0
    theta = (-0.7, 2.4) if spot else (0.7, -2.4)
    strikes = np.array([forward] + [forward * math.exp(t / phi[7].imag) for t in theta] + [0.8])
    x = np.array([math.log(forward / float(K)) for K in strikes])
    assert x[0] == 0.0
    pos_inf = (np.inf, np.inf, -np.inf, np.inf if spot else None)
    for name, edits in NANSUM_EDITS.items():
        e = lm.copy()
        for j, v in edits.items():
            e[j] = v
        got = digital_batch(L, phi, e, forward, strikes, spot, is_simpson)[0]
        for i in range(strikes.size):
            ref = digital_ref(phi, e, float(x[i]), spot, is_simpson)
            if name == "pos_inf" and pos_inf[i] is not None:
                assert got[i] == pos_inf[i] and got[i] == float(ref[0]), (i, got[i], ref[0])
            else:
                assert np.isfinite(got[i]) and mp.isfinite(ref[0]), (name, i, got[i], ref[0])
                check_sum(f"digital {name} strike {i}", got[i], ref, n)


# ---- the five slice kernels against their recorded bits -------------------------------------------------------------------
# tests/golden/mgf_slice_bits.npz holds, per grid length n, the imaginary parts p_n [3][n] of three transform grids and their
# log E lm_n [3][n] (NaN, -inf and +inf planted at n = 257), and per case the rows of them it takes (`sets`), the grids' real
# parts, the entry point's small arguments and the output the library gave when the fixture was made.
SLICE_KERNELS = ("vanilla", "qvar", "gamma", "pdf", "digital")


def slice_case_output(L, g, c):
    """case `c` (an entry of the fixture's index) through its C entry point -> the doubles it wrote"""
    key, n = c["id"] + "/", c["n"]
    sets = g[key + "sets"]
    grid = np.empty((sets.size, n), dtype=np.complex128)
    grid.real = g[key + "re"][:, None]
    grid.imag = g[f"p_{n}"][sets]
    lm = np.ascontiguousarray(g[f"lm_{n}"][sets])
    s = sets.size
    if c["kernel"] == "pdf":
        return pdf_batch(L, grid, lm, g[key + "space"], g[key + "shifts"], g[key + "scales"], c["is_simpson"])
    strikes = np.ascontiguousarray(g[key + "strikes"])
    k = strikes.size
    if c["kernel"] == "digital":
        return digital_batch(L, grid, lm, c["forward"], strikes, c["negative_contour"], c["is_simpson"])
    dgrid, dlm, out = Dev(L, grid), Dev(L, lm), Dev(L, n_doubles=s * k)
    if c["kernel"] == "vanilla":
        _check(L.svmc_mgf_vanilla_slice_batch(dgrid.ptr, dlm.ptr, n, s, c["forward"], _pf(strikes), k, out.ptr, None))
    elif c["kernel"] == "qvar":
        assert s == 1
        _check(L.svmc_mgf_qvar_slice(dgrid.ptr, dlm.ptr, n, c["ttm"], _pf(strikes), k, out.ptr, None))
    else:
        gammas, shortcut, codes = (np.ascontiguousarray(g[key + v]) for v in ("gammas", "shortcut", "codes"))
        norm, gfwd = Dev(L, g[key + "normalizers"]), Dev(L, g[key + "gamma_forwards"])
        pi = C.POINTER(C.c_int)
        _check(L.svmc_mgf_gamma_slice_batch(dgrid.ptr, dlm.ptr, n, s, _pf(gammas), shortcut.ctypes.data_as(pi), norm.ptr,
                                            gfwd.ptr, 0, c["forward"], _pf(strikes), codes.ctypes.data_as(pi), k, out.ptr, None))
    return out.get((s, k), np.float64)


@pytest.mark.parametrize("kernel", SLICE_KERNELS)
def test_slice_kernels_bit_equal_to_recorded(L, kernel):
    """raw bits, so NaN and the sign of zero count"""
    g = np.load(os.path.join(HERE, "golden", "mgf_slice_bits.npz"))
    cases_ = [c for c in json.loads(str(g["index"])) if c["kernel"] == kernel]
    assert {c["n"] for c in cases_} == {3, 256, 257, 1001}
    for c in cases_:
        got, want = slice_case_output(L, g, c), g[c["id"] + "/out"]
        assert got.shape == want.shape, c["id"]
        differ = np.flatnonzero(got.view(np.uint64).ravel() != want.view(np.uint64).ravel())
        assert differ.size == 0, (c["id"], differ[:8], got.ravel()[differ[:8]], want.ravel()[differ[:8]])
