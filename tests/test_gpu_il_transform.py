"""
The transform side of the impermanent-loss pricer on the device:

  * mgf_il_slice_kernel's five sums against the same sums in 50-digit mpmath from the same doubles, in the form of
    test_gpu_transform_odes.py: synthetic_grid moved to the contour Re phi = -0.4, grid lengths around the 256-thread stride,
    the Simpson rule on the odd lengths and the trapezoid rule on all, case counts across the 32-case chunk, three sets with
    different spacings; every case against the float64 sum at 1e-12 sum |t|, the chunk ends against mpmath;
  * the nansum contract (a planted NaN, -inf and +inf in log E), a case in company bit-equal to the case alone;
  * on the reference's own stored log-MGF (tests/golden/il_payoff.npz) each sum against the reference's at 1e-12 sum |t|;
  * logsv_il_pricer end to end against the tight fixture, piece by piece and as the composite; the vector call against scalar
    calls and the batch against single calls, bit for bit.

Every report() line prints the measured worst value against its bound (run with -s).
"""
import math
import os

import mpmath as mp
import numpy as np
import pytest

from test_gpu_transform_odes import (C_SUM, EPS, ODE_ATOL, ODE_BOUND, ODE_RTOL, Dev, _check, _pf, _term, checked_strikes, dp_mp, dp_np,
                                     mp_sum, np_sum_check, report, synthetic_grid)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RE_PHI = -0.4
# The error model of test_gpu_transform_odes.py, |dev - ref| <= 2^-53 (C n sum |t_j| + 2 sum |t_j| a_j), with the constants of
# the new terms:
#   vanilla on a general contour, w = -(dp / pi) / ((phi + 1) phi): the complex product (phi + 1) phi (4 roundings) and the
#   Smith division (6) stand where the family's real weight has 3; with cexp_ (5), the term's product (3) and the weight (3) a
#   term carries at most 21 roundings, the sum n / 256 + 9 as there: 21 + n / 256 + 9 <= 12 n for n >= 3.  C_IL = 12 for all
#   five sums (the digital ones are the family's and need 8).
#   a_j for the vanilla and digital sums: the family's, |Re log E| + |Im log E| + |x - xa| (|Re phi| + |Im phi|).
#   square root: t_j = t_bj - t_aj, t_cj = Re[(v_j / pi) exp((phi + 1/2) xc - phi x) / (phi + 1/2) exp(log E_j)], and the two
#   cancel (at Im phi = 0 they are sqrt(pb) and sqrt(pa) times the same factor), so |t_j| is |t_bj| + |t_aj| with the MODULI of
#   the two complex products -- Re of a difference is bounded by the moduli, not by the real parts.  Per term the two cexp_, the
#   difference, the product with v / pi, the Smith division of two complex numbers (8) and the last product: at most 30
#   roundings of |t_bj| + |t_aj|; 30 + n / 256 + 9 <= 14 n for n >= 3: C_ROOT = 14.
#   a_cj = |Re log E| + |Im log E| + (|Re phi + 1/2| + |Im phi|) |xc| + (|Re phi| + |Im phi|) |x|: the exponent is formed in
#   double from products of that size (log prices are 7 to 8, so this term dominates the bound at the far grid points).
C_IL, C_ROOT = 12.0, 14.0
assert C_IL >= C_SUM


@pytest.fixture(scope="module")
def L():
    from stochvolmodels_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "il_payoff.npz"))


def il_batch(L, phi, lm, x, xa, xb, is_simpson):
    """svmc_mgf_il_slice_batch on [n_sets][n_grid] grids -> [n_sets][n_cases][5]"""
    phi, lm = np.ascontiguousarray(np.atleast_2d(phi)), np.ascontiguousarray(np.atleast_2d(lm))
    x, xa, xb = (np.ascontiguousarray(v, dtype=np.float64) for v in (x, xa, xb))
    s, n = phi.shape
    dphi, dlm, out = Dev(L, phi), Dev(L, lm), Dev(L, n_doubles=s * x.size * 5)
    _check(L.svmc_mgf_il_slice_batch(dphi.ptr, dlm.ptr, n, s, _pf(x), _pf(xa), _pf(xb), x.size, int(is_simpson), out.ptr, None))
    return out.get((s, x.size, 5), np.float64)


def validated_np(grid, is_simpson):
    """compute_integration_weights (utils/mgf_pricer.py:97-155)"""
    if is_simpson:
        return dp_np(grid, True)
    h = grid.imag[1] - grid.imag[0]
    w = np.full(grid.size, h)
    w[0] = w[-1] = 0.5 * h
    return w


def validated_mp(grid, j, is_simpson):
    if is_simpson:
        return dp_mp(grid, j, True)
    h = mp.mpf(grid.imag[1] - grid.imag[0])
    return h / 2 if j in (0, grid.size - 1) else h


def il_np(phi, lm, x, xa, xb, is_simpson):
    """the five sums in float64 for arrays of cases -> (sums [k][5], sum |t| [k][5])"""
    v = validated_np(phi, is_simpson) / np.pi
    w = dp_np(phi, is_simpson) / np.pi
    with np.errstate(all="ignore"):
        e = np.exp(lm)[None, :]
        f, fh = phi[None, :], phi[None, :] + 0.5
        tb = v * np.exp(fh * xb[:, None] - f * x[:, None]) / fh * e
        ta = v * np.exp(fh * xa[:, None] - f * x[:, None]) / fh * e
        out, absum = [(tb - ta).real.sum(axis=1)], [(np.abs(tb) + np.abs(ta)).sum(axis=1)]
        for weight, xc in ((-w / ((phi + 1.0) * phi), xa), (-w / ((phi + 1.0) * phi), xb), (w / phi, xa), (w / phi, xb)):
            t = (weight[None, :] * np.exp(lm[None, :] - (x - xc)[:, None] * f)).real
            out.append(t.sum(axis=1))
            absum.append(np.abs(t).sum(axis=1))
    return np.stack(out, axis=1), np.stack(absum, axis=1)


def root_term(v, lm, x, xa, xb, z):
    """((t_bj - t_aj) in mp, |t_bj| + |t_aj|, |t_bj| a_bj + |t_aj| a_aj); NaN, -inf and +inf in log E as _term treats them -- at
    Re log E = +inf the exponential of log E is (inf cos, inf sin) of ITS phase, (inf, 0) at a phase of exactly 0"""
    if math.isnan(lm.real) or math.isnan(lm.imag):
        return mp.nan, 0, 0
    if lm.real == -math.inf:
        return mp.mpf(0), 0, 0
    zc, zh = mp.mpc(z), mp.mpc(z) + mp.mpf(1) / 2
    base = abs(lm.real) + abs(lm.imag) + (abs(z.real) + abs(z.imag)) * abs(x)
    p = [v * mp.exp(zh * mp.mpf(xc) - zc * mp.mpf(x)) / zh for xc in (xb, xa)]
    if lm.real == math.inf:
        d = p[0] - p[1]
        parts = {mp.sign(u) for u in (d.real * mp.cos(lm.imag), -d.imag * mp.sin(lm.imag))} - {0}
        return (mp.inf * parts.pop() if len(parts) == 1 else mp.nan), 0, 0
    e = mp.exp(mp.mpc(lm))
    tb, ta = p[0] * e, p[1] * e
    a = [base + (abs(z.real + 0.5) + abs(z.imag)) * abs(xc) for xc in (xb, xa)]
    return (tb - ta).real, abs(tb) + abs(ta), abs(tb) * a[0] + abs(ta) * a[1]


def il_ref(phi, lm, x, xa, xb, is_simpson):
    """the five sums of one case in mp -> [(value, sum |t|, sum |t| a)] x 5.  x - xa and x - xb are the doubles the kernel forms"""
    n = phi.size
    with mp.workdps(50):
        vals, absum, absum_a = [], mp.mpf(0), mp.mpf(0)
        for j in range(n):
            t, m, ma = root_term(validated_mp(phi, j, is_simpson) / mp.pi, lm[j], x, xa, xb, phi[j])
            vals.append(t)
            if mp.isfinite(t):
                absum += m
                absum_a += ma
        keep = [t for t in vals if not mp.isnan(t)]
        out = [(mp.fsum(keep), absum, absum_a)]
        for vanilla, xc in ((True, xa), (True, xb), (False, xa), (False, xb)):
            terms = []
            for j in range(n):
                dp_pi = dp_mp(phi, j, is_simpson) / mp.pi
                z = mp.mpc(phi[j])
                terms.append(_term(-dp_pi / ((z + 1) * z) if vanilla else dp_pi / z, lm[j], x - xc, phi[j]))
            out.append(mp_sum(terms))
    return out


def check_il_sum(name, dev, ref, n, c):
    val, absum, absum_a = ref
    if mp.isinf(val):
        assert dev == float(val), (name, dev, val)
        return 0.0
    err = abs(mp.mpf(dev) - val)
    bound = EPS * (c * n * absum + 2 * absum_a)
    assert err <= bound, (name, float(err), float(bound))
    return float(err / bound) if bound > 0 else 0.0


# one list of 65 cases; a call of k cases takes the first k, so a chunk end's reference serves every count it appears in
K_ALL = 65
P1 = 2200.0 * np.exp(np.linspace(-0.15, 0.15, K_ALL))
PA = 2000.0 * (1.0 - 0.001 * np.arange(K_ALL))
PB = 2400.0 * (1.0 + 0.002 * np.arange(K_ALL))
X, XA, XB = np.log(P1), np.log(PA), np.log(PB)


def il_grids(n):
    grids = [synthetic_grid(n, v, seed=40 + i) for i, v in enumerate((0.16, 0.05, 0.3))]
    return np.stack([RE_PHI + 1j * g[0].imag for g in grids]), np.stack([g[1] for g in grids])


@pytest.mark.parametrize("n,is_simpson", [(n, 1) for n in (3, 5, 255, 257, 1001)] + [(n, 0) for n in (3, 4, 5, 255, 256, 257, 1001)])
def test_il_slice_kernel_vs_exact_sums(L, n, is_simpson):
    """three sets, case counts across the 32-case chunk; both arms of the Smith divisions are taken (|Re| >= |Im| at the first
    grid points only)"""
    phi, lm = il_grids(n)
    first_arm = np.abs(phi.real) >= np.abs(phi.imag)
    assert np.all(first_arm.any(axis=1)) and np.all((~first_arm).any(axis=1))
    refs, worst = {}, [0.0, 0.0]
    for k in (1, 32, 33, 65):
        got = il_batch(L, phi, lm, X[:k], XA[:k], XB[:k], is_simpson)
        for s in range(3):
            val, absum = il_np(phi[s], lm[s], X[:k], XA[:k], XB[:k], is_simpson)
            for q in range(5):
                np_sum_check(f"il n={n} simpson={is_simpson} k={k} set={s} sum={q}", got[s, :, q], (val[:, q], absum[:, q]))
            for i in checked_strikes(k):
                if (s, i) not in refs:
                    refs[s, i] = il_ref(phi[s], lm[s], float(X[i]), float(XA[i]), float(XB[i]), is_simpson)
                for q in range(5):
                    r = check_il_sum(f"il n={n} simpson={is_simpson} k={k} set={s} case={i} sum={q}", got[s, i, q], refs[s, i][q], n,
                                     C_ROOT if q == 0 else C_IL)
                    worst[q > 0] = max(worst[q > 0], r)
    report(f"il slice n={n} simpson={is_simpson} square root error / bound", worst[0], 1.0)
    report(f"il slice n={n} simpson={is_simpson} vanilla and digital error / bound", worst[1], 1.0)


NANSUM_EDITS = {"nan": {5: complex(np.nan, 0.0)}, "neg_inf": {5: complex(-np.inf, 0.0), 200: complex(-np.inf, 0.0)},
                "pos_inf": {7: complex(np.inf, 0.0)}}


@pytest.mark.parametrize("is_simpson", [1, 0])
def test_il_slice_kernel_nansum_contract(L, is_simpson):
    """NaN terms dropped, a -inf log E a zero term, +inf kept: an infinite sum of the sign the product gives, or, where the
    product is inf - inf, a dropped term.  The first case has p1 == pa: x - xa = 0, the phase of the pa sums' term is exactly 0"""
    n = 257
    phi, lm = il_grids(n)
    phi, lm = phi[0], lm[0]
    x, xa, xb = np.array([XA[0], X[3], X[40]]), np.array([XA[0], XA[3], XA[40]]), np.array([XB[0], XB[3], XB[40]])
    seen_inf = 0
    for name, edits in NANSUM_EDITS.items():
        e = lm.copy()
        for j, v in edits.items():
            e[j] = v
        got = il_batch(L, phi, e, x, xa, xb, is_simpson)[0]
        for i in range(3):
            ref = il_ref(phi, e, float(x[i]), float(xa[i]), float(xb[i]), is_simpson)
            for q in range(5):
                tag = f"il {name} case {i} sum {q}"
                if name == "pos_inf" and mp.isinf(ref[q][0]):
                    assert got[i, q] == float(ref[q][0]), (tag, got[i, q], ref[q][0])
                    seen_inf += 1
                else:
                    assert np.isfinite(got[i, q]) and mp.isfinite(ref[q][0]), (tag, got[i, q], ref[q][0])
                    check_il_sum(tag, got[i, q], ref[q], n, C_ROOT if q == 0 else C_IL)
        if name == "pos_inf":                                           # the phase-0 terms: Re[w] inf, w = -(dp/pi)/((phi+1)phi) and +(dp/pi)/phi
            assert got[0, 1] == np.inf and got[0, 3] == -np.inf, got[0]
    assert seen_inf >= 5


def test_company_does_not_change_bits(L):
    n = 257
    phi, lm = il_grids(n)
    for is_simpson in (1, 0):
        full = il_batch(L, phi, lm, X, XA, XB, is_simpson)
        for i in (0, 31, 32, 64):
            alone = il_batch(L, phi, lm, X[i:i + 1], XA[i:i + 1], XB[i:i + 1], is_simpson)
            assert np.array_equal(alone[:, 0], full[:, i]), (is_simpson, i)
        for s in range(3):
            assert np.array_equal(il_batch(L, phi[s], lm[s], X, XA, XB, is_simpson)[0], full[s]), (is_simpson, s)


def fixture_cases(fx):
    pa, pb, p1 = fx["cases"].T
    return p1, np.full(3, float(fx["p0"])), pa, pb


def test_reference_log_mgf_sums_and_pieces(L, fx):
    """the reference's own tight log-MGF through the kernel: each of the five sums within 1e-12 of its sum |t| of the sum the
    reference formed, and so each piece (a strike or 1 times a sum)"""
    from stochvolmodels_amd.pricers.il_pricer import il_compose, il_reference_sums
    p1, p0, pa, pb = fixture_cases(fx)
    worst = 0.0
    for tag in fx["set_names"]:
        for t in range(fx["ttms"].size):
            phi, lm = fx[f"f_{tag}_{t}_phi"], fx[f"f_{tag}_{t}_log_mgf"]
            raw = il_batch(L, phi, lm, np.log(p1), np.log(pa), np.log(pb), 1)[0]
            sums = il_reference_sums(raw, True)
            _, absum = il_np(phi, lm, np.log(p1), np.log(pa), np.log(pb), 1)
            dev = np.abs(sums - fx[f"f_{tag}_{t}_sums"]) / absum
            worst = max(worst, float(dev.max()))
            _, pieces = il_compose(sums, p1, p0, pa, pb, float(fx["notional"]))
            scale = np.stack([absum[:, 0], np.ones(3), pa * absum[:, 1], pb * absum[:, 2], absum[:, 3], absum[:, 4]], axis=1)
            assert np.all(np.abs(pieces - fx[f"f_{tag}_{t}_pieces"]) <= 1e-12 * scale), (tag, t)
            assert np.array_equal(pieces[:, 1], fx[f"f_{tag}_{t}_pieces"][:, 1])             # the linear piece is host arithmetic
    report("il sums on the reference's log-MGF, |dev - ref| / sum |t|", worst, 1e-12)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
# Ten times the largest deviation from the tight fixture observed on the MI355X, rounded up to one digit
# (profiles/il_observed_tolerances.txt), the ODE at the rtol 1e-12 / atol 1e-14 at which test_gpu_transform_odes.py grants it
# ODE_BOUND; neither may exceed ODE_BOUND.  Pieces: |dev - ref| over the piece's own size (sqrt(pb), pa, pb, 1, 1); composite:
# over notional0 notional times the sum of the absolute terms of the payoff, IL being a difference of terms about a thousand
# times its size.
E2E_PIECE_BOUND, E2E_VALUE_BOUND = 7e-13, 3e-14             # observed 6.556e-14 and 2.206e-15
assert max(E2E_PIECE_BOUND, E2E_VALUE_BOUND) <= ODE_BOUND


def params_of(fx, tag):
    import stochvolmodels_amd as sv
    return sv.LogSvParams(**dict(zip(("sigma0", "theta", "kappa1", "kappa2", "beta", "volvol"), map(float, fx[f"{tag}_params"]))))


def test_logsv_il_pricer_against_the_tight_fixture(fx):
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.pricers.il_pricer import IL_PIECES, il_notional0
    p1, p0, pa, pb = fixture_cases(fx)
    notional = float(fx["notional"])
    worst_piece, worst_value = 0.0, 0.0
    for tag in fx["set_names"]:
        for t, ttm in enumerate(fx["ttms"]):
            value, pieces = sv.logsv_il_pricer(params_of(fx, tag), float(ttm), p1, p0, pa, pb, notional=notional, return_pieces=True,
                                               ode_rtol=ODE_RTOL, ode_atol=ODE_ATOL)
            got = np.stack([pieces[k] for k in IL_PIECES], axis=1)
            want = fx[f"f_{tag}_{t}_pieces"]
            size = np.stack([np.sqrt(pb), np.ones(3), pa, pb, np.ones(3), np.ones(3)], axis=1)
            dev_p = float(np.max(np.abs(got - want) / size))
            terms = np.abs(want) * np.stack([2 * np.ones(3), np.ones(3), 1 / np.sqrt(pa), 1 / np.sqrt(pb), 2 * np.sqrt(pa),
                                             2 * np.sqrt(pb)], axis=1)
            dev_v = float(np.max(np.abs(value - fx[f"f_{tag}_{t}_values"]) / (il_notional0(p0, pa, pb) * notional * terms.sum(axis=1))))
            print(f"il e2e {tag} ttm {ttm:.4f}: pieces {dev_p:.3e} value {dev_v:.3e}  values {value}")
            worst_piece, worst_value = max(worst_piece, dev_p), max(worst_value, dev_v)
    report("logsv_il_pricer pieces vs tight reference", worst_piece, E2E_PIECE_BOUND)
    report("logsv_il_pricer value vs tight reference", worst_value, E2E_VALUE_BOUND)


def test_vector_call_equals_scalar_calls(fx):
    import stochvolmodels_amd as sv
    params = params_of(fx, "paper")
    forwards = np.linspace(1900.0, 2500.0, 101)
    vec = sv.logsv_il_pricer_vector(params, 10.0 / 365.0, forwards, 2200.0, 2000.0, 2400.0)
    assert vec.shape == (101,) and np.all(np.isfinite(vec))
    for i in (0, 17, 31, 32, 50, 64, 100):
        one = sv.logsv_il_pricer(params, 10.0 / 365.0, float(forwards[i]), 2200.0, 2000.0, 2400.0)
        assert isinstance(one, float) and one == vec[i], (i, one, vec[i])
    every = np.array([sv.logsv_il_pricer(params, 10.0 / 365.0, float(f), 2200.0, 2000.0, 2400.0) for f in forwards])
    assert np.array_equal(every, vec)


def test_batch_sets_equal_single_calls(fx):
    import stochvolmodels_amd as sv
    p1, p0, pa, pb = fixture_cases(fx)
    sets = [params_of(fx, "cand"), params_of(fx, "paper"), sv.LogSvParams(sigma0=0.2, theta=0.22, kappa1=3.0, kappa2=12.0, beta=-0.3, volvol=0.4)]
    batch = sv.logsv_il_pricer_batch(sets, 0.25, p1, p0, pa, pb, return_pieces=True)
    for p, (value, pieces) in zip(sets, batch):
        v1, pc1 = sv.logsv_il_pricer(p, 0.25, p1, p0, pa, pb, return_pieces=True)
        assert np.array_equal(value, v1)
        for k in pieces:
            assert np.array_equal(pieces[k], pc1[k]), k
