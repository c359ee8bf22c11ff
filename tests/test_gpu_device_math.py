"""
The device build of the fp64 helpers every stepping, analytic and calibration kernel runs on, against high-precision
references (run with `-m gpu` on an MI355X).  tests/test_math_accuracy.py holds the same functions to their stated bounds on a
HOST build (g++, no contraction, single-precision stand-ins for the hardware seeds); here the code object is hipcc's, with the
v_rcp_f64 / v_rsq_f64 seeds, the fma_k inline assembly, v_ldexp_f64 saturation, the device libm (erfc, log, exp, sincos, atan2,
hypot) and the tables in LDS.  The whole-price GPU tests cannot see errors of this size: they compare with the CPU twin at
rtol 1e-11 .. 1e-12.

  - svmc_math.h and uniform_32 (svmc_rng.h): the sample sets, edge arrays and bounds of test_math_accuracy.py, 80-bit reference
  - normal_icdf32: the CPU twin bit for bit
  - svmc_complex.h: mpmath at 40 digits, componentwise error relative to |result|
  - heston_mgf_grid_kernel through compute_heston_mgf_grid: mpmath (tests/golden/device_math.npz) and NumPy's complex128
    evaluation of the same closed form
  - svmc_black.h: mpmath quotes (device_math.npz) and the host routine svmc_black_implied_vols

The helpers run in tests/native/libsvmc_device_probe.so (tests/native/device_math_probe.hip, built by
stochvolmodels_amd/build.py build_device_probe with the library's own flags).
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)
N = 400_000
TWO = np.longdouble(2.0)


@pytest.fixture(scope="module")
def probe():
    from stochvolmodels_amd import build as svbuild
    try:
        svbuild.hipcc()
        have_hipcc = True
    except RuntimeError:
        have_hipcc = False
    if have_hipcc and svbuild.probe_is_stale():
        try:
            svbuild.build_device_probe()
        except RuntimeError as exc:
            pytest.fail(f"device probe does not build: {exc}")
    if not os.path.exists(svbuild.PROBE_LIB):
        cmd = " ".join(svbuild.probe_command()) if have_hipcc else \
            "hipcc " + " ".join(svbuild.flags() + [svbuild.PROBE_SRC, "-o", svbuild.PROBE_LIB])
        pytest.fail(f"{svbuild.PROBE_LIB} is missing and cannot be built here; build it with:\n{cmd}")
    # libsvmc's loader imports torch first, so that the process holds ONE HIP runtime (stochvolmodels_amd/_lib.py): the probe
    # must resolve its libamdhip64 to that copy too -- a second copy left torch without devices for every later test
    from stochvolmodels_amd import _lib
    _lib.load()
    return C.CDLL(svbuild.PROBE_LIB)


def run(lib, name, x):
    """dprobe_<name> on the rows of x: the library's dprobe_shape_<name> gives the doubles per item in (nx) and out (ny)"""
    nx, ny = C.c_int(), C.c_int()
    getattr(lib, "dprobe_shape_" + name)(C.byref(nx), C.byref(ny))
    nx, ny = nx.value, ny.value
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    n = x.size // nx
    assert n * nx == x.size, (name, x.size, nx)
    y = np.full(n * ny, np.nan)
    rc = getattr(lib, "dprobe_" + name)(x.ctypes.data_as(DP), y.ctypes.data_as(DP), C.c_size_t(n))
    assert rc == 0, f"dprobe_{name}: hipError {rc}"
    return y if ny == 1 else y.reshape(n, ny)


def ulp(y, ref):
    ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.max(np.abs((np.asarray(y).astype(np.longdouble) - ref) / np.spacing(np.abs(ref.astype(np.float64))))))


def rel(y, ref):
    ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(y).astype(np.longdouble) / ref - 1)))


def report(name, value, bound):
    print(f"DEVICE-MAX {name}: {value:.4g} (bound {bound:.4g})")
    assert value <= bound, (name, value, bound)


# ---- svmc_math.h ------------------------------------------------------------------------------------------------------
def test_exp(probe):
    rng = np.random.default_rng(100)
    for lo, hi in ((-1, 1), (-30, 30), (-700, 700)):
        x = rng.uniform(lo, hi, N)
        report(f"exp_fast [{lo},{hi}] ULP", ulp(run(probe, "exp", x), np.exp(x.astype(np.longdouble))), 2.0)
    got = run(probe, "exp", np.array([800.0, -800.0, np.nan, 0.0]))
    assert got[0] == np.inf and got[1] == 0.0 and np.isnan(got[2]) and got[3] == 1.0   # v_ldexp_f64 saturation


def test_exp_full(probe):
    rng = np.random.default_rng(101)
    for lo, hi in ((-1, 1), (-30, 30), (-708, 709.7)):
        x = rng.uniform(lo, hi, N)
        report(f"exp_full [{lo},{hi}] ULP", ulp(run(probe, "exp_full", x), np.exp(x.astype(np.longdouble))), 2.0)
    x = rng.uniform(-745.0, -708.0, 20000)                                # gradual underflow: denormal results
    got, ref = run(probe, "exp_full", x), np.exp(x)
    assert np.all(np.abs(got - ref) <= 2.0 * 4.9406564584124654e-324 + 4e-16 * ref)
    edge = np.array([709.78, 709.79, 745.9, 746.0, 746.1, 1e4, 1e300, np.inf, -745.13, -745.2, -746.0, -746.1, -1e4, -1e300,
                     -np.inf, 0.0])
    with np.errstate(over="ignore", under="ignore"):
        want = np.exp(edge)
    got = run(probe, "exp_full", edge)
    for g_, w_, x_ in zip(got, want, edge):
        assert (g_ == w_) or (np.isfinite(w_) and w_ > 0 and abs(g_ / w_ - 1) < 1e-15) or (w_ < 1e-320 and abs(g_ - w_) < 1e-322), \
            (x_, g_, w_)
    assert np.isnan(run(probe, "exp_full", np.array([np.nan]))[0])


def test_exp_tab(probe):
    rng = np.random.default_rng(102)
    for lo, hi, bound in ((-1, 1, 1.5), (-5, 5, 3.0), (-30, 30, 11.0)):
        x = rng.uniform(lo, hi, N)
        report(f"exp_tab [{lo},{hi}] ULP", ulp(run(probe, "exp_tab", x), np.exp(x.astype(np.longdouble))), bound)
    x = rng.uniform(-700, 700, N)
    report("exp_tab [-700,700] rel", rel(run(probe, "exp_tab", x), np.exp(x.astype(np.longdouble))), 3e-14)
    x = np.arange(-400, 401) * (np.log(2.0) / 256)                       # the table nodes, both sides of every rounding tie
    for eps in (0.0, 1e-17, -1e-17, 1.35e-3, -1.35e-3):
        report(f"exp_tab nodes{eps:+g} ULP", ulp(run(probe, "exp_tab", x + eps), np.exp((x + eps).astype(np.longdouble))), 1.5)
    got = run(probe, "exp_tab", np.array([800.0, -800.0, 0.0, np.nan]))
    assert got[0] == np.inf and got[1] == 0.0 and got[2] == 1.0 and np.isnan(got[3])


def test_exp2u_tab_and_its_split_forms(probe):
    """exp2u_tab(y) = 2^(y/256) <= 1.1 ULP at any size of y; exp2u_reduce + exp2u_tail + exp2u_scale, and exp2u_tail_v with
    exp2u_tail_consts(), give the same bits (the promise the several-states-per-lane generators rely on)"""
    rng = np.random.default_rng(103)
    ys = []
    for lo, hi in ((-400, 400), (-3000, 3000), (-250000, 250000)):
        y = rng.uniform(lo, hi, N)
        ys.append(y)
        report(f"exp2u_tab [{lo},{hi}] ULP", ulp(run(probe, "exp2u_tab", y), TWO ** (y.astype(np.longdouble) / 256)), 1.1)
    y = np.arange(-2000, 2001).astype(np.float64)                        # the table nodes and the rounding ties between them
    for eps in (0.0, 0.5, -0.5, 0.4999999, -0.4999999):
        ys.append(y + eps)
        report(f"exp2u_tab nodes{eps:+g} ULP", ulp(run(probe, "exp2u_tab", y + eps), TWO ** ((y + eps).astype(np.longdouble) / 256)),
               1.1)
    edge = np.array([0.0, -0.0, 256.0 * 1100, -256.0 * 1200, np.nan, np.inf, -np.inf, 1e-300, -5e-324, 0.5, -0.5])
    got = run(probe, "exp2u_tab", edge)
    assert got[0] == 1.0 and got[1] == 1.0 and got[2] == np.inf and got[3] == 0.0
    assert np.isnan(got[4]) and np.isnan(got[5])                         # as exp_tab: inf - inf in the reduction
    ys.append(edge)
    y = np.concatenate(ys)
    ref = run(probe, "exp2u_tab", y).view(np.uint64)
    np.testing.assert_array_equal(run(probe, "exp2u_split", y).view(np.uint64), ref)
    np.testing.assert_array_equal(run(probe, "exp2u_split_v", y).view(np.uint64), ref)


def test_neg_log(probe):
    rng = np.random.default_rng(104)
    u = rng.integers(0, 2 ** 52, N).astype(np.float64) * 2.0 ** -52 + 2.0 ** -53       # the RNG lattice
    report("neg_log lattice ULP", ulp(run(probe, "neg_log", u), -np.log(u.astype(np.longdouble))), 3.0)
    u = np.concatenate([2.0 ** -rng.uniform(0, 53, N), 1 - 2.0 ** -rng.uniform(1, 53, N), [2.0 ** -53, 1 - 2.0 ** -53, 0.5, np.sqrt(0.5)]])
    u = u[(u > 0) & (u < 1)]
    report("neg_log tails ULP", ulp(run(probe, "neg_log", u), -np.log(u.astype(np.longdouble))), 3.0)


def test_neg_log_tab(probe):
    rng = np.random.default_rng(105)
    u = rng.integers(0, 2 ** 52, N).astype(np.float64) * 2.0 ** -52 + 2.0 ** -53
    report("neg_log_tab lattice ULP", ulp(run(probe, "neg_log_tab", u), -np.log(u.astype(np.longdouble))), 2.0)
    u = np.concatenate([2.0 ** -rng.uniform(0, 53, N), 1 - 2.0 ** -rng.uniform(1, 53, N), [2.0 ** -53, 1 - 2.0 ** -53, 0.5, np.sqrt(0.5)]])
    u = u[(u > 0) & (u < 1)]
    report("neg_log_tab tails ULP", ulp(run(probe, "neg_log_tab", u), -np.log(u.astype(np.longdouble))), 2.0)
    hi = (0x3FE6A09E + np.arange(512, dtype=np.uint64) * 2048)
    ends = np.concatenate([(hi << np.uint64(32)), ((hi + np.uint64(2047)) << np.uint64(32)) | np.uint64(0xFFFFFFFF)]).view(np.float64)
    for scale in (1.0, 0.5, 2.0 ** -20):
        e = ends * scale
        e = e[e < 1.0]
        report(f"neg_log_tab interval ends x{scale:g} ULP", ulp(run(probe, "neg_log_tab", e), -np.log(e.astype(np.longdouble))), 2.0)
    assert run(probe, "neg_log_tab", np.array([1.0]))[0] == 0.0
    v = 2.0 ** rng.uniform(-30, 30, N)                                    # general arguments: absolute accuracy only
    err = np.abs(run(probe, "neg_log_tab", v).astype(np.longdouble) + np.log(v.astype(np.longdouble)))
    report("neg_log_tab general abs", float(err.max()), 4e-15)


def test_log_state(probe):
    rng = np.random.default_rng(106)
    for lo, hi in ((-3, 3), (-60, 60), (-1000, 1000)):
        s = 2.0 ** rng.uniform(lo, hi, N // 4)
        report(f"log_state 2^[{lo},{hi}] ULP", ulp(run(probe, "log_state", s), np.log(s.astype(np.longdouble))), 4.0)
    tiny = 2.0 ** rng.uniform(-1074, -1000, 2000)
    report("log_state denormal ULP", ulp(run(probe, "log_state", tiny), np.log(tiny.astype(np.longdouble))), 3.0)
    got = run(probe, "log_state", np.array([0.0, np.inf, np.nan, -1.0, -np.inf, 1.0, 5e-324, -0.0, -5e-324]))
    assert got[0] == -np.inf and got[1] == np.inf and np.isnan(got[2]) and np.isnan(got[3]) and np.isnan(got[4])
    assert got[5] == 0.0 and abs(got[6] - np.log(5e-324)) < 1e-12
    assert got[7] == -np.inf and np.isnan(got[8])                         # -0 >= 0: ln(-0) = -inf as libm; a negative denormal: NaN


def test_sqrt_family(probe):
    rng = np.random.default_rng(107)
    t = 2.0 ** rng.uniform(-60, 9, N)
    ref = np.sqrt(t.astype(np.longdouble))
    report("sqrt_pos ULP", ulp(run(probe, "sqrt_pos", t), ref), 1.0)
    report("sqrt_pos0 ULP", ulp(run(probe, "sqrt_pos0", t), ref), 1.0)
    # the Goldschmidt step alone: 1.5 e^2 of the hardware seed's error e (2^-24.2) -> 2^-47
    t = np.concatenate([2.0 ** rng.uniform(-53, 5.3, N), [1.1102230246251565e-16, 36.7368005696771]])
    ref = np.sqrt(t.astype(np.longdouble))
    g = run(probe, "sqrt_pos_1g", t)
    report("sqrt_pos_1g rel", rel(g, ref), 2.0 ** -47)
    report("sqrt_pos0_1g rel", rel(run(probe, "sqrt_pos0_1g", t), ref), 2.0 ** -47)
    gh = run(probe, "sqrt_pos_1g_h", t)
    np.testing.assert_array_equal(gh[:, 0], g)                          # the same sqrt, and half the rsq seed beside it
    report("sqrt_pos_1g_h half_rsq rel", rel(2.0 * gh[:, 1], 1 / ref), 2.0 ** -23)
    z = run(probe, "sqrt_pos0", np.array([0.0, -0.0]))
    z1 = run(probe, "sqrt_pos0_1g", np.array([0.0, -0.0]))
    assert np.all(z == 0.0) and np.all(z1 == 0.0)
    assert not np.isfinite(run(probe, "sqrt_pos", np.array([0.0]))[0])    # why the *0 forms exist: the rsq seed of 0 is inf


def test_rcp_family_and_seeds(probe):
    """rcp_fast: correctly rounded on the sampled range; rcp_1n (one Newton step on the seed): e^2 + rounding -> <= 2^-48;
    the raw seeds: <= 2^-23, the worst case every refinement step's comment is written for"""
    rng = np.random.default_rng(108)
    a = 2.0 ** rng.uniform(-20, 20, N) * rng.choice([-1.0, 1.0], N)
    ref = 1 / a.astype(np.longdouble)
    report("rcp_fast ULP", ulp(run(probe, "rcp_fast", a), ref), 1.0)
    report("rcp_1n rel", rel(run(probe, "rcp_1n", a), ref), 2.0 ** -48)
    a = np.concatenate([2.0 ** rng.uniform(-1000, 1000, N) * rng.choice([-1.0, 1.0], N), 1.0 + np.arange(4096) * 2.0 ** -12])
    report("rcp_seed rel", rel(run(probe, "rcp_seed", a), 1 / a.astype(np.longdouble)), 2.0 ** -23)
    t = np.concatenate([2.0 ** rng.uniform(-1000, 1000, N), 1.0 + np.arange(8192) * 2.0 ** -12])
    report("rsq_seed rel", rel(run(probe, "rsq_seed", t), 1 / np.sqrt(t.astype(np.longdouble))), 2.0 ** -23)


# ---- words to variates ------------------------------------------------------------------------------------------------
def test_normal_icdf32_is_the_twin_bit_for_bit(probe, oracle):
    from scipy.special import ndtri
    rng = np.random.default_rng(109)
    w = rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32)
    edges = np.concatenate([np.arange(-3, 4, dtype=np.int64) + (1 << e) for e in range(31)])
    w = np.concatenate([w, edges.astype(np.uint32), (-edges).astype(np.uint32), [0, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000]]).astype(np.uint32)
    z = run(probe, "normal_icdf32", w.astype(np.float64))
    twin = np.array([oracle.normal_from_word(int(v)) for v in w])
    np.testing.assert_array_equal(z.view(np.uint64), twin.view(np.uint64))
    t = w.view(np.int32).astype(np.float64)
    with np.errstate(divide="ignore"):
        exact = np.where(t == 0.0, 0.0, np.copysign(-ndtri(np.abs(t) * 2.0 ** -32), t))
    report("normal_icdf32 abs vs ndtri", float(np.max(np.abs(z - exact))), 1e-9)


def test_uniform_32_is_exact(probe):
    rng = np.random.default_rng(110)
    k = np.concatenate([[0, 1, 2 ** 31, 2 ** 32 - 1], rng.integers(0, 2 ** 32, 100000, dtype=np.uint64)]).astype(np.float64)
    got = run(probe, "uniform_32", k)
    np.testing.assert_array_equal(got, (k + 0.5) * 2.0 ** -32)           # exact in fp64 (k + 1/2 has 33 bits)
    assert got[0] == 2.0 ** -33 and got[3] == 1.0 - 2.0 ** -33


# ---- svmc_complex.h ---------------------------------------------------------------------------------------------------
# componentwise error relative to |result|, measured on the device (the bounds stated in svmc_complex.h)
CABS_BOUND, CDIV_BOUND, CEXP_BOUND, CSQRT_BOUND, CLOG_BOUND = 2.5e-16, 6e-16, 5e-16, 5e-16, 5e-16


def _mp():
    import mpmath
    mpmath.mp.dps = 40
    return mpmath


def _complex_inputs(rng, n=20000, lo=-8.0, hi=8.0):
    """all four quadrants at |z| = 10^[lo, hi], pure real and pure imaginary values of both signs, zeros, and the negative real
    axis with +0.0 and -0.0 imaginary parts"""
    r = 10.0 ** rng.uniform(lo, hi, n)
    ang = rng.uniform(-np.pi, np.pi, n)
    z = [r * np.cos(ang), r * np.sin(ang)]
    m = 10.0 ** rng.uniform(lo, hi, 500)
    re = np.concatenate([z[0], m, -m, 0 * m, 0 * m, -m, -m, [0.0, 0.0, -0.0, -0.0]])
    im = np.concatenate([z[1], 0 * m, 0 * m, m, -m, 0 * m, -0.0 * m, [0.0, -0.0, 0.0, -0.0]])
    return re, im


def _componentwise(got_re, got_im, want, floor=0.0):
    """max(|d re|, |d im|) / max(|want|, floor)"""
    mag = np.maximum(np.array([float(abs(w)) for w in want]), floor)
    d = np.array([max(abs(float(w.real) - a), abs(float(w.imag) - b)) if np.isfinite(a) and np.isfinite(b) else np.inf
                  for w, a, b in zip(want, got_re, got_im)])
    return d / mag


def test_cabs_csqrt_clog(probe):
    mp = _mp()
    rng = np.random.default_rng(111)
    re, im = _complex_inputs(rng)
    x = np.stack([re, im], axis=1)
    nz = (re != 0) | (im != 0)
    zs = [mp.mpc(a, b) for a, b in zip(re, im)]
    got = run(probe, "cabs", x)
    want = np.array([float(abs(z)) for z in zs])
    report("cabs_ rel", float(np.max(np.abs(got[nz] / want[nz] - 1))), CABS_BOUND)
    assert np.all(got[~nz] == 0.0)
    # clog_ = {log(cabs_(z)), atan2}: near |z| = 1 the real part is the log of a number within an ulp of 1, so its error is
    # absolute there -- measured against max(|result|, 1)
    for name, fn, npf, bound, floor in (("csqrt", mp.sqrt, np.sqrt, CSQRT_BOUND, 0.0), ("clog", mp.log, np.log, CLOG_BOUND, 1.0)):
        got = run(probe, name, x)
        want = [fn(z) for z in (zs[i] for i in np.flatnonzero(nz))]
        # mpmath has no signed zero: on the cut it takes the +0 side; -0 is the other side of the cut
        cut = (re[nz] < 0) & (im[nz] == 0) & np.signbit(im[nz])
        want = [w.conjugate() if c else w for w, c in zip(want, cut)]
        report(f"{name}_ componentwise", float(np.max(_componentwise(got[nz, 0], got[nz, 1], want, floor))), bound)
        # signed zeros on the real axis as NumPy gives them (the CPU twin and the reference compute with NumPy)
        axis = nz & (im == 0)
        ref = npf(np.array([complex(a, b) for a, b in zip(re[axis], im[axis])]))
        np.testing.assert_array_equal(np.signbit(got[axis, 1]), np.signbit(ref.imag))
        np.testing.assert_array_equal(np.signbit(got[axis, 0]), np.signbit(ref.real))
        z0 = got[~nz]
        if name == "csqrt":
            assert np.all(z0 == 0.0)
        else:
            assert np.all(z0[:, 0] == -np.inf) and np.all(np.abs(z0[:, 1]) <= np.pi)


def test_cexp(probe):
    mp = _mp()
    rng = np.random.default_rng(112)
    n = 20000
    re = np.concatenate([rng.uniform(-700, 700, n), 10.0 ** rng.uniform(-8, 2, n) * rng.choice([-1, 1], n), [0.0, -0.0, 0.0]])
    im = np.concatenate([10.0 ** rng.uniform(-8, 5, n) * rng.choice([-1, 1], n), 10.0 ** rng.uniform(-8, 5, n) * rng.choice([-1, 1], n),
                         [0.0, -0.0, np.pi]])
    got = run(probe, "cexp", np.stack([re, im], axis=1))
    want = [mp.exp(mp.mpc(a, b)) for a, b in zip(re, im)]
    report("cexp_ componentwise rel", float(np.max(_componentwise(got[:, 0], got[:, 1], want))), CEXP_BOUND)
    assert got[n * 2, 0] == 1.0 and got[n * 2, 1] == 0.0


def test_cdiv(probe):
    """the naive |b|^2 form: asserted where the kernels use it (|b| in 1e-100 .. 1e100, well inside the 1e+-150 of its range)"""
    mp = _mp()
    rng = np.random.default_rng(113)
    ar, ai = _complex_inputs(rng, 10000)
    n = ar.size
    rb = 10.0 ** rng.uniform(-100, 100, n)
    ang = rng.uniform(-np.pi, np.pi, n)
    br, bi = rb * np.cos(ang), rb * np.sin(ang)
    k = rng.integers(0, 4, n)                                           # a quarter each: pure real / pure imaginary divisors
    br[k == 1], bi[k == 2] = 0.0, 0.0
    bi[k == 1] = rb[k == 1]
    br[k == 2] = -rb[k == 2]
    got = run(probe, "cdiv", np.stack([ar, ai, br, bi], axis=1))
    nz = (ar != 0) | (ai != 0)
    want = [mp.mpc(a, b) / mp.mpc(c, d) for a, b, c, d in zip(ar[nz], ai[nz], br[nz], bi[nz])]
    report("operator/ componentwise rel", float(np.max(_componentwise(got[nz, 0], got[nz, 1], want))), CDIV_BOUND)
    assert np.all(got[~nz] == 0.0)


# ---- Heston closed form -----------------------------------------------------------------------------------------------
def _heston_np(ph, ps, ttm, v0, theta, kappa, rho, volvol):
    """heston_mgf_grid_kernel's expressions in NumPy complex128, from a_t0 = b_t0 = 0: log_mgf, and the size of the terms that
    cancel into it where volvol is small (theta kappa / volvol^2 times ttm psi_p and 2 log den, v0 b_t1's numerator over
    volvol^2 den)"""
    with np.errstate(all="ignore"):
        volvol2 = volvol * volvol
        b1 = (rho * volvol) * ph + kappa
        b0 = 0.5 * (ph * (ph + 1.0)) - ps
        zeta = np.sqrt(b1 * b1 - (2.0 * volvol2) * b0)
        exp_zeta = np.exp(-(ttm * zeta))
        psi_p, psi_m = zeta - b1, zeta + b1
        c_p, c_m = psi_p / (2.0 * zeta), psi_m / (2.0 * zeta)
        den = c_p * exp_zeta + c_m
        b_t1 = -((psi_p * c_m - psi_m * c_p * exp_zeta) / (volvol2 * den))
        a_t1 = -(theta * kappa / volvol2) * (ttm * psi_p + 2.0 * np.log(den))
        # psi_p = zeta - b1 cancels where volvol is small (zeta ~ b1 - volvol^2 b0 / b1): its operands' size, not its own
        ab = np.abs(zeta) + np.abs(b1)
        terms = ((theta * kappa / volvol2) * (ttm * ab + np.abs(2.0 * np.log(den)))
                 + v0 * (ab * np.abs(c_m) + np.abs(psi_m * c_p * exp_zeta)) / (volvol2 * np.abs(den)))
        return a_t1 + v0 * b_t1, terms


def _heston_grid(g, i):
    from stochvolmodels_amd.utils.mgf_pricer import get_phi_grid, get_psi_grid
    phi = get_phi_grid(is_spot_measure=True, vol_scaler=float(g["heston_vol_scaler"][i]))
    psi_q = get_psi_grid()[::int(g["heston_psi_stride"])]
    return np.concatenate([phi, np.zeros_like(psi_q)]), np.concatenate([np.zeros_like(phi), psi_q])


def test_heston_mgf_grid_vs_mpmath(golden):
    """compute_heston_mgf_grid (heston_mgf_grid_kernel) against the same closed form in mpmath: within 1e-10 wherever NumPy's
    complex128 evaluation is, never less accurate than NumPy -- |dev - mp| <= 4 |np - mp| + 1e-13 (1 + terms), the floor
    scaled by the size of the terms that cancel into log_mgf (theta kappa / volvol^2 = 900 for volvol 0.01: both evaluations
    round terms 10^3 times the result) -- and non-finite at exactly NumPy's non-finite points"""
    from stochvolmodels_amd.pricers.heston_pricer import compute_heston_mgf_grid
    g = golden("device_math")
    worst_np_good, worst_ratio = 0.0, 0.0
    for i, name in enumerate(g["heston_names"]):
        v0, theta, kappa, rho, volvol = (float(a) for a in g["heston_params"][i])
        phi, psi = _heston_grid(g, i)
        for j, ttm in enumerate(g["heston_ttms"]):
            mpv = g[f"heston_log_mgf_{name}"][j]
            dev, _, _ = compute_heston_mgf_grid(v0, theta, kappa, volvol, rho, float(ttm), phi, psi)
            npv, terms = _heston_np(phi, psi, float(ttm), v0, theta, kappa, rho, volvol)
            where = f"{name} ttm={ttm:g}"
            np.testing.assert_array_equal(np.isfinite(dev), np.isfinite(npv), err_msg=where)
            ok = np.isfinite(npv) & np.isfinite(mpv)
            assert np.array_equal(ok, np.isfinite(npv)), where              # mpmath is finite wherever NumPy is
            e_dev, e_np = np.abs(dev[ok] - mpv[ok]), np.abs(npv[ok] - mpv[ok])
            good = e_np <= 1e-10
            if good.any():
                worst_np_good = max(worst_np_good, float(e_dev[good].max()))
                assert float(e_dev[good].max()) <= 1e-10, where
            slack = 4.0 * e_np + 1e-13 * (1.0 + terms[ok])
            worst_ratio = max(worst_ratio, float(np.max(e_dev / slack)))
            assert np.all(e_dev <= slack), (where, float(np.max(e_dev - slack)))
    report("heston log_mgf |dev - mp| where NumPy is within 1e-10", worst_np_good, 1e-10)
    report("heston |dev - mp| / (4 |np - mp| + 1e-13 (1 + terms))", worst_ratio, 1.0)


def test_heston_mgf_grid_chains_in_time(golden):
    """time homogeneity: two half-maturity calls chained through a_t0 / b_t0 are one full-maturity call"""
    from stochvolmodels_amd.pricers.heston_pricer import compute_heston_mgf_grid
    g = golden("device_math")
    worst = 0.0
    for i, name in enumerate(g["heston_names"]):
        v0, theta, kappa, rho, volvol = (float(a) for a in g["heston_params"][i])
        phi, psi = _heston_grid(g, i)
        for ttm in g["heston_ttms"]:
            full, _, _ = compute_heston_mgf_grid(v0, theta, kappa, volvol, rho, float(ttm), phi, psi)
            _, a1, b1 = compute_heston_mgf_grid(v0, theta, kappa, volvol, rho, 0.5 * float(ttm), phi, psi)
            two, _, _ = compute_heston_mgf_grid(v0, theta, kappa, volvol, rho, 0.5 * float(ttm), phi, psi, a_t0=a1, b_t0=b1)
            ok = np.isfinite(full)
            np.testing.assert_array_equal(np.isfinite(two), ok, err_msg=f"{name} {ttm:g}")
            d = np.abs(two[ok] - full[ok]) / (1.0 + np.abs(full[ok]))
            worst = max(worst, float(d.max()))
    report("heston chained halves vs one call", worst, 1e-10)


# ---- Black-76 ---------------------------------------------------------------------------------------------------------
VOL_LO, VOL_HI = 1e-6, 10.0


def _black_mp(mp, F, K, sqrt_t, vol, is_call):
    """undiscounted price, vega, the larger of the price's two terms and the smaller of its two probabilities, at the double
    sqrt_t the device is given"""
    F, K, st = mp.mpf(float(F)), mp.mpf(float(K)), mp.mpf(float(sqrt_t))
    sv = mp.mpf(float(vol)) * st
    d1 = mp.log(F / K) / sv + sv / 2
    d2 = d1 - sv
    s = 1 if is_call else -1
    a, b = F * mp.ncdf(s * d1), K * mp.ncdf(s * d2)
    return s * (a - b), F * mp.npdf(d1) * st, max(a, b), min(mp.ncdf(s * d1), mp.ncdf(s * d2)), d1, sv


def _host_ivols(quotes):
    """svmc_black_implied_vols (the host build of the same solver), one call per (forward, ttm, discfactor)"""
    from stochvolmodels_amd import _lib
    L = _lib.load()
    price, K, code, F, T, df = (quotes[:, c] for c in range(6))
    out = np.full(len(quotes), -1.0)
    keys = np.stack([F, T, df], axis=1)
    for key in np.unique(keys, axis=0):
        sel = np.flatnonzero(np.all(keys == key, axis=1))
        p, k = np.ascontiguousarray(price[sel]), np.ascontiguousarray(K[sel])
        c = np.ascontiguousarray(code[sel].astype(np.int8))
        o = np.empty(sel.size)
        _lib.check(L.svmc_black_implied_vols(p.ctypes.data_as(DP), k.ctypes.data_as(DP), c.ctypes.data_as(C.POINTER(C.c_int8)),
                                             sel.size, float(key[0]), float(key[1]), float(key[2]), VOL_LO, VOL_HI,
                                             o.ctypes.data_as(DP)))
        out[sel] = o
    return out


def _device_ivols(probe, quotes):
    rows = np.concatenate([quotes, np.full((len(quotes), 1), VOL_LO), np.full((len(quotes), 1), VOL_HI)], axis=1)
    return run(probe, "black_implied_vol", rows)


def test_black_undisc_vs_mpmath(probe, golden):
    """price and vega of black_undisc (device erfc, log, exp): error of the price relative to the larger of its two terms
    (F N(d1) and K N(d2) cancel out of the money: that cancellation is the formula's, not the kernel's), vega relative
    to 2e-13 plus what d1 carries from log(F / K): its rounding (2^-53 absolute, a large relative error where K is within
    a few vol sqrt(T) of F at vol 1e-6) and d1^2 / 2's own, times d1 in exp(-d1^2 / 2).  Not where a probability N(d) itself
    underflows the double range (below 1e-300: strikes of e^200 forwards and beyond)"""
    mp = _mp()
    g = golden("device_math")
    F, K, T, vol = g["black_F"], g["black_K"], g["black_T"], g["black_vol"]
    call = (g["black_code"] == 0) | (g["black_code"] == 2)
    got = run(probe, "black_undisc", np.stack([F, K, np.sqrt(T), vol, call.astype(float)], axis=1))
    worst_p, worst_v = 0.0, 0.0
    eps = 2.0 ** -53
    for i in range(len(F)):
        p, vega, terms, prob, d1, sv = _black_mp(mp, F[i], K[i], np.sqrt(T[i]), vol[i], bool(call[i]))
        if prob >= 1e-300:
            worst_p = max(worst_p, float(abs(got[i, 0] - p) / terms))
        if vega > 1e-290:
            d1 = float(abs(d1))
            allowed = 2e-13 + 4 * eps * d1 * (1 / float(sv) + d1)
            worst_v = max(worst_v, float(abs(got[i, 1] / vega - 1)) / allowed)
    report("black_undisc price err / max term", worst_p, 2e-13)
    report("black_undisc vega err / (2e-13 + 4 eps d1 (1 / (vol sqrt T) + d1))", worst_v, 1.0)


def test_black_implied_vol_vs_mpmath(probe, golden):
    """black_implied_vol as chain_implied_vols_kernel runs it, against the exact vols of device_math.npz.  Where the
    inversion is well conditioned -- one rounding of the quote, of log(F / K) or of the price's two terms moves the vol by
    at most 1e-14 (black_cond) -- 4e-13 relative: the solver stops on a Halley step below 1e-13 v and lands up to 3.2e-13
    away, in the far tails (host and device alike; svmc_black.h).  Elsewhere within 1e-12 + 128 black_cond (55 measured,
    near vol_hi).  Not where a probability N(d) of the quote underflows the double range.  The host routine agrees: the same
    NaN pattern -- except where the solver's target lies within 4 ulp of the band's edge price(vol_lo) or price(vol_hi),
    which the device's and the host's libm may round to either side -- and 1e-12 on every well-conditioned vol both find"""
    mp = _mp()
    g = golden("device_math")
    quotes = np.stack([g["black_price"], g["black_K"], g["black_code"].astype(float), g["black_F"], g["black_T"], g["black_df"]], axis=1)
    dev, host = _device_ivols(probe, quotes), _host_ivols(quotes)
    price, K, code, F, T, df = (quotes[:, c] for c in range(6))
    target = np.where(code >= 2, price * F, price) / df                        # the solver's own target, in double
    edge = np.zeros(len(quotes), dtype=bool)
    for i in np.flatnonzero(np.isnan(dev) != np.isnan(host)):
        band = [_black_mp(mp, F[i], K[i], np.sqrt(T[i]), v, code[i] in (0, 2))[0] for v in (VOL_LO, VOL_HI)]
        edge[i] = min(abs(b - mp.mpf(target[i])) for b in band) <= 4 * mp.mpf(np.spacing(target[i]))
    print(f"NaN on one side only, at the band's edge: {int(edge.sum())}")
    np.testing.assert_array_equal(np.isnan(dev[~edge]), np.isnan(host[~edge]))
    fin = np.isfinite(dev)
    vol, cond = g["black_vol"], g["black_cond"]
    fits = g["black_min_prob"] >= 1e-300
    well = (cond <= 1e-14) & fits
    both = fin & np.isfinite(host) & well
    np.testing.assert_allclose(dev[both], host[both], rtol=1e-12, atol=0)
    # every well-conditioned quote inside the band inverts; a NaN is allowed only where the quote cannot be told apart from
    # the band's edge (the vol at the bracket's end, or the price saturated at the forward)
    assert np.all(fin[well & (vol > 2e-6) & (vol < 9.0)]), np.flatnonzero(~fin & well & (vol > 2e-6) & (vol < 9.0))
    err = np.abs(dev / vol - 1)
    m = well & fin
    report("black_implied_vol rel (well conditioned)", float(np.max(err[m])), 4e-13)
    r = fin & ~well & fits
    report("black_implied_vol rel / (1e-12 + 128 cond) (ill conditioned)", float(np.max(err[r] / (1e-12 + 128 * cond[r]))), 1.0)
    print(f"black quotes: {len(vol)}, finite {int(fin.sum())}, well conditioned {int(m.sum())}, ill conditioned {int(r.sum())}")


def test_black_implied_vol_nan_contract(probe):
    """NaN price, a price at or outside the band attainable on [vol_lo, vol_hi], K <= 0 -> NaN, as the host routine"""
    F, T, df = 100.0, 0.5, 0.9
    rows = []
    for code in (0, 1, 2, 3):
        for price, K in ((np.nan, 100.0), (0.0, 100.0), (-1.0, 100.0), (1e300, 100.0), (df * 100.0, 100.0), (5.0, 0.0),
                         (5.0, -10.0), (df * 30.0, 70.0), (df * 29.0, 70.0), (df * 20.0, 120.0), (df * 120.0, 120.0)):
            p = price / F if code >= 2 else price
            rows.append((p, K, code, F, T, df))
    quotes = np.array(rows)
    dev, host = _device_ivols(probe, quotes), _host_ivols(quotes)
    np.testing.assert_array_equal(np.isnan(dev), np.isnan(host))
    fin = np.isfinite(dev)
    np.testing.assert_allclose(dev[fin], host[fin], rtol=1e-12)
    for r, d in zip(rows, dev):
        price, K, code = r[0] * (F if r[2] >= 2 else 1.0), r[1], int(r[2])
        call = code in (0, 2)
        intrinsic = df * max((F - K) if call else (K - F), 0.0)
        upper = df * (F if call else K)
        if not (K > 0) or not (price > intrinsic) or not (price < upper):
            assert np.isnan(d), (r, d)


def test_payoff_finalize_one(probe):
    rng = np.random.default_rng(114)
    n = 20000
    cnt = rng.integers(1, 2 ** 20, n).astype(np.float64)
    mean = rng.normal(size=n) * 10.0 ** rng.uniform(-8, 2, n)
    sd = 10.0 ** rng.uniform(-6, 2, n)
    s, s2 = cnt * mean, cnt * (sd * sd + mean * mean)
    shift, df, npath = rng.uniform(-5, 5, n), rng.uniform(0.3, 1.0, n), cnt * rng.integers(1, 8, n)
    x = np.stack([s, s2, cnt, shift, df, npath], axis=1)
    got = run(probe, "payoff_finalize_one", x)
    L = lambda a: a.astype(np.longdouble)  # noqa: E731
    dmean = L(s) / L(cnt)
    price = L(df) * (L(shift) + dmean)
    var = np.maximum(L(s2) / L(cnt) - dmean * dmean, 0)
    stderr = L(df) * np.sqrt(var) / np.sqrt(L(npath))
    scale_p = L(df) * (np.abs(L(shift)) + np.abs(dmean))
    report("payoff_finalize_one price err / scale", float(np.max(np.abs(L(got[:, 0]) - price) / scale_p)), 4e-16)
    # the variance is a difference of second moments: its error is relative to s2 / cnt
    scale_v = L(df) * np.sqrt(L(s2) / L(cnt)) / np.sqrt(L(npath))
    err_v = np.abs(L(got[:, 1]) ** 2 - stderr ** 2) / (scale_v ** 2)
    report("payoff_finalize_one stderr^2 err / scale^2", float(err_v.max()), 1e-15)
    edge = run(probe, "payoff_finalize_one", np.array([[0.0, 0.0, 0.0, 1.0, 1.0, 10.0], [2.0, 4.0, 1.0, 0.0, 1.0, 1.0]]))
    assert np.isnan(edge[0, 0]) and np.isnan(edge[0, 1])                 # 0 / 0 -> NaN like NumPy's nanmean of nothing
    assert edge[1, 0] == 2.0 and edge[1, 1] == 0.0
