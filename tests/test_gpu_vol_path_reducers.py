"""
The two streaming reducers of the volatility-path array -- svmc_row_power_sums (row_power_sums_kernel) and
svmc_expanding_mean_squares (expanding_mean_sq_kernel) -- on SUPPLIED arrays, through the C ABI, against EXACT sums.

Every input is a multiple of 2^-52 below 2 in size, so a value, its distance from the centre, the powers of that distance and
their sums are integers over a power of two: the references are fractions.Fraction built from Python integers, with no rounding
anywhere.  The tolerances are a-priori rounding bounds worked out from the kernels' code (nothing is measured), and the data make
every single element count: a lost, doubled or misplaced element is a hundred bounds away.

Shapes: every path the kernels take -- widths around the 16-byte pairs and the block, a width whose quarter-row segments start on
odd columns and run the eight-deep loop twice, row counts around and past the 1024-row chunk of reciprocals, leading dimensions
larger than the width (odd ones: the rows' alignment alternates), bases 8 bytes off a 16-byte boundary, n_moments 1 .. 4.
"""
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest

import vol_paths_steps as vp

pytestmark = pytest.mark.gpu

U = Fraction(1, 2 ** 53)
SLACK = Fraction(101, 100)
Q = 2 ** 52                                                # the inputs are multiples of 1 / Q
CENTERS = {"theta": 1.0413, "zero": 0.0}
# the kernels' constants (stochvolmodels_amd/csrc/svmc_kernels.hip, svmc_block.h)
BLOCK, ROW_SEGMENTS, ROW_SUM_U, EXPANDING_CHUNK = 256, 4, 8, 1024
POISON = np.nan                                            # input padding: a kernel that reads it cannot pass
SENTINEL = vp.SENTINEL                                     # output padding


@pytest.fixture(scope="module")
def sv():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import _lib
    _lib.load()
    return sv


def spread(rng, shape):
    """+-|d|, |d| log-uniform in [0.5, 2] x 0.3"""
    return 0.3 * np.exp2(rng.uniform(-1.0, 1.0, shape)) * rng.choice([-1.0, 1.0], shape)


def on_grid(a):
    """the nearest multiples of 1 / Q (|a| < 2: a Q is below 2^53 and the division is exact)"""
    a = np.round(a * Q) / Q
    assert np.all(np.abs(a) < 2.0) and np.all(a * Q == np.round(a * Q))
    return a


def as_ints(a):
    """a Q as Python integers (exact)"""
    return (a * Q).astype(np.int64).astype(object)


def padded(a, ld, fill, lead):
    """a [rows][cols] laid out with leading dimension ld behind `lead` doubles, everything else `fill`"""
    rows, cols = a.shape
    buf = np.full(lead + rows * ld, fill)
    buf[lead:].reshape(rows, ld)[:, :cols] = a
    return buf


# ---- svmc_row_power_sums --------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 30731)
ROWS = 3


def longest_chain(n_cols):
    """D: the additions on the longest chain from a term to its output, from row_power_sums_kernel's code.
    A block owns one of ROW_SEGMENTS quarter-row segments, columns [n s / 4, n (s + 1) / 4).  Lane i adds the double2 elements
    i, i + BLOCK, ... of the segment's aligned body to its accumulator one after the other (the eight-deep loop and its
    remainder loop keep that order): 2 ceil(pairs / BLOCK) additions for lane 0, the busiest, which also takes the peeled first
    element and the odd last one: + 2.  block_sum_apply then adds across the wave in six levels (xor 32 .. 1; the halving tree
    and the wave_sum branch alike) and across the four waves in three additions, and reduce_columns adds the four segments'
    partials: three more."""
    seg = max(n_cols * (s + 1) // ROW_SEGMENTS - n_cols * s // ROW_SEGMENTS for s in range(ROW_SEGMENTS))
    pairs = seg // 2
    return 2 * -(-pairs // BLOCK) + 2 + 6 + 3 + 3


@lru_cache(maxsize=None)
def row_case(n_cols, center_tag):
    """(a [ROWS][n_cols], S [ROWS][8], A [ROWS][8], min |d|): the data of a width and the exact sums of its powers, computed once"""
    center = CENTERS[center_tag]
    rng = np.random.default_rng(1000 * n_cols + len(center_tag))
    a = on_grid(center + spread(rng, (ROWS, n_cols)))
    c = int(center * Q)
    assert c / Q == center
    m = as_ints(a) - c                                       # (a - center) Q, exact
    assert np.all((a - center) * Q == m.astype(np.float64))  # ... and the kernel's subtraction is exact too: a term rounds j - 1 times
    S = [[Fraction(int(np.sum(r ** j)), Q ** j) for j in range(1, 9)] for r in m]
    A = [[Fraction(int(np.sum(np.abs(r) ** j)), Q ** j) for j in range(1, 9)] for r in m]
    a.setflags(write=False)
    return a, S, A, Fraction(int(np.min(np.abs(m))), Q)


def row_power_sums(a, center, n_moments, ld, lead):
    from stochvolmodels_amd import _lib
    from stochvolmodels_amd.engine import DeviceBuffer
    rows, cols = a.shape
    k2 = 2 * n_moments
    src = vp.upload(padded(a, ld, POISON, lead))
    sums, ws = DeviceBuffer(rows * k2), DeviceBuffer(rows * ROW_SEGMENTS * k2)
    try:
        _lib.check(_lib.load().svmc_row_power_sums(src.offset(lead), ld, rows, cols, center, n_moments, sums.ptr, ws.ptr, ws.nbytes, None))
        return vp.download(sums, rows * k2).reshape(k2, rows)
    finally:
        for b in (src, sums, ws):
            b.free()


def check_row_sums(got, S, A, D, rows, what):
    """|got - S_j| <= (j + D) 2^-53 A_j x 1.01 on `rows`: j roundings of one term (the subtraction and j - 1 multiplications; the
    test's subtraction happens to be exact) and D additions.  Returns the worst error / bound."""
    worst = 0.0
    for j in range(1, got.shape[0] + 1):
        for r in rows:
            assert np.isfinite(got[j - 1, r]), (what, j, r)
            err, lim = abs(Fraction(float(got[j - 1, r])) - S[r][j - 1]), (j + D) * U * A[r][j - 1] * SLACK
            worst = max(worst, float(err / lim))
            assert err <= lim, (what, "j", j, "row", r, float(err), float(lim))
    return worst


def layouts(n_cols):
    out = [(n_cols, 0), (n_cols, 1)]                         # (ld, doubles the base is off its buffer's start: 1 = 8 bytes)
    if n_cols in (1025, 30731):
        out += [(n_cols + 1, 0), (n_cols + 2, 0), (n_cols + 1, 1)]
    return out


@pytest.mark.parametrize("center_tag", sorted(CENTERS))
@pytest.mark.parametrize("n_cols", WIDTHS)
def test_row_power_sums_against_exact_sums(sv, n_cols, center_tag):
    a, S, A, dmin = row_case(n_cols, center_tag)
    D = longest_chain(n_cols)
    for j in range(1, 9):                                    # any single lost or doubled element is a hundred bounds away
        assert all(dmin ** j >= 100 * (j + D) * U * A[r][j - 1] * SLACK for r in range(ROWS)), (n_cols, j)
    if n_cols == 30731:                                      # odd segment starts, and the eight-deep loop runs twice
        seg = n_cols // ROW_SEGMENTS                         # (lane 0's second round starts at double2 element ROW_SUM_U x BLOCK)
        assert seg // 2 > (2 * ROW_SUM_U - 1) * BLOCK and any((n_cols * s // ROW_SEGMENTS) % 2 for s in range(ROW_SEGMENTS))
    for n_moments in (1, 2, 3, 4):
        for ld, lead in layouts(n_cols):
            what = f"row_power_sums n_cols {n_cols} center {center_tag} n_moments {n_moments} ld {ld} base +{8 * lead} B"
            got = row_power_sums(a, CENTERS[center_tag], n_moments, ld, lead)
            print(f"{what}: D {D} worst error / bound {check_row_sums(got, S, A, D, range(ROWS), what):.3f}")


@pytest.mark.parametrize("n_cols,col", [(1025, 513), (30731, 30730), (30731, 9000), (5, 0)])
def test_row_power_sums_keep_a_nan_in_its_row(sv, n_cols, col):
    a, S, A, _ = row_case(n_cols, "theta")
    b = a.copy()
    b[1, col] = np.nan
    for n_moments in (1, 4):
        got = row_power_sums(b, CENTERS["theta"], n_moments, n_cols, 0)
        assert np.all(np.isnan(got[:, 1]))
        check_row_sums(got, S, A, longest_chain(n_cols), (0, 2), f"NaN at row 1, column {col} of {n_cols}")


# ---- svmc_expanding_mean_squares --------------------------------------------------------------------------------------------------------
MAX_ROWS, MAX_COLS = 2049, 514
ROW_COUNTS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 1030, 2049)
COL_COUNTS = (1, 2, 63, 64, 65, 130, 513, 514)
SHAPES = sorted({(r, c) for r in ROW_COUNTS for c in (130, 513)} | {(1030, c) for c in COL_COUNTS})


@pytest.fixture(scope="module")
def expanding():
    """(a [2049][514], S): S[t][p] = Q^2 sum over u <= t of a[u][p]^2 as Python integers -- the top-left block of S is the exact
    expanding sum of the same block of a, so every shape shares this one reference"""
    a = on_grid(spread(np.random.default_rng(77), (MAX_ROWS, MAX_COLS)))
    m = as_ints(a)
    S = np.cumsum(m * m, axis=0)
    a.setflags(write=False)
    S.setflags(write=False)
    return a, S


def expanding_mean_squares(a, ld, ldo, lead_a=0, lead_o=0):
    """the whole output buffer as the device left it: (out [rows][ldo], the `lead_o` doubles in front of it)"""
    from stochvolmodels_amd import _lib
    rows, cols = a.shape
    src = vp.upload(padded(a, ld, POISON, lead_a))
    dst = vp.upload(np.full(lead_o + rows * ldo, SENTINEL))
    try:
        _lib.check(_lib.load().svmc_expanding_mean_squares(src.offset(lead_a), ld, rows, cols, dst.offset(lead_o), ldo, None))
        buf = vp.download(dst, lead_o + rows * ldo)
        return buf[lead_o:].reshape(rows, ldo), buf[:lead_o]
    finally:
        src.free()
        dst.free()


def check_expanding(got, S):
    """|got - M| <= (t + 3) 2^-53 M x 1.01, M = S / (Q^2 (t + 1)): t + 1 fused accumulations of positive terms, one correctly rounded
    reciprocal, one product.  In integers: got = mi 2^(ex - 53), and the inequality times (t + 1) Q^2 2^53 x 100.
    Returns the worst error / bound."""
    rows, cols = got.shape
    assert np.all(np.isfinite(got)) and np.all(got > 0.0)
    mant, ex = np.frexp(got)
    mi = (mant * 2.0 ** 53).astype(np.int64).astype(object)
    assert int(ex.min()) + 104 >= 0
    shift = np.array([1 << int(e) for e in (ex + 104).ravel()], dtype=object).reshape(got.shape)
    t1 = np.arange(1, rows + 1).astype(object)[:, None]
    S = S[:rows, :cols]
    lhs = np.abs(mi * shift * t1 - S * 2 ** 53) * 100
    rhs = (t1 + 2) * 101 * S
    ratio = float(np.max((lhs / rhs).astype(np.float64)))
    assert np.all(lhs <= rhs), ("worst error / bound", ratio, "at", np.argwhere(lhs > rhs)[:4].tolist())
    return ratio


@pytest.mark.parametrize("n_rows,n_cols", SHAPES)
def test_expanding_mean_squares_against_exact_means(sv, expanding, n_rows, n_cols):
    a, S = expanding
    assert n_rows <= EXPANDING_CHUNK or n_rows in (1025, 1030, 2049)      # the second and third chunk of reciprocals
    got, _ = expanding_mean_squares(a[:n_rows, :n_cols], n_cols, n_cols)
    print(f"expanding_mean_squares {n_rows} x {n_cols}: worst error / bound {check_expanding(got, S):.3f}")


def test_expanding_mean_squares_pair_and_single_forms_agree(sv, expanding):
    """514 columns on an aligned even layout take two columns per lane; an odd ld, an odd ldo, or either base 8 bytes off takes one
    column per lane: the same bits per element, and the output's padding (and the double in front of an offset base) untouched"""
    a, S = expanding
    a = a[:1030, :514]
    pair, _ = expanding_mean_squares(a, 514, 514)
    check_expanding(pair, S)
    for ld, ldo, lead_a, lead_o in ((515, 514, 0, 0), (514, 515, 0, 0), (514, 514, 1, 0), (514, 514, 0, 1), (516, 518, 0, 0),
                                    (517, 519, 1, 1)):
        got, front = expanding_mean_squares(a, ld, ldo, lead_a, lead_o)
        np.testing.assert_array_equal(got[:, :514], pair, err_msg=str((ld, ldo, lead_a, lead_o)))
        assert np.all(got[:, 514:] == SENTINEL) and np.all(front == SENTINEL), (ld, ldo, lead_a, lead_o)


@pytest.mark.parametrize("n_rows,n_cols,ld,ldo", [(1030, 513, 514, 516), (1025, 130, 133, 131), (5, 2, 4, 6)])
def test_expanding_mean_squares_padded_layouts(sv, expanding, n_rows, n_cols, ld, ldo):
    a, S = expanding
    got, _ = expanding_mean_squares(a[:n_rows, :n_cols], ld, ldo)
    check_expanding(got[:, :n_cols], S)
    assert np.all(got[:, n_cols:] == SENTINEL)
