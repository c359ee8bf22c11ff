// svmc_tilted_cond.h -- the one home of what the weighted conditional estimators share: the payoff tail of libsvmc_ext.so (svmc_ext.hip,
// DESIGN.md row f17) and, in libsvmc_est.so (svmc_est.hip), its Greeks (row f18), the mixture density (row f19) and the many sets on
// jump rows (row f20).  Row f11's keep rule and Black-76 price restated (svmc_cmc.hip: cmc_keep, cmc_black), a path's weight and
// shifted forward, the forward pass, the strike-group preload, the payoff body on a path policy, the pieces of the finish kernels, the
// table and its ONE walk, and the host's quote check and upload / run / download driver -- written once, so that corr, K' = K + corr,
// the weight, the keep decisions and the sums are the same bits in both libraries.  Device code is __device__ __forceinline__ and the
// host code is inline: each library compiles its own copy and neither links the other.  No kernel is defined here: each unit names
// and launches its own.  A new estimator on rows (mu, cv) is a path policy, its kernels' four lines each and a chain entry.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "svmc_black.h"
#include "svmc_block.h"
#include "svmc_math.h"
#include "svmc_quotes.h"

namespace svmc {

static_assert(QUOTE_BLOCK == BLOCK, "svmc_quotes.h sizes the partial rows for blocks of BLOCK paths");

constexpr int TC_NSTAT = 7;            // [sum W, sum W^2, sum (W-1)^2, sum W ds, sum W^2 ds, sum (W ds)^2, kept], ds = F_t - corr - F
constexpr int TC_STAT_COLS = 8;        // ... padded: an expiry's statistics columns start at a multiple of 64 bytes
constexpr int TC_PAY_COLS = 3;         // per quote [sum W d, sum (W d)^2, sum W^2 d]
constexpr int TC_MAX_GROUPS = 65535;   // the groups are a grid's y dimension

struct TcExpiry {
    const double *mu, *cv;
    double forward, ln_forward;
    int k0, k1;                        // its strikes [k0, k1)
};

// ---- the table of a call and its ONE walk ------------------------------------------------------------------------------------------
// The device table of a tail with a forward pass; the image (expiries .. zs) is uploaded once.  Z: what the grid's z indexes -- a
// gamma (double) or the host constants of a set.  Each unit derives its own table type from this one, so that its kernels keep
// their names; the order of the fields is the kernels' argument layout.
template <class Z>
struct TcTableOf {
    const TcExpiry *expiries;          // [m]
    const QuoteGroup *groups;          // [G] groups of up to KT strikes; pad = 1: the expiry's first, which stores its statistics
                                       // sums (an expiry without strikes has one group of nk = 0 for them)
    const double *strikes;             // [K]
    const double *is_put;              // [K] 0 | 1
    const double *shift;               // [K] the host's shift of a strike's sums
    const Z *zs;                       // [nz]
    double *kp, *ln_kp;                // [K] device-computed: K + corr, its logarithm (0 where K + corr <= 0)
    double *fwd;                       // [m][4]: sum (e - 1), sum (e - 1)^2, kept count of f11's rule, corr
    double *fwd_partials;              // [rows][m][3]
    double *q_partials;                // [rows][NG][K][q_cols]
    double *stat_partials;             // [rows][NG][m][stat_cols]
    double *out;                       // the results, one block
    int m, K, NG;
    unsigned rows;
};
template <class Z>
struct TcImageOf {
    TcExpiry *expiries;
    QuoteGroup *groups;
    double *strikes, *is_put, *shift;
    Z *zs;
};
template <class Z>
inline TcImageOf<Z> tc_image(Layout &w, int m, size_t K, int G, size_t nz)
{
    return TcImageOf<Z>{w.take<TcExpiry>(m), w.take<QuoteGroup>(G), w.take<double>(K), w.take<double>(K), w.take<double>(K),
                        w.take<Z>(nz)};                    // (a braced list: in this order)
}
// ONE walk that is both the workspace's byte count and its carving: the image, the forward pass's head, the results, the partials.
// Returns the bytes of the image, which the walk starts with.
template <class Z>
inline size_t tc_workspace(Layout &w, size_t n_path, int m, size_t K, int G, int NG, size_t nz, size_t out_doubles, int q_cols,
                           int stat_cols, TcTableOf<Z> &t)
{
    const size_t rows = quote_rows(n_path);
    const TcImageOf<Z> im = tc_image<Z>(w, m, K, G, nz);
    const size_t image_bytes = w.bytes();
    t.expiries = im.expiries;
    t.groups = im.groups;
    t.strikes = im.strikes;
    t.is_put = im.is_put;
    t.shift = im.shift;
    t.zs = im.zs;
    t.kp = w.take<double>(K);
    t.ln_kp = w.take<double>(K);
    t.fwd = w.take<double>(4 * static_cast<size_t>(m));
    t.out = w.take<double>(out_doubles);
    t.fwd_partials = w.take<double>(rows * 3 * m);
    t.q_partials = w.take<double>(rows * NG * K * q_cols);
    t.stat_partials = w.take<double>(rows * NG * m * stat_cols);
    t.m = m;
    t.K = static_cast<int>(K);
    t.NG = NG;
    t.rows = static_cast<unsigned>(rows);
    return image_bytes;
}
// the image but for zs: the expiries on their rows (cv null: the tail has none and reads none), the strikes' columns with
// shift(i, k), the groups of up to kt strikes
template <class Z, class Shift>
inline void tc_fill_image(const TcImageOf<Z> &im, int m, const size_t *offsets, int kt, const double *const *mu, const double *const *cv,
                          const double *forwards, const double *strikes, const int8_t *types, Shift &&shift)
{
    quote_image(
        m, offsets,
        [&](int i, int k0, int k1) { im.expiries[i] = TcExpiry{mu[i], cv ? cv[i] : nullptr, forwards[i], std::log(forwards[i]), k0, k1}; },
        [&](int i, int k) {
            im.strikes[k] = strikes[k];
            im.is_put[k] = (types[k] == SVMC_PUT) ? 1.0 : 0.0;
            im.shift[k] = shift(i, k);
        });
    quote_groups(m, offsets, kt, true, im.groups);
}

// ---- the host side of a chain entry -----------------------------------------------------------------------------------------------
#define SVMC_TC_TRY(call)                        \
    do {                                         \
        if ((call) != hipSuccess) return SVMC_ERR_HIP; \
    } while (0)

// The quote check of every entry, before anything is launched: the offsets start at 0, do not decrease and stay within 2^30; a row
// pointer per expiry (cv null: the entry has no such rows); forwards finite and positive (null: the entry has none); the values of
// a and b [offsets[m]] finite (null: none); the types SVMC_CALL | SVMC_PUT (null: none) -- the one SVMC_ERR_UNKNOWN_PAYOFF, last.
inline int tc_check_quotes(int m, const size_t *offsets, const double *const *mu, const double *const *cv, const double *forwards,
                           const double *a, const double *b, const int8_t *types)
{
    if (offsets[0] != 0) return SVMC_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < m; ++i) {
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] > (static_cast<size_t>(1) << 30)) return SVMC_ERR_INVALID_ARGUMENT;
        if (!mu[i] || (cv && !cv[i])) return SVMC_ERR_INVALID_ARGUMENT;
        if (forwards && (!std::isfinite(forwards[i]) || !(forwards[i] > 0.0))) return SVMC_ERR_INVALID_ARGUMENT;
    }
    const size_t K = offsets[m];
    for (size_t k = 0; k < K; ++k)
        if ((a && !std::isfinite(a[k])) || (b && !std::isfinite(b[k]))) return SVMC_ERR_INVALID_ARGUMENT;
    for (size_t k = 0; types && k < K; ++k)
        if (types[k] != SVMC_CALL && types[k] != SVMC_PUT) return SVMC_ERR_UNKNOWN_PAYOFF;
    return SVMC_OK;
}
inline bool tc_all_finite(const double *v, int n)
{
    for (int z = 0; z < n; ++z)
        if (!std::isfinite(v[z])) return false;
    return true;
}

// ONE upload of the table's host image to the head of the workspace, the entry's launches (a callable that returns a status), ONE
// download of the results' block, ONE synchronise
template <class Launches>
inline int tc_run(void *workspace, const std::vector<unsigned char> &image, const double *device_out, std::vector<double> &out,
                  hipStream_t stream, Launches &&launches)
{
    SVMC_TC_TRY(hipMemcpyAsync(workspace, image.data(), image.size(), hipMemcpyHostToDevice, stream));
    const int rc = launches();
    if (rc != SVMC_OK) return rc;
    SVMC_TC_TRY(hipMemcpyAsync(out.data(), device_out, out.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    SVMC_TC_TRY(hipStreamSynchronize(stream));
    return SVMC_OK;
}
// the next `count` doubles of the results' block to the caller's array; returns what follows them
inline const double *tc_split(const double *block, double *dst, size_t count)
{
    if (count > 0) memcpy(dst, block, count * sizeof(double));
    return block + count;
}

// ---- row f11's keep rule and Black-76 price, restated (svmc_cmc.hip: cmc_keep, cmc_black) --------------------------------------
// a path passes f11's rule iff mu, cv and e = exp(mu + cv / 2) are finite and cv >= 0; h = mu + cv / 2
__device__ __forceinline__ bool tc_keep_cmc(double mu, double cv, double &h, double &e)
{
    h = fma(0.5, cv, mu);
    e = exp_full(h);
    const double inf = __builtin_huge_val();
    return fabs(mu) < inf && cv >= 0.0 && cv < inf && e < inf;     // a NaN fails a comparison
}

// the undiscounted Black-76 price of ft against K' at total variance cv, on the quoted side's own formula
__device__ __forceinline__ double tc_black(double ft, double ln_ft, double cv, double sd, double inv_sd, double kp, double ln_kp, bool put)
{
    if (!(kp > 0.0)) return put ? 0.0 : ft - kp;
    if (cv == 0.0) return put ? fmax(kp - ft, 0.0) : fmax(ft - kp, 0.0);
    const double d1 = fma(ln_ft - ln_kp, inv_sd, 0.5 * sd), d2 = d1 - sd;
    return put ? kp * black_norm_cdf(-d2) - ft * black_norm_cdf(-d1) : ft * black_norm_cdf(d1) - kp * black_norm_cdf(d2);
}

// Once per (path, gamma): the weight W = exp(gamma mu + gamma^2 cv / 2), e_t = exp(mu + (gamma + 1/2) cv), the shifted forward
// F_t = F e_t and its logarithm.  half_g2 = gamma^2 / 2 and g_half = gamma + 1/2 are the caller's, formed once per block.  Returns
// the second half of the keep rule: W^2 and (W F_t)^2 finite (a NaN fails the comparison).
__device__ __forceinline__ bool tc_weight_forward(double mu, double cv, double gamma, double half_g2, double g_half, double forward,
                                                  double ln_forward, double &w, double &et, double &ft, double &ln_ft)
{
    constexpr double INF = __builtin_huge_val();
    w = exp_full(fma(half_g2, cv, gamma * mu));
    const double lr = fma(g_half, cv, mu);
    et = exp_full(lr);
    ft = forward * et;
    ln_ft = ln_forward + lr;
    const double wf = w * ft;
    return w * w < INF && wf * wf < INF;
}

// ---- the forward pass: cmc_forward_kernel's and cmc_forward_finish_kernel's statements ------------------------------------------
// ZERO_CV: the rows are (a, 0) -- the constant 0.0 stands where a path's cv is read, and the expiry's cv, null, is not touched
// grid (path blocks, expiries); lds [4 * 3]
template <bool ZERO_CV, class Table>
__device__ __forceinline__ void tc_forward_body(const Table &t, size_t n, double *lds)
{
    const TcExpiry ex = t.expiries[blockIdx.y];
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    double v[3] = {0.0, 0.0, 0.0};
    for (size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x; i < n; i += stride) {
        const double mu = ex.mu[i];
        double h, e, cv = 0.0;
        if constexpr (!ZERO_CV) cv = ex.cv[i];
        if (tc_keep_cmc(mu, cv, h, e)) {
            const double d = e - 1.0;
            v[0] += d;
            v[1] = fma(d, d, v[1]);
            v[2] += 1.0;
        }
    }
    block_sum_store<3>(v, lds, t.fwd_partials + (static_cast<size_t>(blockIdx.x) * t.m + blockIdx.y) * 3, 3);
}

// a block per expiry: the three column sums in row order, corr, and -- once per strike -- K' = K + corr and ln K'; lds [4]
template <class Table>
__device__ __forceinline__ void tc_forward_finish_body(const Table &t, int recenter, double *lds)
{
    const int i = blockIdx.x;
    const TcExpiry ex = t.expiries[i];
    const size_t ld = 3 * static_cast<size_t>(t.m);
    const double *base = t.fwd_partials + 3 * static_cast<size_t>(i);
    const double s0 = block_column_sum(base, t.rows, ld, lds);
    __syncthreads();
    const double s1 = block_column_sum(base + 1, t.rows, ld, lds);
    __syncthreads();
    const double cnt = block_column_sum(base + 2, t.rows, ld, lds);
    __syncthreads();                                       // thread 0 has read the wave totals: lds[0] now carries corr to the block
    if (threadIdx.x == 0) {
        const double dmean = s0 / cnt;                     // 0 / 0 -> NaN like nanmean of an empty slice
        const double corr = recenter ? ex.forward * dmean : 0.0;       // mean_kept(F e) - F
        double *f = t.fwd + 4 * i;
        f[0] = s0;
        f[1] = s1;
        f[2] = cnt;
        f[3] = corr;
        lds[0] = corr;
    }
    __syncthreads();
    const double corr = lds[0];
    for (int k = ex.k0 + static_cast<int>(threadIdx.x); k < ex.k1; k += BLOCK) {
        const double kp = t.strikes[k] + corr;
        t.kp[k] = kp;
        t.ln_kp[k] = (kp > 0.0) ? log(kp) : 0.0;
    }
}

// ---- the weighted Black-76 sums -----------------------------------------------------------------------------------------------------
// (The bodies below take the table by value: with the kernel's own copy behind a reference the compiler no longer sees that the row
// pointers it loads are global memory's and reads the paths through flat loads -- as the forward pass, left as it was, does.)
// the constants of a group's strikes, in vector registers
template <int KT, class Table>
__device__ __forceinline__ void tc_group_preload(const Table t, const QuoteGroup &g, double (&kp)[KT], double (&ln_kp)[KT], double (&shift)[KT],
                                                 bool (&put)[KT])
{
    const int nk = g.nk;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        const int kk = g.k0 + ((k < nk) ? k : 0);          // the unused strikes of a group repeat its first; their sums are dropped
        const bool on = nk > 0;                            // a group without strikes reads none
        kp[k] = on ? t.kp[kk] : 1.0;
        ln_kp[k] = on ? t.ln_kp[kk] : 0.0;
        shift[k] = on ? t.shift[kk] : 0.0;
        put[k] = on ? t.is_put[kk] != 0.0 : false;
    }
}

// (cv, sd, 1 / sd) of a kept path
struct TcVariance {
    double cv, sd, inv_sd;
};
// a path's terms on rows (mu, cv) under exp(gamma x): tc_keep_cmc, tc_weight_forward and sd = sqrt(cv); z: the gamma
struct TcTiltedPath {
    double gamma, half_g2, g_half, forward, ln_forward;
    template <class Table>
    __device__ __forceinline__ TcTiltedPath(const Table t, const TcExpiry &ex, int, unsigned z)
        : gamma(t.zs[z]), half_g2(0.5 * gamma * gamma), g_half(gamma + 0.5), forward(ex.forward), ln_forward(ex.ln_forward)
    {
    }
    // false: the path is dropped
    __device__ __forceinline__ bool operator()(const TcExpiry &ex, size_t i, double &w, double &ft, double &ln_ft, double &cv) const
    {
        const double mu = ex.mu[i];
        cv = ex.cv[i];
        double h, e, et;
        if (!tc_keep_cmc(mu, cv, h, e)) return false;
        // once per (path, gamma): the weight and the shifted forward with its logarithm
        return tc_weight_forward(mu, cv, gamma, half_g2, g_half, forward, ln_forward, w, et, ft, ln_ft);
    }
    __device__ __forceinline__ TcVariance variance(double cv) const
    {
        const double sd = sqrt(cv);                        // once per path
        return TcVariance{cv, sd, 1.0 / sd};
    }
};

constexpr int tc_payoff_sums(int kt) { return block_sum_padded(TC_PAY_COLS * kt + TC_NSTAT); }

// Block (path block, group of up to KT strikes of one expiry, z).  Path: the policy, built once per block from (table, expiry, its
// index, z), that forms a path's (w, F_t, ln F_t) or drops it, and then the kept path's (cv, sd, 1 / sd) -- a call of its own, so that
// a policy whose variance is the block's hands out scalars.  Per kept path the expiry's seven statistics sums and, per strike, the
// Black-76 price B and the sums of w d, (w d)^2, w (w d), d = B - shift; the statistics ride in the same block sum and are stored by the
// expiry's first group.  lds [4 * tc_payoff_sums(KT)].  (jump_sets_payoff_kernel, svmc_est.hip, has these statements typed in: as a
// policy on this body it measured slower, profiles/cond_tails_refactor.txt section 2.)
template <int KT, class Path, class Table>
__device__ __forceinline__ void tc_payoff_body(const Table t, size_t n, double *lds)
{
    constexpr int NP = TC_PAY_COLS * KT, NV = NP + TC_NSTAT, NSUM = tc_payoff_sums(KT);
    const QuoteGroup g = t.groups[blockIdx.y];
    const TcExpiry ex = t.expiries[g.expiry];
    const int nk = g.nk;                                   // (block-uniform; 0: the group only forms the statistics)
    const double corr = t.fwd[4 * g.expiry + 3];
    const double forward = ex.forward;
    const Path path(t, ex, g.expiry, blockIdx.z);
    double kp[KT], ln_kp[KT], shift[KT], acc[NSUM];
    bool put[KT];
#pragma unroll
    for (int j = 0; j < NSUM; ++j) acc[j] = 0.0;
    tc_group_preload(t, g, kp, ln_kp, shift, put);
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    for (size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x; i < n; i += stride) {
        double w, ft, ln_ft, cv = 0.0;                     // cv: the path's own, where the rows carry one
        if (!path(ex, i, w, ft, ln_ft, cv)) continue;
        const TcVariance u = path.variance(cv);            // (... or the block's)
        const double v = w - 1.0;
        const double wds = w * ((ft - corr) - forward);
        acc[NP] += w;
        acc[NP + 1] = fma(w, w, acc[NP + 1]);
        acc[NP + 2] = fma(v, v, acc[NP + 2]);
        acc[NP + 3] += wds;
        acc[NP + 4] = fma(w, wds, acc[NP + 4]);
        acc[NP + 5] = fma(wds, wds, acc[NP + 5]);
        acc[NP + 6] += 1.0;
        if (nk > 0) {
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const double wd = w * (tc_black(ft, ln_ft, u.cv, u.sd, u.inv_sd, kp[k], ln_kp[k], put[k]) - shift[k]);
                acc[k] += wd;
                acc[KT + k] = fma(wd, wd, acc[KT + k]);
                acc[2 * KT + k] = fma(w, wd, acc[2 * KT + k]);
            }
        }
    }
    const bool first = g.pad != 0;
    block_sum_apply<NSUM>(acc, lds, NV, [&](int j, double sum) {
        const size_t slot = static_cast<size_t>(blockIdx.x) * t.NG + blockIdx.z;           // partials[path block][z]
        if (j < NP) {
            const int which = j / KT, k = j - which * KT;
            if (k < nk) t.q_partials[(slot * t.K + g.k0 + k) * TC_PAY_COLS + which] = sum;
        } else if (first) {
            t.stat_partials[(slot * t.m + g.expiry) * TC_STAT_COLS + (j - NP)] = sum;
        }
    });
}

// ---- the pieces of the finish kernels: a block per (column, z), columns [0, K) the quotes, [K, K + m) the expiries' statistics ------
// the expiry of a column (block-uniform)
template <class Expiry>
__device__ __forceinline__ int tc_expiry_of_column(const Expiry *expiries, int m, int K, int col)
{
    int i = col - K;
    if (col < K) {
        i = 0;
        while (i + 1 < m && col >= expiries[i].k1) ++i;    // expiries without strikes are skipped over
    }
    return i;
}

// the sums of N columns of the partial rows, one after the other in row order: column cols[q] of `base` into s[q]
template <int N>
__device__ __forceinline__ void tc_column_sums(const double *base, const int (&cols)[N], unsigned rows, size_t ld, double *lds, double *s)
{
#pragma unroll
    for (int q = 0; q < N; ++q) {
        if (q > 0) __syncthreads();
        s[q] = block_column_sum(base + cols[q], rows, ld, lds);
    }
}

// A value and its error from the sums (c0, c1, c2) = (sum W d, sum (W d)^2, sum W^2 d), d = v - shift, and the expiry's (W, Q, kept):
// e = value - shift = c0 / W and sum (W (v - value))^2 = c1 - 2 e c2 + e^2 Q.  One kept path: the estimate IS that path's value and
// the squares about it are zero identically
__device__ __forceinline__ void tc_value_error(double c0, double c1, double c2, double W, double Q, double kept, double &e, double &err)
{
    e = c0 / W;
    const double var = (kept > 1.0) ? fma(e, fma(e, Q, -2.0 * c2), c1) : 0.0;
    err = sqrt(fmax(var, 0.0)) / W;
}

// the statistics in terms of the weights a tail sums as they are: sum W is the sum, nothing follows the eight doubles
struct TcPlainWeights {
    template <class Table>
    __device__ __forceinline__ static double sum_w(const Table &, int, int, double w) { return w; }
    template <class Table>
    __device__ __forceinline__ static void epilogue(const Table &, int, int) {}
};

// The quotes' prices and errors and the expiries' SVMC_TILTED_STATS_DOUBLES statistics of a payoff tail; the sums are the column sums
// of the partial rows in row order, formed as row f8's finish forms them (svmc_kernels.hip).  Weights: sum_w(t, z, expiry, w), the sum
// of the weights in terms of the summed w, and epilogue(t, z, expiry), what the expiry's block stores besides.  lds [4]
template <class Weights, class Table>
__device__ __forceinline__ void tc_finish_body(const Table t, size_t n, double *lds)
{
    const int col = blockIdx.x, gi = blockIdx.y;
    const size_t K = static_cast<size_t>(t.K), m = static_cast<size_t>(t.m), NG = static_cast<size_t>(t.NG);
    const size_t ld_stat = NG * m * TC_STAT_COLS, ld_pay = NG * K * TC_PAY_COLS;
    const int i = tc_expiry_of_column(t.expiries, t.m, t.K, col);
    const double *st = t.stat_partials + (static_cast<size_t>(gi) * m + i) * TC_STAT_COLS;
    double s[TC_NSTAT];
    if (col < t.K) {
        // the expiry's sum W, sum W^2 and kept count, then the quote's three columns
        const double *pay = t.q_partials + (static_cast<size_t>(gi) * K + col) * TC_PAY_COLS;
        tc_column_sums(st, {0, 1, 6}, t.rows, ld_stat, lds, s);
        __syncthreads();
        tc_column_sums(pay, {0, 1, 2}, t.rows, ld_pay, lds, s + 3);
        if (threadIdx.x != 0) return;
        double e, err;                                     // price = shift + e
        tc_value_error(s[3], s[4], s[5], s[0], s[1], s[2], e, err);
        t.out[gi * K + col] = e + t.shift[col];
        t.out[NG * K + gi * K + col] = err;
        return;
    }
    tc_column_sums(st, {0, 1, 2, 3, 4, 5, 6}, t.rows, ld_stat, lds, s);
    if (threadIdx.x != 0) return;
    const double w = s[0], Q = s[1], V2 = s[2], D0 = s[3], D1 = s[4], D2 = s[5], kept = s[6];
    // normalizer n / sum W, a ratio of sums: error sqrt(sum (1 - N W)^2) / sum W = N sqrt(sum (W - mean W)^2) / sum W, the squares
    // about the mean from the sums of W - 1; gamma forward = F + sum W ds / sum W, its error as a strike's.  Where W = c w the
    // normalizer and sum W carry c and every ratio of two weighted sums is free of it
    const double W = Weights::sum_w(t, gi, i, w);
    const double N = kept / W, sv = w - kept;
    const double dev2 = (kept > 1.0) ? V2 - sv * sv / kept : 0.0;
    double gd, gerr;
    tc_value_error(D0, D2, D1, w, Q, kept, gd, gerr);
    double *out = t.out + 2 * NG * K + (static_cast<size_t>(gi) * m + i) * SVMC_TILTED_STATS_DOUBLES;
    out[0] = N;
    out[1] = N * sqrt(fmax(dev2, 0.0)) / w;
    out[2] = t.expiries[i].forward + gd;
    out[3] = gerr;
    out[4] = (w / Q) * w;                                  // effective sample size (sum W)^2 / sum W^2
    out[5] = kept;
    out[6] = static_cast<double>(n) - kept;
    out[7] = W;
    Weights::epilogue(t, gi, i);
}

}  // namespace svmc
