// svmc_ext.hip -- libsvmc_ext.so, the model-agnostic estimators beside the closed core (include/svmc_ext.h).
// One translation unit on the header-only parts of csrc/; nothing of libsvmc.so is linked and no session is needed.
//
// Conditional Monte Carlo under the exponential risk-premia kernel (svmc_tilted_cond_payoff_chain; the header states the
// estimator, the keep rule, the recentring and the degenerate cases).  Four launches on one uploaded table:
//   tilted_cond_forward_kernel, tilted_cond_forward_finish_kernel   the statements of row f11's forward pass (svmc_cmc.hip): per
//                                expiry the sums of exp(mu + cv/2) - 1 and the kept count in the same blocks and the same order, so
//                                that corr is svmc_cmc_payoff_chain's to the bit; then K' = K + corr and ln K' once per strike
//   tilted_cond_payoff_kernel    block (path block, group of up to TC_KT strikes of one expiry, gamma): a thread forms per path
//                                sd and 1 / sd, the weight W and ln F_t once, then per strike the Black-76 price B and the sums of
//                                W d, (W d)^2, W (W d), d = B - shift; the expiry's seven statistics sums ride in the same block
//                                sum and are stored by the expiry's first group
//   tilted_cond_finish_kernel    a block per (quote | expiry, gamma): the column sums in row order, price, error, statistics
// The path blocks are quote_rows(n_path), a function of the path count alone; a strike's accumulators do not look at its
// neighbours' and the block sum's tree is the same for every accumulator index: a gamma's, an expiry's and a strike's results
// are the same bits whichever others share the call.  No atomics, no scratch, LDS for the block sums' exchange only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "svmc_ext.h"

#include "svmc_tilted_cond.h"

namespace svmc {

constexpr int TC_KT = 8;               // strikes per group: three accumulators and three constants per strike in vector registers
constexpr int TC_NSTAT = 7;            // [sum W, sum W^2, sum (W-1)^2, sum W ds, sum W^2 ds, sum (W ds)^2, kept], ds = F_t - corr - F
constexpr int TC_STAT_COLS = 8;        // ... padded: an expiry's statistics columns start at a multiple of 64 bytes
constexpr int TC_PAY_COLS = 3;         // per quote [sum W d, sum (W d)^2, sum W^2 d]
constexpr int TC_MAX_GROUPS = 65535;   // the groups are a grid's y dimension

// the device table of a call; the image (expiries .. gammas) is uploaded once
struct TcTable {
    const TcExpiry *expiries;          // [m]
    const QuoteGroup *groups;          // [G] groups of up to TC_KT strikes; pad = 1: the expiry's first, which stores its statistics
                                       // sums (an expiry without strikes has one group of nk = 0 for them)
    const double *strikes;             // [K]
    const double *is_put;              // [K] 0 | 1
    const double *shift;               // [K] the host's shift of a strike's sums
    const double *gammas;              // [NG]
    double *kp, *ln_kp;                // [K] device-computed: K + corr, its logarithm (0 where K + corr <= 0)
    double *fwd;                       // [m][4]: sum (e - 1), sum (e - 1)^2, kept count of f11's rule, corr
    double *fwd_partials;              // [rows][m][3]
    double *pay_partials;              // [rows][NG][K][TC_PAY_COLS]
    double *stat_partials;             // [rows][NG][m][TC_STAT_COLS]
    double *out;                       // prices [NG][K], errors [NG][K], statistics [NG][m][SVMC_TILTED_STATS_DOUBLES]: one block
    int m, K, NG;
    unsigned rows;
};
struct TcImage {
    TcExpiry *expiries;
    QuoteGroup *groups;
    double *strikes, *is_put, *shift, *gammas;
};
inline TcImage tc_image(Layout &w, int m, size_t K, int G, int NG)
{
    return TcImage{w.take<TcExpiry>(m), w.take<QuoteGroup>(G), w.take<double>(K), w.take<double>(K), w.take<double>(K),
                   w.take<double>(NG)};                    // (a braced list: in this order)
}
inline size_t tc_out_doubles(int m, size_t K, int NG)
{
    return static_cast<size_t>(NG) * (2 * K + static_cast<size_t>(SVMC_TILTED_STATS_DOUBLES) * m);
}
// ONE walk that is both the workspace's byte count and its carving: the image, the forward pass's head, the results, the partials.
// Returns the bytes of the image, which the walk starts with.
inline size_t tc_workspace(Layout &w, size_t n_path, int m, size_t K, int G, int NG, TcTable &t)
{
    const size_t rows = quote_rows(n_path);
    const TcImage im = tc_image(w, m, K, G, NG);
    const size_t image_bytes = w.bytes();
    t.expiries = im.expiries;
    t.groups = im.groups;
    t.strikes = im.strikes;
    t.is_put = im.is_put;
    t.shift = im.shift;
    t.gammas = im.gammas;
    t.kp = w.take<double>(K);
    t.ln_kp = w.take<double>(K);
    t.fwd = w.take<double>(4 * static_cast<size_t>(m));
    t.out = w.take<double>(tc_out_doubles(m, K, NG));
    t.fwd_partials = w.take<double>(rows * 3 * m);
    t.pay_partials = w.take<double>(rows * NG * K * TC_PAY_COLS);
    t.stat_partials = w.take<double>(rows * NG * m * TC_STAT_COLS);
    t.m = m;
    t.K = static_cast<int>(K);
    t.NG = NG;
    t.rows = static_cast<unsigned>(rows);
    return image_bytes;
}

// tc_keep_cmc, tc_black, tc_weight_forward and the forward pass's two bodies: svmc_tilted_cond.h, shared with svmc_est.hip (row f18)

// ---- the forward pass: cmc_forward_kernel's and cmc_forward_finish_kernel's statements ------------------------------------------
__global__ __launch_bounds__(BLOCK) void tilted_cond_forward_kernel(TcTable t, size_t n)
{
    __shared__ double lds[4 * 3];
    tc_forward_body(t, n, lds);
}

// a block per expiry: the three column sums in row order, corr, and -- once per strike -- K' = K + corr and ln K'
__global__ __launch_bounds__(BLOCK) void tilted_cond_forward_finish_kernel(TcTable t, int recenter)
{
    __shared__ double lds[4];
    tc_forward_finish_body(t, recenter, lds);
}

// ---- the weighted Black-76 sums -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void tilted_cond_payoff_kernel(TcTable t, size_t n)
{
    constexpr int NV = TC_PAY_COLS * TC_KT + TC_NSTAT;
    constexpr int NSUM = block_sum_padded(NV);
    __shared__ double lds[4 * NSUM];
    const QuoteGroup g = t.groups[blockIdx.y];
    const TcExpiry ex = t.expiries[g.expiry];
    const int nk = g.nk;                                   // (block-uniform; 0: the group only forms the statistics)
    const double gamma = t.gammas[blockIdx.z];
    const double corr = t.fwd[4 * g.expiry + 3];
    const double half_g2 = 0.5 * gamma * gamma, g_half = gamma + 0.5;
    double kp[TC_KT], ln_kp[TC_KT], shift[TC_KT], acc[NSUM];
    bool put[TC_KT];
#pragma unroll
    for (int j = 0; j < NSUM; ++j) acc[j] = 0.0;
#pragma unroll
    for (int k = 0; k < TC_KT; ++k) {
        const int kk = g.k0 + ((k < nk) ? k : 0);          // the unused strikes of a group repeat its first; their sums are dropped
        const bool on = nk > 0;                            // a group without strikes reads none
        kp[k] = on ? t.kp[kk] : 1.0;
        ln_kp[k] = on ? t.ln_kp[kk] : 0.0;
        shift[k] = on ? t.shift[kk] : 0.0;
        put[k] = on ? t.is_put[kk] != 0.0 : false;
    }
    const double forward = ex.forward, ln_forward = ex.ln_forward;
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    for (size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x; i < n; i += stride) {
        const double mu = ex.mu[i], cv = ex.cv[i];
        double h, e;
        if (!tc_keep_cmc(mu, cv, h, e)) continue;
        // once per (path, gamma): the weight and the shifted forward with its logarithm
        double w, et, ft, ln_ft;
        if (!tc_weight_forward(mu, cv, gamma, half_g2, g_half, forward, ln_forward, w, et, ft, ln_ft)) continue;
        const double sd = sqrt(cv), inv_sd = 1.0 / sd;     // once per path
        const double v = w - 1.0;
        const double wds = w * ((ft - corr) - forward);
        acc[TC_PAY_COLS * TC_KT] += w;
        acc[TC_PAY_COLS * TC_KT + 1] = fma(w, w, acc[TC_PAY_COLS * TC_KT + 1]);
        acc[TC_PAY_COLS * TC_KT + 2] = fma(v, v, acc[TC_PAY_COLS * TC_KT + 2]);
        acc[TC_PAY_COLS * TC_KT + 3] += wds;
        acc[TC_PAY_COLS * TC_KT + 4] = fma(w, wds, acc[TC_PAY_COLS * TC_KT + 4]);
        acc[TC_PAY_COLS * TC_KT + 5] = fma(wds, wds, acc[TC_PAY_COLS * TC_KT + 5]);
        acc[TC_PAY_COLS * TC_KT + 6] += 1.0;
        if (nk > 0) {
#pragma unroll
            for (int k = 0; k < TC_KT; ++k) {
                const double wd = w * (tc_black(ft, ln_ft, cv, sd, inv_sd, kp[k], ln_kp[k], put[k]) - shift[k]);
                acc[k] += wd;
                acc[TC_KT + k] = fma(wd, wd, acc[TC_KT + k]);
                acc[2 * TC_KT + k] = fma(w, wd, acc[2 * TC_KT + k]);
            }
        }
    }
    const size_t slot = static_cast<size_t>(blockIdx.x) * t.NG + blockIdx.z;               // partials[path block][gamma]
    double *pay = t.pay_partials + (slot * t.K + g.k0) * TC_PAY_COLS;
    double *stat = (g.pad != 0) ? t.stat_partials + (slot * t.m + g.expiry) * TC_STAT_COLS : nullptr;
    block_sum_apply<NSUM>(acc, lds, NV, [&](int j, double s) {
        if (j < TC_PAY_COLS * TC_KT) {
            const int which = j / TC_KT, k = j - which * TC_KT;
            if (k < nk) pay[TC_PAY_COLS * k + which] = s;
        } else if (stat != nullptr) {
            stat[j - TC_PAY_COLS * TC_KT] = s;
        }
    });
}

// A block per (column, gamma): columns [0, K) are the quotes, [K, K + m) the expiries' statistics.  The sums are the column sums of
// the partial rows in row order; price, error and statistics are formed as row f8's finish forms them (svmc_kernels.hip).
__global__ __launch_bounds__(BLOCK) void tilted_cond_finish_kernel(TcTable t, size_t n)
{
    __shared__ double lds[4];
    const int col = blockIdx.x, gi = blockIdx.y;
    const size_t K = static_cast<size_t>(t.K), m = static_cast<size_t>(t.m), NG = static_cast<size_t>(t.NG);
    const size_t ld_stat = NG * m * TC_STAT_COLS, ld_pay = NG * K * TC_PAY_COLS;
    int i = col - t.K;                                     // the expiry (block-uniform)
    if (col < t.K) {
        i = 0;
        while (i + 1 < t.m && col >= t.expiries[i].k1) ++i;            // expiries without strikes are skipped over
    }
    const double *st = t.stat_partials + (static_cast<size_t>(gi) * m + i) * TC_STAT_COLS;
    double s[TC_NSTAT];
    if (col < t.K) {
        // the expiry's sum W, sum W^2 and kept count, then the quote's three columns
        const double *pay = t.pay_partials + (static_cast<size_t>(gi) * K + col) * TC_PAY_COLS;
        s[0] = block_column_sum(st, t.rows, ld_stat, lds);
        __syncthreads();
        s[1] = block_column_sum(st + 1, t.rows, ld_stat, lds);
        __syncthreads();
        s[2] = block_column_sum(st + 6, t.rows, ld_stat, lds);
#pragma unroll
        for (int q = 0; q < TC_PAY_COLS; ++q) {
            __syncthreads();
            s[3 + q] = block_column_sum(pay + q, t.rows, ld_pay, lds);
        }
        if (threadIdx.x != 0) return;
        // price = shift + sum W d / sum W; sum (W (B - price))^2 = sum (W d)^2 - 2 e sum W^2 d + e^2 sum W^2, e = price - shift.
        // One kept path: the estimate IS that path's price and the squares about it are zero identically
        const double W = s[0], Q = s[1], kept = s[2];
        const double e = s[3] / W;
        const double var = (kept > 1.0) ? fma(e, fma(e, Q, -2.0 * s[5]), s[4]) : 0.0;
        t.out[gi * K + col] = e + t.shift[col];
        t.out[NG * K + gi * K + col] = sqrt(fmax(var, 0.0)) / W;
        return;
    }
#pragma unroll
    for (int q = 0; q < TC_NSTAT; ++q) {
        if (q > 0) __syncthreads();
        s[q] = block_column_sum(st + q, t.rows, ld_stat, lds);
    }
    if (threadIdx.x != 0) return;
    const double W = s[0], Q = s[1], V2 = s[2], D0 = s[3], D1 = s[4], D2 = s[5], kept = s[6];
    // normalizer n / sum W, a ratio of sums: error sqrt(sum (1 - N W)^2) / sum W = N sqrt(sum (W - mean W)^2) / sum W, the squares
    // about the mean from the sums of W - 1; gamma forward = F + sum W ds / sum W, its error as a strike's
    const double N = kept / W, sv = W - kept;
    const double dev2 = (kept > 1.0) ? V2 - sv * sv / kept : 0.0;
    const double gd = D0 / W;
    const double varg = (kept > 1.0) ? fma(gd, fma(gd, Q, -2.0 * D1), D2) : 0.0;
    double *out = t.out + 2 * NG * K + (static_cast<size_t>(gi) * m + i) * SVMC_TILTED_STATS_DOUBLES;
    out[0] = N;
    out[1] = N * sqrt(fmax(dev2, 0.0)) / W;
    out[2] = t.expiries[i].forward + gd;
    out[3] = sqrt(fmax(varg, 0.0)) / W;
    out[4] = (W / Q) * W;                                  // effective sample size (sum W)^2 / sum W^2
    out[5] = kept;
    out[6] = static_cast<double>(n) - kept;
    out[7] = W;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static bool tc_sizes_ok(size_t n_path, int n_expiries, int n_gammas)
{
    return n_path >= 1 && n_expiries >= 1 && n_gammas >= 1 && n_gammas <= SVMC_TILTED_MAX_GAMMAS;
}

}  // namespace svmc

using namespace svmc;

extern "C" {

int svmc_ext_version(void) { return SVMC_EXT_VERSION; }

int svmc_tilted_cond_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, int n_gammas, size_t *bytes)
{
    if (bytes == nullptr || !tc_sizes_ok(n_path, n_expiries, n_gammas)) return SVMC_ERR_INVALID_ARGUMENT;
    TcTable t;
    Layout w{nullptr};
    tc_workspace(w, n_path, n_expiries, total_strikes, quote_groups_bound(n_expiries, total_strikes, TC_KT), n_gammas, t);
    *bytes = w.bytes();
    return SVMC_OK;
}

int svmc_tilted_cond_payoff_chain(const double *const *mu_snapshots_host, const double *const *cv_snapshots_host, size_t n_path,
                                  const double *forwards_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                  const double *shifts_host, const size_t *strike_offsets_host, const double *gammas_host, int n_gammas,
                                  int recenter, double *prices_host, double *stderrs_host, double *stats_host, void *workspace,
                                  size_t workspace_bytes, svmc_stream_t stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // everything is checked before anything is launched
    if (!mu_snapshots_host || !cv_snapshots_host || !forwards_host || !strikes_host || !types_host || !shifts_host ||
        !strike_offsets_host || !gammas_host || !prices_host || !stderrs_host || !stats_host || !workspace)
        return SVMC_ERR_INVALID_ARGUMENT;
    if (!tc_sizes_ok(n_path, n_expiries, n_gammas)) return SVMC_ERR_INVALID_ARGUMENT;
    const int m = n_expiries, NG = n_gammas;
    if (strike_offsets_host[0] != 0) return SVMC_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < m; ++i) {
        if (strike_offsets_host[i + 1] < strike_offsets_host[i] || strike_offsets_host[i + 1] > (static_cast<size_t>(1) << 30))
            return SVMC_ERR_INVALID_ARGUMENT;
        if (!mu_snapshots_host[i] || !cv_snapshots_host[i]) return SVMC_ERR_INVALID_ARGUMENT;
        if (!std::isfinite(forwards_host[i]) || !(forwards_host[i] > 0.0)) return SVMC_ERR_INVALID_ARGUMENT;
    }
    const size_t K = strike_offsets_host[m];
    for (int z = 0; z < NG; ++z)
        if (!std::isfinite(gammas_host[z])) return SVMC_ERR_INVALID_ARGUMENT;
    for (size_t k = 0; k < K; ++k)
        if (!std::isfinite(strikes_host[k]) || !std::isfinite(shifts_host[k])) return SVMC_ERR_INVALID_ARGUMENT;
    for (size_t k = 0; k < K; ++k)
        if (types_host[k] != SVMC_CALL && types_host[k] != SVMC_PUT) return SVMC_ERR_UNKNOWN_PAYOFF;
    const int G = quote_groups(m, strike_offsets_host, TC_KT, true);
    if (G > TC_MAX_GROUPS) return SVMC_ERR_INVALID_ARGUMENT;
    TcTable t;
    Layout w{static_cast<unsigned char *>(workspace)};
    const size_t image_bytes = tc_workspace(w, n_path, m, K, G, NG, t);
    if (workspace_bytes < w.bytes()) return SVMC_ERR_WORKSPACE;

    // the table's host image, then ONE upload
    std::vector<unsigned char> image(image_bytes);
    Layout h{image.data()};
    const TcImage im = tc_image(h, m, K, G, NG);
    quote_image(
        m, strike_offsets_host,
        [&](int i, int k0, int k1) {
            im.expiries[i] = TcExpiry{mu_snapshots_host[i], cv_snapshots_host[i], forwards_host[i], std::log(forwards_host[i]), k0, k1};
        },
        [&](int, int k) {
            im.strikes[k] = strikes_host[k];
            im.is_put[k] = (types_host[k] == SVMC_PUT) ? 1.0 : 0.0;
            im.shift[k] = shifts_host[k];
        });
    quote_groups(m, strike_offsets_host, TC_KT, true, im.groups);
    for (int z = 0; z < NG; ++z) im.gammas[z] = gammas_host[z];
#define SVMC_EXT_TRY(call)                       \
    do {                                         \
        if ((call) != hipSuccess) return SVMC_ERR_HIP; \
    } while (0)
    SVMC_EXT_TRY(hipMemcpyAsync(workspace, image.data(), image_bytes, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(tilted_cond_forward_kernel, dim3(t.rows, m), dim3(BLOCK), 0, stream, t, n_path);
    SVMC_EXT_TRY(hipGetLastError());
    hipLaunchKernelGGL(tilted_cond_forward_finish_kernel, dim3(m), dim3(BLOCK), 0, stream, t, recenter ? 1 : 0);
    SVMC_EXT_TRY(hipGetLastError());
    hipLaunchKernelGGL(tilted_cond_payoff_kernel, dim3(t.rows, G, NG), dim3(BLOCK), 0, stream, t, n_path);
    SVMC_EXT_TRY(hipGetLastError());
    hipLaunchKernelGGL(tilted_cond_finish_kernel, dim3(static_cast<unsigned>(K) + m, NG), dim3(BLOCK), 0, stream, t, n_path);
    SVMC_EXT_TRY(hipGetLastError());
    // ONE download of the results' block, ONE synchronise
    std::vector<double> out(tc_out_doubles(m, K, NG));
    SVMC_EXT_TRY(hipMemcpyAsync(out.data(), t.out, out.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    SVMC_EXT_TRY(hipStreamSynchronize(stream));
#undef SVMC_EXT_TRY
    const size_t GK = static_cast<size_t>(NG) * K;
    if (GK > 0) {
        memcpy(prices_host, out.data(), GK * sizeof(double));
        memcpy(stderrs_host, out.data() + GK, GK * sizeof(double));
    }
    memcpy(stats_host, out.data() + 2 * GK, static_cast<size_t>(NG) * m * SVMC_TILTED_STATS_DOUBLES * sizeof(double));
    return SVMC_OK;
}

}  // extern "C"
