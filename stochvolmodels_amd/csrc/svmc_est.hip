// svmc_est.hip -- libsvmc_est.so, the estimators beside the core (include/svmc_est.h states the rule that keeps this library
// open).  One translation unit on the header-only parts of csrc/; nothing of libsvmc.so or libsvmc_ext.so
// is linked and no session is needed.  Three estimators: the Greeks under the risk-premia kernel (below), the mixture density of
// the log-return (svmc_cond_density_chain: its block further down states its three launches) and many (sigma, gamma) sets on one set
// of jump rows (svmc_jump_sets_payoff_chain, row f20: its block after that).
//
// Conditional Monte Carlo Greeks under the exponential risk-premia kernel (svmc_tilted_cond_greeks_chain; the header states the
// estimator, the degenerate cases and the two identities).  Four launches on one uploaded table:
//   tilted_cond_greeks_forward_kernel, tilted_cond_greeks_forward_finish_kernel
//                                the forward pass of rows f11 / f17, the SAME statements (svmc_tilted_cond.h): corr, K' = K + corr
//                                and ln K' are svmc_tilted_cond_payoff_chain's to the bit
//   tilted_cond_greeks_kernel    block (path block, group of up to TCG_KT strikes of one expiry, gamma): a thread forms per path
//                                sd and 1 / sd, the weight W, ln F_t and e_t once, then per strike two normal CDFs and one exp for
//                                phi(d2) and, for each of delta, dual delta and dual gamma, the sums of W d, (W d)^2, W (W d),
//                                d = v - shift: nine fused accumulations; the (expiry, gamma) statistics sums ride in the same
//                                block sum and are stored by the expiry's first group
//   tilted_cond_greeks_finish_kernel   a block per (quote | expiry, gamma): the column sums in row order, values, errors, statistics
// The path blocks are quote_rows(n_path), a function of the path count alone; a strike's accumulators do not look at its
// neighbours' and the block sum's tree is the same for every accumulator index: a gamma's, an expiry's and a strike's results
// are the same bits whichever others share the call, and sum W and the kept count are row f17's bits.  No atomics, no scratch,
// LDS for the block sums' exchange only.
// What the three share with each other and with libsvmc_ext.so -- the forward pass, the strike-group preload, the payoff and finish
// bodies, the finish kernels' pieces, the table's walk and the host's check and driver -- is svmc_tilted_cond.h's.
#include <hip/hip_runtime.h>

#include "svmc_est.h"

#include "svmc_tilted_cond.h"

namespace svmc {

// Strikes per group.  A strike carries nine accumulators and five constants in vector registers (row f17's payoff kernel: three and
// three at eight strikes).  At 4 the kernel takes 160 VGPRs: THREE waves per SIMD, one fewer than row f17's payoff kernel has at 128 --
// the occupancy is not kept.  Measured on the MI355X (profiles/hawkes_tilted_cond_greeks_bench.json, "kt"): 8 (262 VGPRs, one wave) takes
// 1.5 to 1.9 times as long; 2 (107 VGPRs, four waves) is within 2 % of 4, mostly behind it: what a fourth wave hides, forming the
// per-path terms twice as often costs.
#ifndef SVMC_TCG_KT
#define SVMC_TCG_KT 4
#endif
constexpr int TCG_KT = SVMC_TCG_KT;
constexpr int TCG_COLS = 9;            // per quote, for v = delta, dual delta, dual gamma: [sum W d, sum (W d)^2, sum W^2 d]
constexpr int TCG_NSTAT = 4;           // per (expiry, gamma): [sum W, sum W^2, kept, kept with cv == 0]

// the device table of a call (svmc_tilted_cond.h): zs the gammas [NG]; shift [K] s 1{s (F - K) > 0}, the shift of delta's sums (dual
// delta's is its negative); q_partials [rows][NG][K][TCG_COLS], stat_partials [rows][NG][m][TCG_NSTAT]; out: greeks
// [NG][SVMC_TCG_ROWS][K], statistics [NG][m][SVMC_TCG_STATS_DOUBLES]
struct TcgTable : TcTableOf<double> {};
inline size_t tcg_out_doubles(int m, size_t K, int NG)
{
    return static_cast<size_t>(NG) * (SVMC_TCG_ROWS * K + static_cast<size_t>(SVMC_TCG_STATS_DOUBLES) * m);
}
inline size_t tcg_workspace(Layout &w, size_t n_path, int m, size_t K, int G, int NG, TcgTable &t)
{
    return tc_workspace(w, n_path, m, K, G, NG, NG, tcg_out_doubles(m, K, NG), TCG_COLS, TCG_NSTAT, t);
}

// ---- the forward pass: rows f11's / f17's statements (svmc_tilted_cond.h) ---------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void tilted_cond_greeks_forward_kernel(TcgTable t, size_t n)
{
    __shared__ double lds[4 * 3];
    tc_forward_body<false>(t, n, lds);
}

__global__ __launch_bounds__(BLOCK) void tilted_cond_greeks_forward_finish_kernel(TcgTable t, int recenter)
{
    __shared__ double lds[4];
    tc_forward_finish_body(t, recenter, lds);
}

// ---- the weighted Black-76 derivatives ----------------------------------------------------------------------------------------------
// Per kept path and strike (B_f, B_k, dual_gamma_j) as row f13's cmc_derivs forms them (svmc_cmc.hip), at the shifted forward: each
// side's B_f and B_k come from its own tail (put: B_f = -N(-d1), B_k = N(-d2)), as its price does.
__device__ __forceinline__ void tcg_derivs(double ft, double ln_ft, double cv, double sd, double inv_sd, double kp, double ln_kp,
                                           double inv_kp, bool put, double &bf, double &bk, double &dg)
{
    dg = 0.0;
    if (!(kp > 0.0)) {
        bf = put ? 0.0 : 1.0;
        bk = -bf;
    } else if (cv == 0.0) {
        const bool itm = put ? (ft < kp) : (ft > kp);      // strict: a tie has payoff 0 and indicator 0
        bf = itm ? (put ? -1.0 : 1.0) : 0.0;
        bk = -bf;
    } else {
        const double d1 = fma(ln_ft - ln_kp, inv_sd, 0.5 * sd), d2 = d1 - sd;
        bf = put ? -black_norm_cdf(-d1) : black_norm_cdf(d1);
        bk = put ? black_norm_cdf(-d2) : -black_norm_cdf(d2);
        dg = (exp_full((-0.5 * d2) * d2) * 0.39894228040143267794) * (inv_sd * inv_kp);
    }
}

template <int KT>
__global__ __launch_bounds__(BLOCK) void tilted_cond_greeks_kernel(TcgTable t, size_t n, int recenter)
{
    constexpr int NQ = TCG_COLS * KT;
    constexpr int NV = NQ + TCG_NSTAT;
    constexpr int NSUM = block_sum_padded(NV);
    __shared__ double lds[4 * NSUM];
    const QuoteGroup g = t.groups[blockIdx.y];
    const TcExpiry ex = t.expiries[g.expiry];
    const int nk = g.nk;                                   // (block-uniform; 0: the group only forms the statistics)
    const double gamma = t.zs[blockIdx.z];
    const double *fw = t.fwd + 4 * g.expiry;
    const double c = recenter ? fw[0] / fw[2] : 0.0;       // mean_kept(e) - 1, the quotient the forward finish forms: corr = F c
    const double half_g2 = 0.5 * gamma * gamma, g_half = gamma + 0.5;
    double kp[KT], ln_kp[KT], inv_kp[KT], dshift[KT], acc[NSUM];
    bool put[KT];
#pragma unroll
    for (int j = 0; j < NSUM; ++j) acc[j] = 0.0;
    tc_group_preload(t, g, kp, ln_kp, dshift, put);
#pragma unroll
    for (int k = 0; k < KT; ++k) inv_kp[k] = 1.0 / kp[k];
    const double forward = ex.forward, ln_forward = ex.ln_forward;
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    for (size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x; i < n; i += stride) {
        const double mu = ex.mu[i], cv = ex.cv[i];
        double h, e;
        if (!tc_keep_cmc(mu, cv, h, e)) continue;
        // once per (path, gamma): the weight, e_t and the shifted forward with its logarithm
        double w, et, ft, ln_ft;
        if (!tc_weight_forward(mu, cv, gamma, half_g2, g_half, forward, ln_forward, w, et, ft, ln_ft)) continue;
        const double sd = sqrt(cv), inv_sd = 1.0 / sd;     // once per path
        acc[NQ] += w;
        acc[NQ + 1] = fma(w, w, acc[NQ + 1]);
        acc[NQ + 2] += 1.0;
        if (cv == 0.0) acc[NQ + 3] += 1.0;
        if (nk > 0) {
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                double bf, bk, dg;
                tcg_derivs(ft, ln_ft, cv, sd, inv_sd, kp[k], ln_kp[k], inv_kp[k], put[k], bf, bk, dg);
                const double v[3] = {fma(et, bf, c * bk) - dshift[k], bk + dshift[k], dg};
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const double wd = w * v[q];
                    acc[(3 * q) * KT + k] += wd;
                    acc[(3 * q + 1) * KT + k] = fma(wd, wd, acc[(3 * q + 1) * KT + k]);
                    acc[(3 * q + 2) * KT + k] = fma(w, wd, acc[(3 * q + 2) * KT + k]);
                }
            }
        }
    }
    const size_t slot = static_cast<size_t>(blockIdx.x) * t.NG + blockIdx.z;               // partials[path block][gamma]
    double *qp = t.q_partials + (slot * t.K + g.k0) * TCG_COLS;
    double *stat = (g.pad != 0) ? t.stat_partials + (slot * t.m + g.expiry) * TCG_NSTAT : nullptr;
    block_sum_apply<NSUM>(acc, lds, NV, [&](int j, double s) {
        if (j < NQ) {
            const int which = j / KT, k = j - which * KT;
            if (k < nk) qp[TCG_COLS * k + which] = s;
        } else if (stat != nullptr) {
            stat[j - NQ] = s;
        }
    });
}

// A block per (column, gamma): columns [0, K) are the quotes, [K, K + m) the expiries' statistics.  The sums are the column sums of
// the partial rows in row order; a value and its error are formed as row f17's finish forms a price and its error.
__global__ __launch_bounds__(BLOCK) void tilted_cond_greeks_finish_kernel(TcgTable t, size_t n)
{
    __shared__ double lds[4];
    const int col = blockIdx.x, gi = blockIdx.y;
    const size_t K = static_cast<size_t>(t.K), m = static_cast<size_t>(t.m), NG = static_cast<size_t>(t.NG);
    const size_t ld_stat = NG * m * TCG_NSTAT, ld_q = NG * K * TCG_COLS;
    const int i = tc_expiry_of_column(t.expiries, t.m, t.K, col);
    const double *st = t.stat_partials + (static_cast<size_t>(gi) * m + i) * TCG_NSTAT;
    double s[TCG_NSTAT];
    tc_column_sums(st, {0, 1, 2, 3}, t.rows, ld_stat, lds, s);
    const double W = s[0], Q = s[1], kept = s[2];
    if (col >= t.K) {
        if (threadIdx.x != 0) return;
        double *out = t.out + NG * SVMC_TCG_ROWS * K + (static_cast<size_t>(gi) * m + i) * SVMC_TCG_STATS_DOUBLES;
        out[0] = W;
        out[1] = kept;
        out[2] = static_cast<double>(n) - kept;
        out[3] = s[3];
        return;
    }
    const double *qp = t.q_partials + (static_cast<size_t>(gi) * K + col) * TCG_COLS;
    double c[TCG_COLS];
#pragma unroll
    for (int q = 0; q < TCG_COLS; ++q) {
        __syncthreads();
        c[q] = block_column_sum(qp + q, t.rows, ld_q, lds);
    }
    if (threadIdx.x != 0) return;
    const double dshift = t.shift[col];
    const double shift[3] = {dshift, -dshift, 0.0};
    double v[3], err[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        double e;                                          // value = shift + e
        tc_value_error(c[3 * q], c[3 * q + 1], c[3 * q + 2], W, Q, kept, e, err[q]);
        v[q] = e + shift[q];
    }
    const double r = t.strikes[col] / t.expiries[i].forward, r2 = r * r;
    double *out = t.out + static_cast<size_t>(gi) * SVMC_TCG_ROWS * K + col;
    out[0] = v[0];
    out[K] = err[0];
    out[2 * K] = v[1];
    out[3 * K] = err[1];
    out[4 * K] = r2 * v[2];
    out[5 * K] = r2 * err[2];
    out[6 * K] = v[2];
    out[7 * K] = err[2];
}

// ---- the mixture density of the log-return (svmc_cond_density_chain; the header states the estimator) --------------
// Three launches on one uploaded table:
//   cond_density_weight_kernel   block (path block, expiry, gamma): W = exp(gamma mu + gamma^2 cv / 2) once per (path, gamma), stored
//                                as a row of the workspace (0 for a path that f11's rule drops or whose W^2 is not finite), with the
//                                (expiry, gamma) statistics sums -- row f18's statements and order, hence its bits
//   cond_density_kernel          block (path block, group of up to CD_XT points of one expiry, tile of gammas): a thread forms
//                                per path 1 / sd and 1 / (sd sqrt(2 pi)) once and reads the tile's weights, then per point z and ONE exp
//                                for n = N(x; mu, cv), n and n^2 into S1 and S2 (stored by the first tile only) and per gamma one FMA
//                                into C: no exp and no CDF per (path, point, gamma)
//   cond_density_finish_kernel   a block per (point | expiry, gamma): the column sums in row order, e^{gamma x} once, pdf, error, statistics
// Every accumulator is one (point) or one (point, gamma) and the block sum's tree is the same for every accumulator index: a gamma's, an
// expiry's and a point's results are the same bits whichever others share the call, whatever the tiles are.
//
// Points per thread and gammas per tile, chosen by measurement on the MI355X (profiles/cond_density_bench.json, "variants": the tail for
// 200 points at 10^5 | 2^20 paths, ms for 1 / 5 / 16 gammas; VGPRs and waves per SIMD of this kernel from the ISA metadata).  The
// accumulators are XT (2 + GT) doubles in the first tile.
//   XT, GT   VGPRs  waves   10^5 paths             2^20 paths
//   2, 4       68     7     0.163 0.267 0.545      0.668 1.317 3.048
//   4, 2       76     6     0.129 0.239 0.559      0.474 1.209 3.001
//   4, 4       96     5     0.139 0.214 0.421      0.523 0.941 2.019
//   8, 4      153     3     0.151 0.230 0.434      0.469 0.852 1.664
//   4, 8      141     3     0.196 0.216 0.401      0.661 0.724 1.525
//   8, 8      223     2     0.202 0.219 0.405      0.643 0.725 1.394
//   2, 16     137     3     0.325 0.349 0.437      1.190 1.344 2.703
//   4, 16     215     2     0.312 0.325 0.403      1.004 1.121 1.411
// No one tile serves every count: a tile wider than the call wastes its FMAs and its registers on gammas nobody asked for (one gamma at
// GT = 8: 1.3 to 1.4 times GT = 4's time), a narrower one repeats the exp per tile (five gammas at GT = 4: 1.3 times GT = 8's at 2^20
// paths).  So the host picks the tile by the call's gamma count -- CD_GT for up to CD_GT gammas, CD_GT_WIDE beyond: 0.141 0.210 0.378 |
// 0.510 0.785 1.598 ms in that run -- which changes no bit: an accumulator is one (point, gamma) whatever the tile, and a thread adds the
// same paths in the same order.  XT = 8 is no better than 4 at either tile beyond 10 % at one gamma and 2^20 paths, and costs the waves.
// THE WEIGHTS.  The other design forms W in the block, one exp per (path, gamma) and point group, and needs no pre-pass and no rows.
// Measured in the same run with a build that is not kept, the statistics pass left in: at (4, 4) 0.164 0.257 0.479 | 0.699 1.241 2.447 ms,
// 1.14 to 1.34 times the pre-pass's; at (8, 8) 1.04 to 1.24 times; at (4, 16) 1.06 to 1.59 times.  With 200 points in groups of 4 a block
// repeats for 50 groups what the pre-pass does once, and the row it reads back is 8 bytes per (path, gamma) beside XT exponentials.  The
// pre-pass is kept.
#ifndef SVMC_CD_XT
#define SVMC_CD_XT 4
#endif
#ifndef SVMC_CD_GT
#define SVMC_CD_GT 4
#endif
#ifndef SVMC_CD_GT_WIDE
#define SVMC_CD_GT_WIDE 8
#endif
constexpr int CD_XT = SVMC_CD_XT;
constexpr int CD_GT = SVMC_CD_GT;
constexpr int CD_GT_WIDE = SVMC_CD_GT_WIDE;
constexpr int CD_NSTAT = 8;            // per (expiry, gamma): [sum W, sum W^2, kept, kept with cv == 0, kept with W^2 not finite], zeros
                                       // up to eight: the block sum's halving tree, row f18's

struct CdExpiry {
    const double *mu, *cv;
    int k0, k1;                        // its points [k0, k1)
};
// the device table of a call; the image (expiries .. gammas) is uploaded once
struct CdTable {
    const CdExpiry *expiries;          // [m]
    const QuoteGroup *groups;          // [G] groups of up to CD_XT points of one expiry
    const double *points;              // [P]
    const double *gammas;              // [NG]
    double *weights;                   // [m][NG][n]
    double *s_partials;                // [rows][P][2]: S1, S2
    double *c_partials;                // [rows][NG][P]
    double *stat_partials;             // [rows][NG][m][CD_NSTAT]
    double *out;                       // pdf [NG][P], errors [NG][P], statistics [NG][m][SVMC_CD_STATS_DOUBLES]: one block
    int m, P, NG;
    unsigned rows;
};
struct CdImage {
    CdExpiry *expiries;
    QuoteGroup *groups;
    double *points, *gammas;
};
inline CdImage cd_image(Layout &w, int m, size_t P, int G, int NG)
{
    return CdImage{w.take<CdExpiry>(m), w.take<QuoteGroup>(G), w.take<double>(P), w.take<double>(NG)};     // (in this order)
}
inline size_t cd_out_doubles(int m, size_t P, int NG) { return static_cast<size_t>(NG) * (2 * P + static_cast<size_t>(SVMC_CD_STATS_DOUBLES) * m); }
// ONE walk that is both the workspace's byte count and its carving; returns the bytes of the image, which the walk starts with
inline size_t cd_workspace(Layout &w, size_t n_path, int m, size_t P, int G, int NG, CdTable &t)
{
    const size_t rows = quote_rows(n_path);
    const CdImage im = cd_image(w, m, P, G, NG);
    const size_t image_bytes = w.bytes();
    t.expiries = im.expiries;
    t.groups = im.groups;
    t.points = im.points;
    t.gammas = im.gammas;
    t.out = w.take<double>(cd_out_doubles(m, P, NG));
    t.s_partials = w.take<double>(rows * P * 2);
    t.c_partials = w.take<double>(rows * NG * P);
    t.stat_partials = w.take<double>(rows * NG * m * CD_NSTAT);
    t.weights = w.take<double>(static_cast<size_t>(m) * NG * n_path);
    t.m = m;
    t.P = static_cast<int>(P);
    t.NG = NG;
    t.rows = static_cast<unsigned>(rows);
    return image_bytes;
}

// grid (path blocks, expiries, gammas)
__global__ __launch_bounds__(BLOCK) void cond_density_weight_kernel(CdTable t, size_t n)
{
    __shared__ double lds[4 * CD_NSTAT];
    constexpr double INF = __builtin_huge_val();
    const CdExpiry ex = t.expiries[blockIdx.y];
    const double gamma = t.gammas[blockIdx.z];
    const double half_g2 = 0.5 * gamma * gamma;
    double *wrow = t.weights + (static_cast<size_t>(blockIdx.y) * t.NG + blockIdx.z) * n;
    double acc[CD_NSTAT];
#pragma unroll
    for (int j = 0; j < CD_NSTAT; ++j) acc[j] = 0.0;
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    for (size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x; i < n; i += stride) {
        const double mu = ex.mu[i], cv = ex.cv[i];
        double h, e, w = 0.0;
        if (tc_keep_cmc(mu, cv, h, e)) {
            w = exp_full(fma(half_g2, cv, gamma * mu));    // tc_weight_forward's statement: gamma = 0 gives exp(0) = 1
            acc[2] += 1.0;
            if (cv == 0.0) acc[3] += 1.0;
            if (w * w < INF) {
                acc[0] += w;
                acc[1] = fma(w, w, acc[1]);
            } else {
                acc[4] += 1.0;
                w = 0.0;
            }
        }
        wrow[i] = w;
    }
    const size_t slot = static_cast<size_t>(blockIdx.x) * t.NG + blockIdx.z;               // partials[path block][gamma]
    block_sum_store<CD_NSTAT>(acc, lds, t.stat_partials + (slot * t.m + blockIdx.y) * CD_NSTAT, CD_NSTAT);
}

// FIRST: the tile that holds S1 and S2
template <int XT, int GT, bool FIRST>
__device__ __forceinline__ void cond_density_body(const CdTable &t, size_t n, double *lds)
{
    constexpr int NS = FIRST ? 2 * XT : 0;
    constexpr int NV = NS + XT * GT;
    constexpr int NSUM = block_sum_padded(NV);
    const QuoteGroup g = t.groups[blockIdx.y];
    const CdExpiry ex = t.expiries[g.expiry];
    const int nk = g.nk;                                   // (block-uniform, >= 1)
    const int g0 = static_cast<int>(blockIdx.z) * GT, ng = min(GT, t.NG - g0);
    double x[XT], acc[NSUM];
    const double *wrow[GT];
#pragma unroll
    for (int j = 0; j < NSUM; ++j) acc[j] = 0.0;
#pragma unroll
    for (int k = 0; k < XT; ++k) x[k] = t.points[g.k0 + ((k < nk) ? k : 0)];      // the unused points of a group repeat its first
#pragma unroll
    for (int q = 0; q < GT; ++q)                                                  // ... and the unused gammas of a tile likewise
        wrow[q] = t.weights + (static_cast<size_t>(g.expiry) * t.NG + g0 + ((q < ng) ? q : 0)) * n;
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    for (size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x; i < n; i += stride) {
        const double mu = ex.mu[i], cv = ex.cv[i];
        double w[GT];
#pragma unroll
        for (int q = 0; q < GT; ++q) w[q] = wrow[q][i];
        double h, e;
        if (!tc_keep_cmc(mu, cv, h, e) || cv == 0.0) continue;         // a point mass adds nothing to any x-sum
        const double inv_sd = 1.0 / sqrt(cv), f = inv_sd * 0.39894228040143267794;         // once per path
#pragma unroll
        for (int k = 0; k < XT; ++k) {
            const double z = (x[k] - mu) * inv_sd;
            const double nn = exp_full((-0.5 * z) * z) * f;
            if constexpr (FIRST) {
                acc[k] += nn;
                acc[XT + k] = fma(nn, nn, acc[XT + k]);
            }
#pragma unroll
            for (int q = 0; q < GT; ++q) acc[NS + q * XT + k] = fma(w[q], nn, acc[NS + q * XT + k]);
        }
    }
    double *sp = t.s_partials + (static_cast<size_t>(blockIdx.x) * t.P + g.k0) * 2;
    double *cp = t.c_partials + (static_cast<size_t>(blockIdx.x) * t.NG + g0) * t.P + g.k0;
    const size_t P = static_cast<size_t>(t.P);
    block_sum_apply<NSUM>(acc, lds, NV, [&](int j, double s) {
        if (j < NS) {
            const int which = j / XT, k = j - which * XT;
            if (k < nk) sp[2 * k + which] = s;
        } else {
            const int q = (j - NS) / XT, k = (j - NS) - q * XT;
            if (k < nk && q < ng) cp[q * P + k] = s;
        }
    });
}

// grid (path blocks, point groups, gamma tiles)
template <int XT, int GT>
__global__ __launch_bounds__(BLOCK) void cond_density_kernel(CdTable t, size_t n)
{
    __shared__ double lds[4 * block_sum_padded(XT * (2 + GT))];
    if (blockIdx.z == 0)                                   // (block-uniform)
        cond_density_body<XT, GT, true>(t, n, lds);
    else
        cond_density_body<XT, GT, false>(t, n, lds);
}

// A block per (column, gamma): columns [0, P) are the points, [P, P + m) the expiries' statistics
__global__ __launch_bounds__(BLOCK) void cond_density_finish_kernel(CdTable t, size_t n)
{
    __shared__ double lds[4];
    const int col = blockIdx.x, gi = blockIdx.y;
    const size_t P = static_cast<size_t>(t.P), m = static_cast<size_t>(t.m), NG = static_cast<size_t>(t.NG);
    const size_t ld_stat = NG * m * CD_NSTAT;
    const int i = tc_expiry_of_column(t.expiries, t.m, t.P, col);
    const double *st = t.stat_partials + (static_cast<size_t>(gi) * m + i) * CD_NSTAT;
    double s[5];
    tc_column_sums(st, {0, 1, 2, 3, 4}, t.rows, ld_stat, lds, s);
    const double W = s[0], Q = s[1], kept = s[2], bad = s[4];
    if (col >= t.P) {
        if (threadIdx.x != 0) return;
        double *out = t.out + 2 * NG * P + (static_cast<size_t>(gi) * m + i) * SVMC_CD_STATS_DOUBLES;
        out[0] = W;
        out[1] = kept;
        out[2] = static_cast<double>(n) - kept;
        out[3] = s[3];
        out[4] = bad;
        return;
    }
    __syncthreads();
    const double s1 = block_column_sum(t.s_partials + 2 * col, t.rows, 2 * P, lds);
    __syncthreads();
    const double s2 = block_column_sum(t.s_partials + 2 * col + 1, t.rows, 2 * P, lds);
    __syncthreads();
    const double c = block_column_sum(t.c_partials + static_cast<size_t>(gi) * P + col, t.rows, NG * P, lds);
    if (threadIdx.x != 0) return;
    // tc_value_error's sums with W v = e^{gamma x} n: sum W v = e^{gamma x} S1, sum (W v)^2 = e^{2 gamma x} S2, sum W^2 v = e^{gamma x} C
    const double gamma = t.gammas[gi];
    const double eg = (gamma == 0.0) ? 1.0 : exp_full(gamma * t.points[col]);              // once per (point, gamma)
    const double nan = __builtin_nan("");
    double pdf, err;                                       // 0 / 0 -> NaN: no kept path
    tc_value_error(eg * s1, (eg * eg) * s2, eg * c, W, Q, kept, pdf, err);
    const bool ok = bad == 0.0;
    t.out[static_cast<size_t>(gi) * P + col] = ok ? pdf : nan;
    t.out[(NG + gi) * P + col] = ok ? err : nan;
}

// ---- many (sigma, gamma) sets on one set of jump rows (svmc_jump_sets_payoff_chain; the header states the estimator) ----
// Four launches on one uploaded table:
//   jump_sets_forward_kernel, jump_sets_forward_finish_kernel
//                                the forward pass of rows f11 / f17 on the rows (a, 0): tc_forward_body with the constant 0.0 where it
//                                reads cv (ZERO_CV: the table's cv is null), then tc_forward_finish_body -- corr, K' = K + corr and
//                                ln K' are svmc_cmc_payoff_chain's bits on (a, 0), ONCE for all sets
//   jump_sets_payoff_kernel      block (path block, group of up to JS_KT strikes of one expiry, set): the set's constants
//                                (g, c, v, sd, 1 / sd, F exp(g v), ln F + g v) come from the table at a block-uniform address; per path
//                                ONE 8-byte load, exp(a) and exp(g a); per strike tc_black and the sums of w d, (w d)^2, w (w d); the
//                                seven statistics sums ride in the same block sum and are stored by the expiry's first group.  The
//                                statements are tc_payoff_body's (svmc_tilted_cond.h) with this path's terms typed in: on that body, with
//                                the terms as a path policy, the kernel measured 2.3 % slower at 2^20 paths and 16 sets -- 88 to 92
//                                VGPRs for 86 and more scalars parked in vector lanes (profiles/cond_tails_refactor.txt) -- so it keeps
//                                its own
//   jump_sets_finish_kernel      tc_finish_body, a block per (quote | expiry, set): the column sums in row order, price, error, statistics
//                                in terms of W = c w, c applied here once (JsWeights), and the corr row
// Every accumulator is one (set, strike) or one (set, statistic), and a thread adds the same paths in the same order: a set's, an
// expiry's and a strike's results are the same bits whichever others share the call.
//
// THE LAYOUT, measured on the MI355X (profiles/hawkes_jump_sets_bench.json, "layouts": the tail alone on the BTC chain's 49 strikes at
// 10^5 | 2^20 paths, ms for 1 / 3 / 16 sets; VGPRs and waves per SIMD of the payoff kernel from the ISA metadata).  ST = 1 is row f17's
// layout, a block per set; ST > 1 loops the sets of a tile inside the block, so that a path's load, its keep test and exp(a) are shared,
// at ST times the accumulators.
//   KT, ST   VGPRs  waves   10^5 paths             2^20 paths
//   8, 1      119     4     0.188 0.308 1.125      0.603 1.468 7.215      row f17's group of eight
//   4, 1       86     5     0.185 0.296 1.072      0.551 1.326 6.478      kept
//   4, 2      130     3     0.241 0.351 1.091      1.000 1.875 6.900
//   8, 2      187     2     0.283 0.429 1.365      1.288 2.405 9.232
//   2, 4      158     3     0.351 0.355 1.082      1.815 1.822 6.933
//   4, 4      211     2     0.387 0.385 1.177      2.058 2.069 7.880
//   2, 8      270     1     0.969 0.971 1.895      6.714 6.721 13.37
// Sharing the load and exp(a) buys nothing: per (path, set, strike) the kernel pays two normal CDFs, per (path, set) one exp, and the
// load is 8 bytes against all of that; a tile wider than the call wastes its lanes' work on sets nobody asked for (one set at ST = 4:
// twice to nearly four times ST = 1's time) and the accumulators cost the waves.  The set-per-block layout is kept.  Within it a group of
// four strikes (19 accumulators, 86 VGPRs, five waves) is 2 to 10 % ahead of row f17's eight (31 accumulators, 119 VGPRs, four waves)
// in all six cells, in two runs that agree within 2 %: forming w and F_t twice as often costs less than the fifth wave hides.  No bit depends on either choice.
// The ST > 1 rows were measured with a build that is not kept: the kernel is a block per set and the grid's z is the set.
#ifndef SVMC_JS_KT
#define SVMC_JS_KT 4
#endif
constexpr int JS_KT = SVMC_JS_KT;      // strikes per group

// the host constants of one (set, expiry)
struct JsSet {
    double g, c, v, sd, inv_sd;        // gamma, exp(g (g - 1) v / 2), the variance, its root and the root's inverse (inf at v == 0: unused)
    double fs, ln_fs;                  // F exp(g v), ln F + g v
    double gv;                         // g v
};
// the device table of a call (svmc_tilted_cond.h): expiries with mu = a and cv = null, nothing reads it; zs the sets [Q][m];
// q_partials [rows][Q][K][TC_PAY_COLS], stat_partials [rows][Q][m][TC_STAT_COLS]; NG: the sets; out: prices [Q][K], errors [Q][K],
// statistics [Q][m][SVMC_TILTED_STATS_DOUBLES], corr [m]
struct JsTable : TcTableOf<JsSet> {};
inline size_t js_out_doubles(int m, size_t K, int Q)
{
    return static_cast<size_t>(Q) * (2 * K + static_cast<size_t>(SVMC_TILTED_STATS_DOUBLES) * m) + m;
}
inline size_t js_workspace(Layout &w, size_t n_path, int m, size_t K, int G, int Q, JsTable &t)
{
    return tc_workspace(w, n_path, m, K, G, Q, static_cast<size_t>(Q) * m, js_out_doubles(m, K, Q), TC_PAY_COLS, TC_STAT_COLS, t);
}

// row f17's statistics with W = c w, c applied once; the expiry's block of set 0 stores corr behind the statistics
struct JsWeights {
    __device__ __forceinline__ static double sum_w(const JsTable &t, int z, int i, double w)
    {
        return t.zs[static_cast<size_t>(z) * t.m + i].c * w;
    }
    __device__ __forceinline__ static void epilogue(const JsTable &t, int z, int i)
    {
        const size_t K = static_cast<size_t>(t.K), m = static_cast<size_t>(t.m), NG = static_cast<size_t>(t.NG);
        if (z == 0) t.out[NG * (2 * K + SVMC_TILTED_STATS_DOUBLES * m) + i] = t.fwd[4 * i + 3];           // corr, once per expiry
    }
};

// grid (path blocks, expiries)
__global__ __launch_bounds__(BLOCK) void jump_sets_forward_kernel(JsTable t, size_t n)
{
    __shared__ double lds[4 * 3];
    tc_forward_body<true>(t, n, lds);
}

__global__ __launch_bounds__(BLOCK) void jump_sets_forward_finish_kernel(JsTable t, int recenter)
{
    __shared__ double lds[4];
    tc_forward_finish_body(t, recenter, lds);
}

// grid (path blocks, strike groups, sets); tc_payoff_body's statements, its path's terms and strike preload typed in (above)
template <int KT>
__global__ __launch_bounds__(BLOCK) void jump_sets_payoff_kernel(JsTable t, size_t n)
{
    constexpr int NP = TC_PAY_COLS * KT, NV = NP + TC_NSTAT, NSUM = tc_payoff_sums(KT);
    constexpr double INF = __builtin_huge_val();
    __shared__ double lds[4 * NSUM];
    const QuoteGroup g = t.groups[blockIdx.y];
    const TcExpiry ex = t.expiries[g.expiry];
    const int nk = g.nk;                                   // (block-uniform; 0: the group only forms the statistics)
    const double corr = t.fwd[4 * g.expiry + 3];
    const double forward = ex.forward;
    const JsSet s = t.zs[static_cast<size_t>(blockIdx.z) * t.m + g.expiry];
    double kp[KT], ln_kp[KT], shift[KT], acc[NSUM];
    bool put[KT];
#pragma unroll
    for (int j = 0; j < NSUM; ++j) acc[j] = 0.0;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        const int kk = g.k0 + ((k < nk) ? k : 0);          // the unused strikes of a group repeat its first; their sums are dropped
        const bool on = nk > 0;                            // a group without strikes reads none
        kp[k] = on ? t.kp[kk] : 1.0;
        ln_kp[k] = on ? t.ln_kp[kk] : 0.0;
        shift[k] = on ? t.shift[kk] : 0.0;
        put[k] = on ? t.is_put[kk] != 0.0 : false;
    }
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    for (size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x; i < n; i += stride) {
        const double a = ex.mu[i];
        double h, e;
        if (!tc_keep_cmc(a, 0.0, h, e)) continue;          // f11's rule on (a, 0): a and e = exp(a) finite
        // once per (path, set): the weight and the shifted forward with its logarithm
        const double w = exp_full(s.g * a);
        const double ft = s.fs * e, ln_ft = s.ln_fs + a;
        const double W = s.c * w, wf = W * ft;
        if (!(W * W < INF && wf * wf < INF)) continue;     // (a NaN fails the comparison)
        const double v = w - 1.0;
        const double wds = w * ((ft - corr) - forward);
        double *st = acc + NP;
        st[0] += w;
        st[1] = fma(w, w, st[1]);
        st[2] = fma(v, v, st[2]);
        st[3] += wds;
        st[4] = fma(w, wds, st[4]);
        st[5] = fma(wds, wds, st[5]);
        st[6] += 1.0;
        if (nk > 0) {
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const double wd = w * (tc_black(ft, ln_ft, s.v, s.sd, s.inv_sd, kp[k], ln_kp[k], put[k]) - shift[k]);
                acc[k] += wd;
                acc[KT + k] = fma(wd, wd, acc[KT + k]);
                acc[2 * KT + k] = fma(w, wd, acc[2 * KT + k]);
            }
        }
    }
    const bool first = g.pad != 0;
    block_sum_apply<NSUM>(acc, lds, NV, [&](int j, double sum) {
        const size_t slot = static_cast<size_t>(blockIdx.x) * t.NG + blockIdx.z;           // partials[path block][set]
        if (j < NP) {
            const int which = j / KT, k = j - which * KT;
            if (k < nk) t.q_partials[(slot * t.K + g.k0 + k) * TC_PAY_COLS + which] = sum;
        } else if (first) {
            t.stat_partials[(slot * t.m + g.expiry) * TC_STAT_COLS + (j - NP)] = sum;
        }
    });
}

// a block per (column, set): columns [0, K) are the quotes, [K, K + m) the expiries' statistics
__global__ __launch_bounds__(BLOCK) void jump_sets_finish_kernel(JsTable t, size_t n)
{
    __shared__ double lds[4];
    tc_finish_body<JsWeights>(t, n, lds);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static bool tcg_sizes_ok(size_t n_path, int n_expiries, int n_gammas)
{
    return n_path >= 1 && n_expiries >= 1 && n_gammas >= 1 && n_gammas <= SVMC_TILTED_MAX_GAMMAS;
}
static bool js_sizes_ok(size_t n_path, int n_expiries, int n_sets)
{
    return n_path >= 1 && n_expiries >= 1 && n_sets >= 1 && n_sets <= SVMC_JUMP_SETS_MAX;
}

}  // namespace svmc

using namespace svmc;

extern "C" {

int svmc_est_version(void) { return SVMC_EST_VERSION; }

int svmc_tilted_cond_greeks_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, int n_gammas, size_t *bytes)
{
    if (bytes == nullptr || !tcg_sizes_ok(n_path, n_expiries, n_gammas)) return SVMC_ERR_INVALID_ARGUMENT;
    TcgTable t;
    Layout w{nullptr};
    tcg_workspace(w, n_path, n_expiries, total_strikes, quote_groups_bound(n_expiries, total_strikes, TCG_KT), n_gammas, t);
    *bytes = w.bytes();
    return SVMC_OK;
}

int svmc_tilted_cond_greeks_chain(const double *const *mu_snapshots_host, const double *const *cv_snapshots_host, size_t n_path,
                                  const double *forwards_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                  const size_t *strike_offsets_host, const double *gammas_host, int n_gammas, int recenter,
                                  double *greeks_host, double *stats_host, void *workspace, size_t workspace_bytes,
                                  svmc_stream_t stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // everything is checked before anything is launched
    if (!mu_snapshots_host || !cv_snapshots_host || !forwards_host || !strikes_host || !types_host || !strike_offsets_host ||
        !gammas_host || !greeks_host || !stats_host || !workspace)
        return SVMC_ERR_INVALID_ARGUMENT;
    if (!tcg_sizes_ok(n_path, n_expiries, n_gammas) || !tc_all_finite(gammas_host, n_gammas)) return SVMC_ERR_INVALID_ARGUMENT;
    const int m = n_expiries, NG = n_gammas;
    const int rc = tc_check_quotes(m, strike_offsets_host, mu_snapshots_host, cv_snapshots_host, forwards_host, strikes_host, nullptr,
                                   types_host);
    if (rc != SVMC_OK) return rc;
    const size_t K = strike_offsets_host[m];
    const int G = quote_groups(m, strike_offsets_host, TCG_KT, true);
    if (G > TC_MAX_GROUPS) return SVMC_ERR_INVALID_ARGUMENT;
    TcgTable t;
    Layout w{static_cast<unsigned char *>(workspace)};
    std::vector<unsigned char> image(tcg_workspace(w, n_path, m, K, G, NG, t));
    if (workspace_bytes < w.bytes()) return SVMC_ERR_WORKSPACE;

    Layout h{image.data()};
    const TcImageOf<double> im = tc_image<double>(h, m, K, G, NG);
    tc_fill_image(im, m, strike_offsets_host, TCG_KT, mu_snapshots_host, cv_snapshots_host, forwards_host, strikes_host, types_host,
                  [&](int i, int k) {
                      const double sgn = (types_host[k] == SVMC_PUT) ? -1.0 : 1.0;
                      return (sgn * (forwards_host[i] - strikes_host[k]) > 0.0) ? sgn : 0.0;
                  });
    for (int z = 0; z < NG; ++z) im.zs[z] = gammas_host[z];
    std::vector<double> out(tcg_out_doubles(m, K, NG));
    const int run = tc_run(workspace, image, t.out, out, stream, [&]() {
        hipLaunchKernelGGL(tilted_cond_greeks_forward_kernel, dim3(t.rows, m), dim3(BLOCK), 0, stream, t, n_path);
        SVMC_TC_TRY(hipGetLastError());
        hipLaunchKernelGGL(tilted_cond_greeks_forward_finish_kernel, dim3(m), dim3(BLOCK), 0, stream, t, recenter ? 1 : 0);
        SVMC_TC_TRY(hipGetLastError());
        hipLaunchKernelGGL(tilted_cond_greeks_kernel<TCG_KT>, dim3(t.rows, G, NG), dim3(BLOCK), 0, stream, t, n_path, recenter ? 1 : 0);
        SVMC_TC_TRY(hipGetLastError());
        hipLaunchKernelGGL(tilted_cond_greeks_finish_kernel, dim3(static_cast<unsigned>(K) + m, NG), dim3(BLOCK), 0, stream, t, n_path);
        SVMC_TC_TRY(hipGetLastError());
        return SVMC_OK;
    });
    if (run != SVMC_OK) return run;
    const double *block = tc_split(out.data(), greeks_host, static_cast<size_t>(NG) * SVMC_TCG_ROWS * K);
    tc_split(block, stats_host, static_cast<size_t>(NG) * m * SVMC_TCG_STATS_DOUBLES);
    return SVMC_OK;
}

int svmc_cond_density_workspace_bytes(size_t n_path, int n_expiries, size_t total_points, int n_gammas, size_t *bytes)
{
    if (bytes == nullptr || !tcg_sizes_ok(n_path, n_expiries, n_gammas)) return SVMC_ERR_INVALID_ARGUMENT;
    CdTable t;
    Layout w{nullptr};
    cd_workspace(w, n_path, n_expiries, total_points, quote_groups_bound(n_expiries, total_points, CD_XT), n_gammas, t);
    *bytes = w.bytes();
    return SVMC_OK;
}

int svmc_cond_density_chain(const double *const *mu_snapshots_host, const double *const *cv_snapshots_host, size_t n_path, int n_expiries,
                            const double *points_host, const size_t *point_offsets_host, const double *gammas_host, int n_gammas,
                            double *pdf_host, double *stderr_host, double *stats_host, void *workspace, size_t workspace_bytes,
                            svmc_stream_t stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // everything is checked before anything is launched
    if (!mu_snapshots_host || !cv_snapshots_host || !points_host || !point_offsets_host || !gammas_host || !pdf_host || !stderr_host ||
        !stats_host || !workspace)
        return SVMC_ERR_INVALID_ARGUMENT;
    if (!tcg_sizes_ok(n_path, n_expiries, n_gammas) || !tc_all_finite(gammas_host, n_gammas)) return SVMC_ERR_INVALID_ARGUMENT;
    const int m = n_expiries, NG = n_gammas;
    const int rc = tc_check_quotes(m, point_offsets_host, mu_snapshots_host, cv_snapshots_host, nullptr, points_host, nullptr, nullptr);
    if (rc != SVMC_OK) return rc;
    const size_t P = point_offsets_host[m];
    const int G = quote_groups(m, point_offsets_host, CD_XT, false);
    if (G > TC_MAX_GROUPS || m > TC_MAX_GROUPS) return SVMC_ERR_INVALID_ARGUMENT;
    CdTable t;
    Layout w{static_cast<unsigned char *>(workspace)};
    std::vector<unsigned char> image(cd_workspace(w, n_path, m, P, G, NG, t));
    if (workspace_bytes < w.bytes()) return SVMC_ERR_WORKSPACE;

    Layout h{image.data()};
    const CdImage im = cd_image(h, m, P, G, NG);
    quote_image(
        m, point_offsets_host, [&](int i, int p0, int p1) { im.expiries[i] = CdExpiry{mu_snapshots_host[i], cv_snapshots_host[i], p0, p1}; },
        [&](int, int p) { im.points[p] = points_host[p]; });
    quote_groups(m, point_offsets_host, CD_XT, false, im.groups);
    for (int z = 0; z < NG; ++z) im.gammas[z] = gammas_host[z];
    std::vector<double> out(cd_out_doubles(m, P, NG));
    const int run = tc_run(workspace, image, t.out, out, stream, [&]() {
        hipLaunchKernelGGL(cond_density_weight_kernel, dim3(t.rows, m, NG), dim3(BLOCK), 0, stream, t, n_path);
        SVMC_TC_TRY(hipGetLastError());
        if (G > 0) {
            if (NG <= CD_GT)
                hipLaunchKernelGGL((cond_density_kernel<CD_XT, CD_GT>), dim3(t.rows, G, 1), dim3(BLOCK), 0, stream, t, n_path);
            else
                hipLaunchKernelGGL((cond_density_kernel<CD_XT, CD_GT_WIDE>), dim3(t.rows, G, (NG + CD_GT_WIDE - 1) / CD_GT_WIDE), dim3(BLOCK), 0,
                                   stream, t, n_path);
            SVMC_TC_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(cond_density_finish_kernel, dim3(static_cast<unsigned>(P) + m, NG), dim3(BLOCK), 0, stream, t, n_path);
        SVMC_TC_TRY(hipGetLastError());
        return SVMC_OK;
    });
    if (run != SVMC_OK) return run;
    const size_t GP = static_cast<size_t>(NG) * P;
    const double *block = tc_split(tc_split(out.data(), pdf_host, GP), stderr_host, GP);
    tc_split(block, stats_host, static_cast<size_t>(NG) * m * SVMC_CD_STATS_DOUBLES);
    return SVMC_OK;
}

int svmc_jump_sets_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, int n_sets, size_t *bytes)
{
    if (bytes == nullptr || !js_sizes_ok(n_path, n_expiries, n_sets)) return SVMC_ERR_INVALID_ARGUMENT;
    JsTable t;
    Layout w{nullptr};
    js_workspace(w, n_path, n_expiries, total_strikes, quote_groups_bound(n_expiries, total_strikes, JS_KT), n_sets, t);
    *bytes = w.bytes();
    return SVMC_OK;
}

int svmc_jump_sets_payoff_chain(const double *const *a_snapshots_host, size_t n_path, const double *forwards_host, int n_expiries,
                                const double *strikes_host, const int8_t *types_host, const double *shifts_host,
                                const size_t *strike_offsets_host, const double *variances_host, const double *gammas_host, int n_sets,
                                int recenter, double *prices_host, double *stderrs_host, double *stats_host, double *corr_host,
                                void *workspace, size_t workspace_bytes, svmc_stream_t stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // everything is checked before anything is launched
    if (!a_snapshots_host || !forwards_host || !strikes_host || !types_host || !shifts_host || !strike_offsets_host || !variances_host ||
        !gammas_host || !prices_host || !stderrs_host || !stats_host || !corr_host || !workspace)
        return SVMC_ERR_INVALID_ARGUMENT;
    if (!js_sizes_ok(n_path, n_expiries, n_sets) || !tc_all_finite(gammas_host, n_sets)) return SVMC_ERR_INVALID_ARGUMENT;
    const int m = n_expiries, Q = n_sets;
    for (int j = 0; j < Q * m; ++j)
        if (!std::isfinite(variances_host[j]) || !(variances_host[j] >= 0.0)) return SVMC_ERR_INVALID_ARGUMENT;
    const int rc = tc_check_quotes(m, strike_offsets_host, a_snapshots_host, nullptr, forwards_host, strikes_host, shifts_host, types_host);
    if (rc != SVMC_OK) return rc;
    const size_t K = strike_offsets_host[m];
    const int G = quote_groups(m, strike_offsets_host, JS_KT, true);
    if (G > TC_MAX_GROUPS) return SVMC_ERR_INVALID_ARGUMENT;
    JsTable t;
    Layout w{static_cast<unsigned char *>(workspace)};
    std::vector<unsigned char> image(js_workspace(w, n_path, m, K, G, Q, t));
    if (workspace_bytes < w.bytes()) return SVMC_ERR_WORKSPACE;

    Layout h{image.data()};
    const TcImageOf<JsSet> im = tc_image<JsSet>(h, m, K, G, static_cast<size_t>(Q) * m);
    tc_fill_image(im, m, strike_offsets_host, JS_KT, a_snapshots_host, nullptr, forwards_host, strikes_host, types_host,
                  [&](int, int k) { return shifts_host[k]; });
    for (int q = 0; q < Q; ++q)
        for (int i = 0; i < m; ++i) {
            // the constants of a (set, expiry), each rounded once, from the set's own numbers alone
            const double g = gammas_host[q], v = variances_host[static_cast<size_t>(q) * m + i], gv = g * v, sd = std::sqrt(v);
            im.zs[static_cast<size_t>(q) * m + i] = JsSet{g,  std::exp(0.5 * ((g * (g - 1.0)) * v)), v, sd, 1.0 / sd,
                                                          forwards_host[i] * std::exp(gv), std::log(forwards_host[i]) + gv, gv};
        }
    std::vector<double> out(js_out_doubles(m, K, Q));
    const int run = tc_run(workspace, image, t.out, out, stream, [&]() {
        hipLaunchKernelGGL(jump_sets_forward_kernel, dim3(t.rows, m), dim3(BLOCK), 0, stream, t, n_path);
        SVMC_TC_TRY(hipGetLastError());
        hipLaunchKernelGGL(jump_sets_forward_finish_kernel, dim3(m), dim3(BLOCK), 0, stream, t, recenter ? 1 : 0);
        SVMC_TC_TRY(hipGetLastError());
        hipLaunchKernelGGL(jump_sets_payoff_kernel<JS_KT>, dim3(t.rows, G, Q), dim3(BLOCK), 0, stream, t, n_path);
        SVMC_TC_TRY(hipGetLastError());
        hipLaunchKernelGGL(jump_sets_finish_kernel, dim3(static_cast<unsigned>(K) + m, Q), dim3(BLOCK), 0, stream, t, n_path);
        SVMC_TC_TRY(hipGetLastError());
        return SVMC_OK;
    });
    if (run != SVMC_OK) return run;
    const size_t QK = static_cast<size_t>(Q) * K;
    const double *block = tc_split(tc_split(out.data(), prices_host, QK), stderrs_host, QK);
    block = tc_split(block, stats_host, static_cast<size_t>(Q) * m * SVMC_TILTED_STATS_DOUBLES);
    tc_split(block, corr_host, m);
    return SVMC_OK;
}

}  // extern "C"
