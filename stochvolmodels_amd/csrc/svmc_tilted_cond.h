// svmc_tilted_cond.h -- the statements the conditional estimators under the exponential risk-premia kernel share: the payoff tail of
// libsvmc_ext.so (svmc_ext.hip) and the Greeks tail of libsvmc_est.so (svmc_est.hip, row f18).  Row f11's keep
// rule and Black-76 price restated (svmc_cmc.hip: cmc_keep, cmc_black), a path's weight and shifted forward, and the bodies of the
// forward pass's two kernels, written once so that corr, K' = K + corr, the weight and the keep decisions are the same bits in
// both libraries.  Device code is __device__ __forceinline__; no kernel is defined here: each unit names and launches its own.
#pragma once
#include <hip/hip_runtime.h>

#include "svmc_black.h"
#include "svmc_block.h"
#include "svmc_math.h"
#include "svmc_quotes.h"

namespace svmc {

static_assert(QUOTE_BLOCK == BLOCK, "svmc_quotes.h sizes the partial rows for blocks of BLOCK paths");

struct TcExpiry {
    const double *mu, *cv;
    double forward, ln_forward;
    int k0, k1;                        // its strikes [k0, k1)
};

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
// Table: a unit's device table with expiries, strikes, kp, ln_kp, fwd [m][4], fwd_partials [rows][m][3], m and rows.
// grid (path blocks, expiries); lds [4 * 3]
template <class Table>
__device__ __forceinline__ void tc_forward_body(const Table &t, size_t n, double *lds)
{
    const TcExpiry ex = t.expiries[blockIdx.y];
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    double v[3] = {0.0, 0.0, 0.0};
    for (size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x; i < n; i += stride) {
        double h, e;
        if (tc_keep_cmc(ex.mu[i], ex.cv[i], h, e)) {
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

}  // namespace svmc
