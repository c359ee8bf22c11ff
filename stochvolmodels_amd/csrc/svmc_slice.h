// svmc_slice.h -- the slice epilogue every on-device-RNG generator shares (svmc_kernels.hip, svmc_heston.hip, svmc_rough.hip,
// svmc_hawkes.hip): the terminal snapshot and the per-wave spot partials the chain payoff tail (payoff_group_kernel / chain_finish_kernel) reads.
#pragma once
#include <hip/hip_runtime.h>

#include "svmc_math.h"

namespace svmc {

// the sum over a wave's 64 lanes in a fixed shuffle tree (lane 0 holds it): the deterministic first level of every reduction
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Optional slice epilogue fused into the stepping kernels: the terminal x (and qvar) is also written to the
// per-expiry snapshot the payoff pass reads, and [sum F*exp(x), count] (utils/mc_payoffs.py:61-62) goes out as one row PER
// WAVE -- partials[column][wave], wave = global thread index / 64 -- which reduce_columns_kernel adds up in row order: one
// launch and one pass over x less per expiry.  Rows per wave, not per block: the sum's order of additions is then the same
// whatever block size a kernel runs (the one-slice generators run 512-thread blocks, the whole-chain kernel 1024, the
// streamed ones 256, and their results must agree to the bit), and the epilogue needs no LDS and no barrier.
struct SliceOut {
    double *x_snap;     // nullable
    double *q_snap;     // nullable
    double *partials;   // nullable: this slice's two COLUMNS, [2][rows] -- column-major, so that the reduction reads them coalesced
    double forward;
    size_t rows = 0;    // column stride of `partials`: wave_rows(n) of the launch
};

// the outputs of row `row` of a whole-chain launch of n paths: snapshots [rows][n], one column pair of per-wave partials per row
__device__ __forceinline__ SliceOut slice_out_row(double *x_snap, double *q_snap, double *partials, size_t row, size_t n, double forward)
{
    const size_t waves = (n + 63) >> 6;
    return {x_snap + row * n, q_snap ? q_snap + row * n : nullptr, partials + 2 * row * waves, forward, waves};
}

// Start state of a generator launch: read from x / vol / qvar (uniform = 0), or the same three constants for every path --
// what a chain pricing starts from (x0 = 0, sigma0 | v0, qvar0 = 0: pricers/logsv_pricer.py:823-826, heston_pricer.py:303-305).
// The svmc_*_rng_from entry points use it: no fill launch (11 us + the write-back of its 24 bytes per path at the kernel
// boundary) and no 24-byte read per path ahead of the stepping.
struct StateInit {
    int uniform = 0;
    double x0 = 0.0, vol0 = 0.0, qvar0 = 0.0;
};

__device__ __forceinline__ void slice_epilogue(const SliceOut &so, size_t p, bool active, double xv, double q)
{
    if (active) {
        if (so.x_snap != nullptr) so.x_snap[p] = xv;
        if (so.q_snap != nullptr) so.q_snap[p] = q;
    }
    if (so.partials != nullptr) {
        const double sp = so.forward * exp_full(xv);       // full-range exp: x = +-inf must give inf / 0   :61
        const bool ok = active && (sp == sp);                                                   // nanmean :62
        const double v0 = wave_sum(ok ? sp : 0.0), v1 = wave_sum(ok ? 1.0 : 0.0);
        if ((threadIdx.x & 63u) == 0u && (p >> 6) < so.rows) {        // a launch's last block may hold waves past the last path
            so.partials[p >> 6] = v0;
            so.partials[so.rows + (p >> 6)] = v1;
        }
    }
}

}  // namespace svmc
