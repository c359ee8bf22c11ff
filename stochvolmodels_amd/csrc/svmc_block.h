// svmc_block.h -- what the kernels and launchers of every Monte Carlo unit share (svmc_kernels.hip, svmc_heston.hip,
// svmc_rough.hip): the block and grid constants with their host helpers, the clock probe's stamp, the deterministic block and
// column sums and the streamed-randoms time loop.  Device code is __device__ __forceinline__ or constexpr; the host helpers are
// static inline.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "svmc_slice.h"

namespace svmc {

constexpr int BLOCK = 256;             // 4 waves of 64 lanes
#ifndef SVMC_MAX_REDUCE_GRID
#define SVMC_MAX_REDUCE_GRID 1024
#endif
constexpr int MAX_REDUCE_GRID = SVMC_MAX_REDUCE_GRID;  // 256 CUs x 4 blocks: cap for grid-stride reductions

// block size of the on-device-RNG generators: a block stages the draw's tables in LDS once for all of its waves
#ifndef SVMC_RNG_BLOCK
#define SVMC_RNG_BLOCK 512
#endif
constexpr int RNG_BLOCK = SVMC_RNG_BLOCK;
static constexpr int rng_block() { return RNG_BLOCK; }
static inline unsigned rng_grid(size_t n) { return static_cast<unsigned>((n + rng_block() - 1) / rng_block()); }

static inline unsigned grid_for(size_t n) { return static_cast<unsigned>((n + BLOCK - 1) / BLOCK); }

// block size of the few-waves form of the on-device-RNG generators (few_waves_launch(), svmc_kernels.hip)
constexpr int FEW_BLOCK = 256;
static inline unsigned lat_grid(size_t n, int block = FEW_BLOCK) { return static_cast<unsigned>((n + block - 1) / block); }
// the Philox counter word of a call: the call id above the 8 bits of the stream tag (svmc_rng.h)
static inline uint32_t make_c3(uint32_t call_id) { return (call_id << 8); }

// expiries per whole-chain launch (= MAX_FUSED_SLICES of svmc_internal.h)
constexpr int MAX_CHAIN_SLICES = 16;

// In-kernel clock probe of the on-device-RNG LogSV generators (svmc_clock_probe_arm / _read; bench.py
// roofline.clock_mhz_in_kernel): measurement plumbing, OFF unless the calling host thread armed it.  The stepping kernels
// take a nullable `probe` argument -- null in every product launch: one scalar test, nothing else.  When a thread has armed
// the probe, ITS launches pass that thread's own 8-word device buffer and thread 0 of the launch's FIRST and LAST block stamp
// s_memtime (tick = shader cycle) and s_memrealtime (100 MHz, chip-wide) at kernel entry and again after the time loop:
// (t_exit - t_entry) / (r_exit - r_entry) x 100 MHz is the shader clock that wave saw while it stepped -- measured in the
// timed launch itself, where the SMU's sysfs sensor (absent on some boxes of the pool) lags and averages.  No global: two
// engines on two streams (tests/test_gpu_parity.py::test_two_engines_on_their_own_streams) never share stamps, and a
// thread that did not arm the probe never writes any (round 4 kept one __device__ array every launch of three kernels
// wrote: a race between engines and bench-only code on the hot path).
// Layout: [which = 0 first block | 1 last block][t_entry, r_entry, t_exit, r_exit]; the latest armed launch wins.
// In the many-job launches (grid = path blocks x jobs) a block stamps by its blockIdx.x alone: with J jobs each slot has J writers,
// on different XCDs whose cycle counters are not comparable, and a slot's entry and exit may come from two of them (seen with two
// jobs: t_exit < t_entry).  The clock read off a many-job launch is meaningful for ONE job only.
__device__ __forceinline__ void clock_probe_stamp(uint64_t *probe, int at_exit)
{
    if (probe == nullptr) return;                                                    // wave-uniform (a kernel argument)
    const bool first = blockIdx.x == 0u, last = blockIdx.x == gridDim.x - 1u;        // wave-uniform
    if (first || last) {
        const uint64_t t = __builtin_readcyclecounter(), r = wall_clock64();
        if (threadIdx.x == 0u) {
            uint64_t *o = probe + (first ? 0 : 4) + 2 * at_exit;
            o[0] = t;
            o[1] = r;
        }
    }
}

// Least-progress-first wave priority (the LogSV stepping loops of svmc_kernels.hip and svmc_cmc.hip).  The SIMD arbiter picks by
// priority, then age; with equal priorities the
// oldest wave always wins, younger waves starve and each launch ends in a long ramp-down where lone, late waves run
// at ~60 % of the saturated rate (tools/ubench/tail_probe.hip).  Dropping a wave's own priority as it progresses
// through the time loop (3 -> 0 at the quarter points) lets waves that are behind catch up: residency stays at 8
// waves per SIMD and the ramp-down shrinks from ~30 % to ~10 % of the launch.
__device__ __forceinline__ void progress_priority(int stage)
{
    switch (stage) {
    case 0: __builtin_amdgcn_s_setprio(3); break;
    case 1: __builtin_amdgcn_s_setprio(2); break;
    case 2: __builtin_amdgcn_s_setprio(1); break;
    default: __builtin_amdgcn_s_setprio(0); break;
    }
}

// where a launch stands on that ladder: wave-uniform counters, carried from slice to slice of a chain
struct LogsvProgress {
    int quarter;                       // a quarter of the launch's steps, rounded up
    int stage = 0, next_stage_t = 0;
};

// ---------------------------------------------------------------------------------------------------
// Deterministic block reductions: wave shuffles in a fixed tree, one LDS exchange, ONE barrier for any number of
// values (the first version paid two barriers per value: 96 per payoff block).
// ---------------------------------------------------------------------------------------------------
// One halving level of the multi-value butterfly: lanes with (lane & MASK) set keep the upper half of v[0..2H),
// the others the lower half, and add the partner lane's copy of the half they keep.
template <int H, int MASK>
__device__ __forceinline__ void butterfly_halve(const double *v, double *w, int lane)
{
    const bool hi = (lane & MASK) != 0;
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const double mine = hi ? v[H + j] : v[j];
        const double other = hi ? v[j] : v[H + j];
        w[j] = mine + __shfl_xor(other, MASK, 64);
    }
}

// values a block sum works on: NV rounded up to a multiple of 8 from 8 on (the halving tree below wants it; zeros fill up)
constexpr int block_sum_padded(int nv) { return nv >= 8 ? (nv + 7) / 8 * 8 : nv; }

// every thread of the block calls; thread j < n_out ends up with the block total of v[j] and hands it to store(j, total)
template <int NV, class Store>
__device__ __forceinline__ void block_sum_apply(double (&v)[NV], double *lds /* [4 * block_sum_padded(NV)] */, int n_out,
                                                Store &&store)
{
    constexpr int NP = block_sum_padded(NV);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    if constexpr (NP % 8 == 0) {
        // NP values over 64 lanes in NP/2 + NP/4 + NP/8 + 3*NP/8 shuffles instead of 6*NP: three halving levels
        // (xor 32, 16, 8) leave every lane with NP/8 partial sums of the index block its bits 5..3 select, three
        // plain levels (xor 4, 2, 1) finish them.  Fixed tree, hence deterministic.
        double vp[NP], a[NP / 2], b[NP / 4], c[NP / 8];
#pragma unroll
        for (int j = 0; j < NP; ++j) vp[j] = (j < NV) ? v[j] : 0.0;
        butterfly_halve<NP / 2, 32>(vp, a, lane);
        butterfly_halve<NP / 4, 16>(a, b, lane);
        butterfly_halve<NP / 8, 8>(b, c, lane);
#pragma unroll
        for (int j = 0; j < NP / 8; ++j) {
            c[j] += __shfl_xor(c[j], 4, 64);
            c[j] += __shfl_xor(c[j], 2, 64);
            c[j] += __shfl_xor(c[j], 1, 64);
        }
        if ((lane & 7) == 0) {
            const int off = ((lane & 32) ? NP / 2 : 0) + ((lane & 16) ? NP / 4 : 0) + ((lane & 8) ? NP / 8 : 0);
#pragma unroll
            for (int j = 0; j < NP / 8; ++j) lds[wave * NP + off + j] = c[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = wave_sum(v[j]);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < NV; ++j) lds[wave * NP + j] = v[j];
        }
    }
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < n_out) {
        const int j = threadIdx.x;
        double t = lds[j];
        for (int w = 1; w < n_waves; ++w) t += lds[w * NP + j];      // fixed order: wave 0, 1, 2, 3
        store(j, t);
    }
}

// thread j < n_out writes the block total of v[j] to out[j]
template <int NV>
__device__ __forceinline__ void block_sum_store(double (&v)[NV], double *lds /* [4 * block_sum_padded(NV)] */, double *out, int n_out)
{
    block_sum_apply<NV>(v, lds, n_out, [&](int j, double t) { out[j] = t; });
}

// The sum of one column, the ONE order of additions every column reduction of the library uses (so that a sum does not depend on
// which kernel formed it).  256 (virtual) threads: thread t adds rows t, t + 256, ... into four accumulators -- sixteen rows at a
// time into a[k mod 4] while sixteen remain, then four at a time into a[0..3], then the last three or fewer into a[0] --, forms
// (a0 + a1) + (a2 + a3), each wave adds its 64 lanes in a fixed shuffle tree and the four wave totals are added in wave order.
// A row is one 8-byte read at a stride of ld -- latency, not bandwidth: what a reduction costs is how many DEPENDENT round trips
// it makes, so the loads are batched (sixteen per trip in the long loop; a column of up to NR x 256 rows has ALL its loads in
// flight before the first addition -- round 6: the spot columns of a 10^5-path launch were 1 + 3 dependent round trips, 4.7 us of
// a 5 us kernel) and the additions keep the order above: the same bits whichever route.
template <int NR>
__device__ __forceinline__ void column_rows_load(const double *__restrict__ partials, unsigned r, unsigned n_rows, size_t ld, double (&t)[NR])
{
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const unsigned rk = r + static_cast<unsigned>(k) * BLOCK;
        t[k] = (rk < n_rows) ? partials[static_cast<size_t>(rk) * ld] : 0.0;
    }
}
// ... for n_rows <= NR x 256 (NR = 4 or 8: the sixteen-row loop never runs): the additions of the loops, on the preloaded rows
template <int NR>
__device__ __forceinline__ double column_rows_add(const double (&t)[NR], unsigned r, unsigned n_rows)
{
    static_assert(NR == 4 || NR == 8, "one or two trips of the four-row loop");
    const unsigned cnt = (n_rows > r) ? (n_rows - r + BLOCK - 1) / BLOCK : 0u;        // rows of this thread
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    unsigned k = 0;
    if (cnt >= 4u) {
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] += t[u];
        k = 4;
        if constexpr (NR == 8) {
            if (cnt >= 8u) {
#pragma unroll
                for (int u = 0; u < 4; ++u) a[u] += t[4 + u];
                k = 8;
            }
        }
    }
#pragma unroll
    for (int kk = 0; kk < NR; ++kk)
        if (static_cast<unsigned>(kk) >= k && static_cast<unsigned>(kk) < cnt) a[0] += t[kk];
    return (a[0] + a[1]) + (a[2] + a[3]);
}
// any n_rows: the loops themselves
__device__ __forceinline__ double column_rows_sum(const double *__restrict__ partials, unsigned r, unsigned n_rows, size_t ld)
{
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (; r + 15 * BLOCK < n_rows; r += 16 * BLOCK) {
        double t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) t[u] = partials[static_cast<size_t>(r + u * BLOCK) * ld];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] += t[4 * k + u];
        }
    }
    for (; r + 3 * BLOCK < n_rows; r += 4 * BLOCK) {
        double t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = partials[static_cast<size_t>(r + u * BLOCK) * ld];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] += t[u];
    }
    for (; r < n_rows; r += BLOCK) a[0] += partials[static_cast<size_t>(r) * ld];
    return (a[0] + a[1]) + (a[2] + a[3]);
}

// by a 256-thread block: every thread calls; thread 0 returns the total (the others a partial)
__device__ __forceinline__ double block_column_sum(const double *__restrict__ partials, unsigned n_rows, size_t ld, double *lds /* [4] */)
{
    double v[1];
    if (n_rows <= 8u * BLOCK) {                             // (block-uniform)
        double t[8];
        column_rows_load<8>(partials, threadIdx.x, n_rows, ld, t);
        v[0] = column_rows_add<8>(t, threadIdx.x, n_rows);
    } else {
        v[0] = column_rows_sum(partials, threadIdx.x, n_rows, ld);
    }
    double total = 0.0;
    block_sum_apply<1>(v, lds, 1, [&](int, double t) { total = t; });
    return total;
}

// two columns by one block with the loads of BOTH in flight together (the payoff kernel's spot sums: [sum F exp(x), count])
__device__ __forceinline__ void block_column_sum2(const double *__restrict__ p0, const double *__restrict__ p1, unsigned n_rows, double *lds,
                                                  double &s0, double &s1)
{
    double v0[1], v1[1];
    if (n_rows <= 8u * BLOCK) {
        double t0[8], t1[8];
        column_rows_load<8>(p0, threadIdx.x, n_rows, 1, t0);
        column_rows_load<8>(p1, threadIdx.x, n_rows, 1, t1);
        v0[0] = column_rows_add<8>(t0, threadIdx.x, n_rows);
        v1[0] = column_rows_add<8>(t1, threadIdx.x, n_rows);
    } else {
        v0[0] = column_rows_sum(p0, threadIdx.x, n_rows, 1);
        v1[0] = column_rows_sum(p1, threadIdx.x, n_rows, 1);
    }
    s0 = s1 = 0.0;
    block_sum_apply<1>(v0, lds, 1, [&](int, double t) { s0 = t; });
    __syncthreads();                                        // thread 0 has read the wave totals: lds may be written again
    block_sum_apply<1>(v1, lds, 1, [&](int, double t) { s1 = t; });
}

// Streamed-randoms time loop: HBM-bound (8 B per supplied random per path-step).  Software-pipelined by hand:
// the NARR*U loads of the next U steps are issued before the current U steps are computed, so every wave keeps
// NARR*U x 512 B in flight (hipcc does not unroll a loop that contains inline asm, and one load per array in
// flight leaves the memory system latency-bound: 5.3 -> 5.7 TB/s for LogSV at U = 4; U = 8, 16 give no more).
constexpr int STREAM_U = 4;

template <int NARR, int U = STREAM_U, class Step>
__device__ __forceinline__ void streamed_time_loop(const double *const (&w)[NARR], size_t ldw, int nb_steps,
                                                   Step &&step)
{
    double a[NARR][U], b[NARR][U];
    int t = 0;
    if (nb_steps >= U) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int k = 0; k < NARR; ++k) a[k][u] = w[k][static_cast<size_t>(u) * ldw];
        for (; t + 2 * U <= nb_steps; t += U) {
#pragma unroll
            for (int u = 0; u < U; ++u)                         // prefetch steps t+U .. t+2U-1
#pragma unroll
                for (int k = 0; k < NARR; ++k) b[k][u] = w[k][static_cast<size_t>(t + U + u) * ldw];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                double v[NARR];
#pragma unroll
                for (int k = 0; k < NARR; ++k) v[k] = a[k][u];
                step(v);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int k = 0; k < NARR; ++k) a[k][u] = b[k][u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double v[NARR];
#pragma unroll
            for (int k = 0; k < NARR; ++k) v[k] = a[k][u];
            step(v);
        }
        t += U;
    }
    for (; t < nb_steps; ++t) {
        double v[NARR];
#pragma unroll
        for (int k = 0; k < NARR; ++k) v[k] = w[k][static_cast<size_t>(t) * ldw];
        step(v);
    }
}

}  // namespace svmc
