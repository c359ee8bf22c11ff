// svmc_kernels.hip -- gfx950 kernels and compute entry points of the C ABI (include/svmc.h).
//
// Mapping: one wavefront lane per Monte Carlo path.  A path's state (x, L = ln sigma, sigma, I) lives in
// VGPRs for the whole slice; HBM is touched once per slice per path (24 B read + 24 B write) in the
// on-device-RNG kernels, and 16 B per path-step (the two supplied normals, coalesced 512 B per wave
// per load) in the streamed-randoms kernels.  No MFMA: the work is elementwise fp64 VALU +
// transcendentals (DESIGN.md "Rooflines").
//
// The Heston and the rough-LogSV families are units of their own (svmc_heston.hip, svmc_rough.hip); what they share with this
// file is in svmc_block.h and svmc_jobs.h, and the host functions they call here are declared in svmc_internal.h.
#include "svmc_internal.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>
#include "svmc_black.h"
#include "svmc_block.h"
#include "svmc_jobs.h"
#include "svmc_models.h"
#include "svmc_rng.h"
#include "svmc_slice.h"

namespace svmc {

#ifndef SVMC_RNG_SGPRS
#define SVMC_RNG_SGPRS 72              // SGPR budget of the LogSV stepping kernels (tools/ubench/ab_kernels.py sweeps it)
#endif

// the calling host thread's armed probe buffer (device memory of the device that was current at svmc_clock_probe_arm), or null
uint64_t *&armed_probe()
{
    thread_local uint64_t *p = nullptr;
    return p;
}

// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void fill_state_kernel(double *__restrict__ x, double *__restrict__ vol,
                                                           double *__restrict__ qvar, size_t n, double x0,
                                                           double vol0, double qvar0)
{
    const size_t p = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x;
    if (p < n) {
        x[p] = x0;
        vol[p] = vol0;
        qvar[p] = qvar0;
    }
}

__global__ __launch_bounds__(RNG_BLOCK) void fill_normals_kernel(double *__restrict__ W0, double *__restrict__ W1,
                                                             size_t ldw, size_t n, int nb_steps, uint64_t seed,
                                                             uint32_t c3, uint64_t path_offset,
                                                             uint32_t step_offset)
{
    __shared__ RngTablesLds s_tab;
    const RngTables tab = stage_rng_tables(s_tab);
    const size_t p = static_cast<size_t>(blockIdx.x) * RNG_BLOCK + threadIdx.x;
    if (p >= n) return;
    const PhiloxLane lane = philox_prepare(seed, c3, path_offset + p);
    size_t row = p;
    rng_time_loop(lane, step_offset, nb_steps, tab, [&](double w0, double w1) {
        W0[row] = w0;
        W1[row] = w1;
        row += ldw;
    });
}

__global__ __launch_bounds__(BLOCK) void fill_uniforms_kernel(double *__restrict__ U, size_t ldw, size_t n,
                                                              int nb_steps, uint64_t seed, uint32_t c3,
                                                              uint64_t path_offset, uint32_t step_offset)
{
    const size_t p = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint64_t gp = path_offset + p;
    for (int t = 0; t < nb_steps; ++t)
        U[static_cast<size_t>(t) * ldw + p] = draw_uniform(seed, c3, gp, step_offset + static_cast<uint32_t>(t));
}

// ---------------------------------------------------------------------------------------------------
// LogSV generators (pricers/logsv_pricer.py:950-1047)
// ---------------------------------------------------------------------------------------------------
// (the least-progress-first wave priority of the time loops, progress_priority / LogsvProgress: svmc_block.h)
// what a slice's time loop leaves for logsv_fold_acc
struct LogsvSliceSums {
    double xacc, acc, s2_start;
};

// ONE slice of a LogSV path in the full-launch form, the statements every full-launch generator runs (logsv_rng_kernel, the
// whole-chain kernels through logsv_chain_full_body): nb steps from step `step0` of the lane's stream on the volatility s, which
// it advances; `t0` is how many steps the launch ran before this slice (the priority ladder's clock).  It returns the
// accumulators instead of folding them: the whole-chain body keeps x and qvar in LDS while this runs.
__device__ __forceinline__ LogsvSliceSums logsv_slice_full(const LogsvFast c, double &s, const PhiloxLane &lane, uint32_t step0, int t0,
                                                           int nb, const RngTables &tab, const double *exp_table, LogsvProgress &prog)
{
    // the tail's leading coefficient stays in one register pair for the whole loop: left to the compiler, the second step of a trip
    // overwrites it and every trip pays a v_mov_b64 to bring it back
    double k0 = EXP2U_TAIL_K0;
    asm volatile("" : "+v"(k0));
    const auto exp_of = [&](double v) { return exp2u_tab(v, exp_table, k0); };  // L is carried in units of ln2/256
    double L = log_state(s) * LOG_UNITS_PER_NAT;                                                      // :1039
    double s2 = square_rn(s), acc = 0.0, xacc = 0.0;
    const double s2_start = s2;
    // one pair ahead, keys un-hoisted: the draw's reads land under the wave's own step (svmc_rng.h), the same bits as rng_time_loop
    rng_time_loop_pair_ahead<false>(
        lane, step0, nb, tab, [&](double z0, double z1) { logsv_step_acc(c, xacc, L, s, s2, acc, z0, z1, exp_of); },
        [&](int t) {
            if (t0 + t >= prog.next_stage_t) {             // wave-uniform
                progress_priority(prog.stage++);
                prog.next_stage_t += prog.quarter;
            }
        });
    return {xacc, acc, s2_start};
}

__global__ __launch_bounds__(RNG_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8), amdgpu_num_sgpr(SVMC_RNG_SGPRS))) void logsv_rng_kernel(double *__restrict__ x, double *__restrict__ sigma,
                                                          double *__restrict__ qvar, size_t n, int nb_steps,
                                                          LogsvFast c, uint64_t seed, uint32_t c3,
                                                          uint64_t path_offset, uint32_t step_offset, SliceOut so,
                                                          StateInit init, uint64_t *probe)
{
    __shared__ RngTablesLds s_tab;
    __shared__ double s_exp[256];
    const RngTables tab = stage_tables<RNG_BLOCK>(s_tab, s_exp);
    clock_probe_stamp(probe, 0);
    const size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool active = p < n;
    double xv = 0.0, s = 1.0, q = 0.0;
    if (active) {
        if (init.uniform) {                                // wave-uniform
            xv = init.x0;
            s = init.vol0;
            q = init.qvar0;
        } else {
            xv = x[p];
            s = sigma[p];
            q = qvar[p];
        }
        const PhiloxLane lane = philox_prepare(seed, c3, path_offset + p);
        LogsvProgress prog = {(nb_steps + 3) >> 2};
        const LogsvSliceSums a = logsv_slice_full(c, s, lane, step_offset, 0, nb_steps, tab, s_exp, prog);
        logsv_fold_acc(c, xv, q, a.xacc, a.acc, a.s2_start, square_rn(s));
        x[p] = xv;
        sigma[p] = s;
        qvar[p] = q;
    }
    clock_probe_stamp(probe, 1);
    slice_epilogue(so, p, active, xv, q);
}

// logsv_rng_kernel for a launch of a few waves per SIMD (few_waves_launch(): up to seven; the reference's default 10^5 paths are
// 1.5).  Statement for statement the kernel above -- the same bits -- but compiled for latency instead of residency: TB-thread
// blocks (256: every CU gets work, and four blocks' tables fit a CU's LDS), the register budget of WAVES waves per SIMD, and the
// time loop in form GEN_LOOP_PIPE (svmc_rng.h): the step in two halves around its exp-table read, the next pair's cubics, the
// next Philox call and the issue of the pair after that between them -- a wave overlaps its own LDS round trips with its own
// arithmetic, and the waves of a CU cannot fall into a common LDS phase.  The forms it was measured against:
// profiles/r06_mid_waves_sweep.json.
// the time loop of a LogSV generator: the pipelined form, the step in its two halves
template <int LOOP>
__device__ __forceinline__ void logsv_gen_time_loop(const PhiloxLane &lane, uint32_t step0, int nb, const RngTables &tab, const LogsvFast &c,
                                                    double &xacc, double &L, double &s, double &acc, const double *exp_table)
{
    static_assert(LOOP == GEN_LOOP_PIPE, "the LogSV few-waves generators run the pipelined loop");
    LogsvStepInFlight h;
    const Exp2uTailV k = exp2u_tail_consts();
    rng_time_loop_pipelined(
        lane, step0, nb, tab, [&](double z0, double z1) { logsv_step_acc_front(c, xacc, L, s, acc, z0, z1, exp_table, h); },
        [&]() { logsv_step_acc_mid(h, k); }, [&]() { logsv_step_acc_back(s, h); });
}

// ONE slice of a LogSV path in the few-waves form, the statements every few-waves generator runs (logsv_rng_lat_kernel, the
// whole-chain kernels through logsv_chain_lat_body): logsv_slice_full's arithmetic on the pipelined loop, folded into (xv, q)
template <int LOOP>
__device__ __forceinline__ void logsv_slice_lat(const LogsvFast c, double &xv, double &s, double &q, const PhiloxLane &lane, uint32_t step0,
                                                int nb, const RngTables &tab, const double *exp_table)
{
    double L = log_state(s) * LOG_UNITS_PER_NAT;                                                      // :1039
    double acc = 0.0, xacc = 0.0;
    const double s2_start = square_rn(s);
    logsv_gen_time_loop<LOOP>(lane, step0, nb, tab, c, xacc, L, s, acc, exp_table);
    logsv_fold_acc(c, xv, q, xacc, acc, s2_start, square_rn(s));
}

template <int LOOP, int WAVES, int TB>
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void logsv_rng_lat_kernel(
    double *__restrict__ x, double *__restrict__ sigma, double *__restrict__ qvar, size_t n, int nb_steps, LogsvFast c,
    uint64_t seed, uint32_t c3, uint64_t path_offset, uint32_t step_offset, SliceOut so, StateInit init, uint64_t *probe)
{
    __shared__ RngTablesLds s_tab;
    __shared__ double s_exp[256];
    const RngTables tab = stage_tables(s_tab, s_exp);
    clock_probe_stamp(probe, 0);
    const size_t p = static_cast<size_t>(blockIdx.x) * TB + threadIdx.x;
    const bool active = p < n;
    double xv = 0.0, s = 1.0, q = 0.0;
    if (active) {
        if (init.uniform) {
            xv = init.x0;
            s = init.vol0;
            q = init.qvar0;
        } else {
            xv = x[p];
            s = sigma[p];
            q = qvar[p];
        }
        const PhiloxLane lane = philox_prepare(seed, c3, path_offset + p);
        logsv_slice_lat<LOOP>(c, xv, s, q, lane, step_offset, nb_steps, tab, s_exp);
        x[p] = xv;
        sigma[p] = s;
        qvar[p] = q;
    }
    clock_probe_stamp(probe, 1);
    slice_epilogue(so, p, active, xv, q);
}

// Which form of a generator a launch runs is decided by how many waves per SIMD it puts on the device, not by a path constant:
//   up to lat_waves_per_simd() (7: 458752 paths on an MI355X, 256 CUs x 4 SIMDs)   the few-waves form: 256-thread blocks, the
//                                                                                  pipelined time loop, a 128-register budget
//   above                                                                          the full-launch kernels (eight waves per SIMD)
// Round 6 (profiles/r06_mid_waves_sweep.json; wall time of logsv_mc_chain_pricer, 4 x 13 chain x 364 steps, pipelined form /
// round 5's batched form / full-launch kernels): 2^16 paths 0.125 / 0.140 / 0.211 ms, 10^5 0.151 /
// 0.165 / 0.212, 2 x 10^5 0.221 / 0.264 / 0.219, 4 x 10^5 0.331 / 0.411 / 0.344, 2^19 0.371 / 0.459 / 0.362.  From two waves per
// SIMD on EVERY form runs at 250-275 cycles per wave-step -- C2's rate: the loop is bound by VALU issue and the LDS pipe together,
// not by latency -- and a launch takes as long as its fullest SIMD: 200 000 paths are 3.05 waves per SIMD on average but four on
// the fullest, so they cost what 262 144 cost.  What the pipelined form buys is the latency-bound end (one or two waves per SIMD,
// the reference's default 10^5 paths) and the block shape in between (256-thread blocks spread 6.1 waves per SIMD evenly where
// 1024-thread blocks leave a third of the CUs with eight).
// SVMC_FEW_WAVES_MAX_PATHS overrides the limit as a path count (0: the full-launch kernels always).
size_t device_simds()
{
    // per device of the calling thread's current context; the attribute query costs microseconds, so it is cached per device
    static std::atomic<size_t> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 1024;
    size_t v = cache[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        v = static_cast<size_t>(cus) * 4;
        cache[dev].store(v, std::memory_order_relaxed);
    }
    return v;
}

constexpr int LAT_WAVES_PER_SIMD = 7;

// true: the launch runs the few-waves form of its generator
bool few_waves_launch(size_t n_path)
{
    static const long long env_max = [] {
        const char *e = getenv("SVMC_FEW_WAVES_MAX_PATHS");
        return e ? static_cast<long long>(strtoull(e, nullptr, 10)) : -1ll;
    }();
    const size_t limit = env_max >= 0 ? static_cast<size_t>(env_max) : static_cast<size_t>(LAT_WAVES_PER_SIMD) * 64 * device_simds();
    return n_path <= limit;
}

// All expiries of a chain in ONE stepping launch: the slice loop runs inside the kernel, each slice with its own
// constants (dt, vol backbone) and its own epilogue (snapshot row i, spot partials column pair i).  Eight 128-step
// launches each pay their own ramp-up and ramp-down (C4: 8 x 1.03 ms against 7.44 ms for one 1024-step launch);
// here the chain pays one.  L and sigma^2 are re-derived from sigma at every slice start exactly as a fresh launch
// would (the slice is the one function the single-slice kernels call), so the results are the bits of the slice-by-slice path.
struct ChainSlices {
    LogsvFast c[MAX_CHAIN_SLICES];
    double forward[MAX_CHAIN_SLICES];
    int nb_steps[MAX_CHAIN_SLICES];
    int m, total_steps = 0;
    __device__ __forceinline__ LogsvFast consts(int i) const { return c[i]; }
};

// a (job, expiry) entry of the many-job table (ManyTable<LogsvFast>, svmc_jobs.h) goes through uniform_load: the step takes its
// constants as scalar operands
__device__ __forceinline__ LogsvFast many_consts_load(const LogsvFast *p) { return uniform_load(p); }

#ifndef SVMC_CHAIN_WAVES
#define SVMC_CHAIN_WAVES 8, 8          // A/B hook: residency of the whole-chain kernel (7, 8 lifts the 64-VGPR cap)
#endif
// The whole-chain kernel runs 1024-thread blocks: two blocks per CU share the CU's LDS, which leaves room -- beside the
// draw's 32 KB table -- to PARK each path's x and qvar (16 KB per block) while the time loop runs.  They are dead inside
// the loop (the loop advances the accumulators, logsv_fold_acc folds them in at the slice's end) but live across it, and
// in registers they pushed the kernel over the 64 VGPRs that eight waves per SIMD allow: the round-2 kernel spilled 68
// bytes per lane to scratch at every slice boundary (2.4 x its algorithmic HBM traffic).  Now: no scratch.
#ifndef SVMC_CHAIN_BLOCK
#define SVMC_CHAIN_BLOCK 1024
#endif
#ifndef SVMC_CHAIN_SGPRS
#define SVMC_CHAIN_SGPRS 80            // the slice loop's scalars on top of the stepping loop's; 80 still admits 8 waves per SIMD
#endif
constexpr int CHAIN_BLOCK = SVMC_CHAIN_BLOCK;
static inline unsigned chain_grid(size_t n) { return static_cast<unsigned>((n + CHAIN_BLOCK - 1) / CHAIN_BLOCK); }

// the body of the full-launch whole-chain kernels (logsv_chain_rng_kernel, logsv_chain_rng_many_kernel)
template <class Source>
__device__ __forceinline__ void logsv_chain_full_body(size_t n, const Source &src, uint64_t path_offset, double *__restrict__ x_snap,
                                                      double *__restrict__ q_snap, double *__restrict__ partials, uint64_t *probe)
{
    __shared__ RngTablesLds s_tab;
    __shared__ double s_exp[256];
    __shared__ double s_park[2 * CHAIN_BLOCK];             // [0, B): x, [B, 2B): qvar -- lane t owns elements t and B + t
    const RngTables tab = stage_tables<CHAIN_BLOCK>(s_tab, s_exp);
    clock_probe_stamp(probe, 0);
    // the path index is re-derived from threadIdx.x wherever it is needed (opaque to CSE): one VGPR across the time loop
    // instead of the 64-bit index and the addresses formed from it
    const auto path_index = [&]() {
        uint32_t t = threadIdx.x;
        asm volatile("" : "+v"(t));
        return static_cast<size_t>(blockIdx.x) * CHAIN_BLOCK + t;
    };
    const bool active = path_index() < n;
    double s;
    {
        double xv, q;
        src.start(path_index(), active, xv, s, q);
        s_park[threadIdx.x] = xv;
        s_park[CHAIN_BLOCK + threadIdx.x] = q;
    }
    const PhiloxLane lane = philox_prepare(src.seed(), src.c3(), path_offset + path_index());
    LogsvProgress prog = {(src.total_steps() + 3) >> 2};
    int tg = 0;
    for (int i = 0; i < src.m(); ++i) {
        const int nb = src.nb_steps(i);
        // every lane steps, the lanes past the last path on a dummy state: inside `if (active)` the progress counters
        // would be divergent values (vector registers, exec-masked branches in the time loop)
        const LogsvFast c = src.consts(i);
        const LogsvSliceSums a = logsv_slice_full(c, s, lane, src.step_origin() + static_cast<uint32_t>(tg), tg, nb, tab, s_exp, prog);
        double xv = s_park[threadIdx.x];                   // a lane reads back what it alone wrote: no barrier needed
        double q = s_park[CHAIN_BLOCK + threadIdx.x];
        logsv_fold_acc(c, xv, q, a.xacc, a.acc, a.s2_start, square_rn(s));
        s_park[threadIdx.x] = xv;
        s_park[CHAIN_BLOCK + threadIdx.x] = q;
        tg += nb;
        slice_epilogue(slice_out_row(x_snap, q_snap, partials, src.row(i), n, src.forward(i)), path_index(), active, xv, q);
    }
    if (active) src.finish(path_index(), s_park[threadIdx.x], s, s_park[CHAIN_BLOCK + threadIdx.x]);
    clock_probe_stamp(probe, 1);
}

// ... and of the whole-chain kernels for a launch of a few waves per SIMD (see logsv_rng_lat_kernel): the same slice loop on
// logsv_slice_lat -- the same bits -- with x and qvar in registers (there are registers to spare)
template <int LOOP, int TB, class Source>
__device__ __forceinline__ void logsv_chain_lat_body(size_t n, const Source &src, uint64_t path_offset, double *__restrict__ x_snap,
                                                     double *__restrict__ q_snap, double *__restrict__ partials, uint64_t *probe)
{
    __shared__ RngTablesLds s_tab;
    __shared__ double s_exp[256];
    const RngTables tab = stage_tables(s_tab, s_exp);
    clock_probe_stamp(probe, 0);
    const size_t p = static_cast<size_t>(blockIdx.x) * TB + threadIdx.x;
    const bool active = p < n;
    double xv, s, q;
    src.start(p, active, xv, s, q);
    const PhiloxLane lane = philox_prepare(src.seed(), src.c3(), path_offset + p);
    int tg = 0;
    for (int i = 0; i < src.m(); ++i) {
        const int nb = src.nb_steps(i);
        logsv_slice_lat<LOOP>(src.consts(i), xv, s, q, lane, src.step_origin() + static_cast<uint32_t>(tg), nb, tab, s_exp);
        tg += nb;
        slice_epilogue(slice_out_row(x_snap, q_snap, partials, src.row(i), n, src.forward(i)), p, active, xv, q);
    }
    if (active) src.finish(p, xv, s, q);
    clock_probe_stamp(probe, 1);
}

__global__ __launch_bounds__(CHAIN_BLOCK) __attribute__((amdgpu_waves_per_eu(SVMC_CHAIN_WAVES), amdgpu_num_sgpr(SVMC_CHAIN_SGPRS))) void logsv_chain_rng_kernel(
    double *__restrict__ x, double *__restrict__ sigma, double *__restrict__ qvar, size_t n, ChainSlices cs, uint64_t seed,
    uint32_t c3, uint64_t path_offset, uint32_t step_offset, double *__restrict__ x_snap, double *__restrict__ q_snap,
    double *__restrict__ partials, StateInit init, uint64_t *probe)
{
    logsv_chain_full_body(n, ChainArgs<ChainSlices>{cs, seed, c3, step_offset, init, x, sigma, qvar}, path_offset, x_snap, q_snap, partials,
                          probe);
}

template <int LOOP, int WAVES, int TB>
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void logsv_chain_rng_lat_kernel(
    double *__restrict__ x, double *__restrict__ sigma, double *__restrict__ qvar, size_t n, ChainSlices cs, uint64_t seed,
    uint32_t c3, uint64_t path_offset, uint32_t step_offset, double *__restrict__ x_snap, double *__restrict__ q_snap,
    double *__restrict__ partials, StateInit init, uint64_t *probe)
{
    logsv_chain_lat_body<LOOP, TB>(n, ChainArgs<ChainSlices>{cs, seed, c3, step_offset, init, x, sigma, qvar}, path_offset, x_snap, q_snap,
                                   partials, probe);
}

__global__ __launch_bounds__(CHAIN_BLOCK) __attribute__((amdgpu_waves_per_eu(SVMC_CHAIN_WAVES), amdgpu_num_sgpr(SVMC_CHAIN_SGPRS))) void logsv_chain_rng_many_kernel(
    size_t n, ManySlices cs, ManyJobs jobs, uint64_t path_offset, double *__restrict__ x_snap, double *__restrict__ q_snap,
    double *__restrict__ partials, uint64_t *probe)
{
    logsv_chain_full_body(n, ManyTable<LogsvFast>{cs, jobs}, path_offset, x_snap, q_snap, partials, probe);
}

// (a few waves per SIMD in all: J x n paths)
template <int LOOP, int WAVES, int TB>
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void logsv_chain_rng_many_lat_kernel(
    size_t n, ManySlices cs, ManyJobs jobs, uint64_t path_offset, double *__restrict__ x_snap, double *__restrict__ q_snap,
    double *__restrict__ partials, uint64_t *probe)
{
    logsv_chain_lat_body<LOOP, TB>(n, ManyTable<LogsvFast>{cs, jobs}, path_offset, x_snap, q_snap, partials, probe);
}

// The few-waves form of the LogSV generators.
using LogsvSliceKernel = void (*)(double *, double *, double *, size_t, int, LogsvFast, uint64_t, uint32_t, uint64_t, uint32_t, SliceOut,
                                  StateInit, uint64_t *);
using LogsvChainKernel = void (*)(double *, double *, double *, size_t, ChainSlices, uint64_t, uint32_t, uint64_t, uint32_t, double *,
                                  double *, double *, StateInit, uint64_t *);
struct LogsvLatVariant {
    LogsvSliceKernel slice;
    LogsvChainKernel chain;
    int block;
};
static const LogsvLatVariant LOGSV_FEW_WAVES_KERNELS = {logsv_rng_lat_kernel<GEN_LOOP_PIPE, 4, FEW_BLOCK>,
                                                        logsv_chain_rng_lat_kernel<GEN_LOOP_PIPE, 4, FEW_BLOCK>, FEW_BLOCK};

// -> the few-waves kernels a launch of n_path paths runs, or null: the full-launch kernels
static const LogsvLatVariant *logsv_lat_variant(size_t n_path)
{
    return few_waves_launch(n_path) ? &LOGSV_FEW_WAVES_KERNELS : nullptr;
}

__device__ __forceinline__ void logsv_w_body(double *__restrict__ x, double *__restrict__ sigma,
                                             double *__restrict__ qvar, size_t n, int nb_steps, const LogsvConsts &c,
                                             const double *__restrict__ W0, const double *__restrict__ W1, size_t ldw,
                                             const SliceOut &so)
{
    const size_t p = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x;
    const bool active = p < n;
    double xv = 0.0, q = 0.0;
    if (active) {
        xv = x[p];
        q = qvar[p];
        double s = sigma[p];
        double L = log(s);
        const double *const w[2] = {W0 + p, W1 + p};
        streamed_time_loop<2>(w, ldw, nb_steps, [&](const double(&v)[2]) {
            logsv_step(c, xv, L, s, q, c.sdt * v[0], c.sdt * v[1]);                               // :1028-1030
        });
        x[p] = xv;
        sigma[p] = s;
        qvar[p] = q;
    }
    slice_epilogue(so, p, active, xv, q);
}

__global__ __launch_bounds__(BLOCK) void logsv_w_kernel(double *__restrict__ x, double *__restrict__ sigma,
                                                        double *__restrict__ qvar, size_t n, int nb_steps,
                                                        LogsvConsts c, const double *__restrict__ W0,
                                                        const double *__restrict__ W1, size_t ldw, SliceOut so)
{
    logsv_w_body(x, sigma, qvar, n, nb_steps, c, W0, W1, ldw, so);
}

// The same kernel with its model constants read from device memory: every launch argument is then fixed for a given
// chain and set of randoms, so the launch can sit in a captured hipGraph that is replayed for each new parameter set
// (svmc_chain.hip) -- only the small constants block is rewritten between replays.
__global__ __launch_bounds__(BLOCK) void logsv_w_indirect_kernel(double *__restrict__ x, double *__restrict__ sigma,
                                                                 double *__restrict__ qvar, size_t n, int nb_steps,
                                                                 const LogsvConsts *__restrict__ consts,
                                                                 const double *__restrict__ W0,
                                                                 const double *__restrict__ W1, size_t ldw, SliceOut so)
{
    const LogsvConsts c = *consts;                      // wave-uniform: scalar loads
    logsv_w_body(x, sigma, qvar, n, nb_steps, c, W0, W1, ldw, so);
}

// All expiries of a chain on resident fixed randoms in ONE launch, state initialised in the kernel: what the graph of
// svmc_logsv_chain_price_fixed replays per calibration iterate.  An objective evaluation on a 4 x 13 chain with 10^5 paths
// is a dozen microsecond-scale kernels; one launch per expiry (+ its reduce) and a separate fill were most of them.
// Per slice the arithmetic is logsv_w_body's (L re-derived from sigma at the slice start), so the bits equal the
// slice-by-slice launches.  `init` != nullptr: start every path from (0, *init, 0) instead of reading the state.
static_assert(MAX_FUSED_SLICES == MAX_CHAIN_SLICES, "svmc_internal.h and the chain kernels must agree");
struct ChainWSlices {
    const double *W0[MAX_CHAIN_SLICES], *W1[MAX_CHAIN_SLICES];
    double forward[MAX_CHAIN_SLICES];
    int nb_steps[MAX_CHAIN_SLICES];
    int m;
};

__global__ __launch_bounds__(BLOCK) void logsv_chain_w_indirect_kernel(double *__restrict__ x, double *__restrict__ sigma,
                                                                       double *__restrict__ qvar, size_t n, ChainWSlices cs,
                                                                       const LogsvConsts *__restrict__ consts,
                                                                       const double *__restrict__ init, size_t ldw,
                                                                       double *__restrict__ x_snap, double *__restrict__ q_snap,
                                                                       double *__restrict__ partials)
{
    const size_t p = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x;
    const bool active = p < n;
    double xv = 0.0, s = 1.0, q = 0.0;
    if (active) {
        if (init != nullptr) {
            s = *init;
        } else {
            xv = x[p];
            s = sigma[p];
            q = qvar[p];
        }
    }
    for (int i = 0; i < cs.m; ++i) {
        if (active) {
            const LogsvConsts c = consts[i];                    // wave-uniform: scalar loads
            double L = log(s);
            const double *const w[2] = {cs.W0[i] + p, cs.W1[i] + p};
            streamed_time_loop<2>(w, ldw, cs.nb_steps[i], [&](const double(&v)[2]) {
                logsv_step(c, xv, L, s, q, c.sdt * v[0], c.sdt * v[1]);                           // :1028-1030
            });
        }
        const SliceOut so = {x_snap + static_cast<size_t>(i) * n, q_snap ? q_snap + static_cast<size_t>(i) * n : nullptr,
                             partials + 2 * static_cast<size_t>(i) * ((n + 63) >> 6), cs.forward[i], (n + 63) >> 6};
        slice_epilogue(so, p, active, xv, q);
    }
    if (active) {
        x[p] = xv;
        sigma[p] = s;
        qvar[p] = q;
    }
}

// The same chain for P PARAMETER SETS in one launch, the resident randoms read ONCE: every lane carries the P states of
// its path and steps them all on each pair of normals it loads.  The single-set launch moves 16 B per path-step for some
// 45 instructions of arithmetic and is HBM-bound on a calibration-sized path set (5.2 TB/s); the base point of an SLSQP
// iterate and its finite-difference neighbours share their randoms, so P sets cost one pass over them.  Per set the
// arithmetic is logsv_chain_w_indirect_kernel's, statement for statement (L re-derived from sigma at every slice start;
// the same step, the same epilogue), hence the same bits as P single-set launches.  The model constants of the
// (slice, set) pairs sit in LDS: P x 13 doubles would not fit the scalar registers, and in vector registers they would
// cost the residency the loads need -- a broadcast ds_read per use runs beside the VALU stream.
// consts: [m][P] LogsvConsts, init: [P] initial volatilities, x_snap / q_snap rows and partial column pairs: set-major,
// (set s, slice i) at s m + i.
constexpr int MAX_CHAIN_SETS = 8;
static_assert(MAX_FUSED_SETS == MAX_CHAIN_SETS, "svmc_internal.h and the chain kernels must agree");
template <int P>
__global__ __launch_bounds__(BLOCK) void logsv_chain_w_sets_kernel(size_t n, ChainWSlices cs,
                                                                   const LogsvConsts *__restrict__ consts,
                                                                   const double *__restrict__ init, size_t ldw,
                                                                   double *__restrict__ x_snap, double *__restrict__ q_snap,
                                                                   double *__restrict__ partials)
{
    __shared__ LogsvConsts s_c[P];
    const size_t p = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x;
    const bool active = p < n;
    double xv[P], sg[P], q[P], L[P];
#pragma unroll
    for (int s = 0; s < P; ++s) {
        xv[s] = 0.0;
        sg[s] = init[s];
        q[s] = 0.0;
    }
    for (int i = 0; i < cs.m; ++i) {
        __syncthreads();                                   // everybody is done with the previous slice's constants
        {
            constexpr int ND = P * static_cast<int>(sizeof(LogsvConsts) / sizeof(double));
            const double *src = reinterpret_cast<const double *>(consts + static_cast<size_t>(i) * P);
            double *dst = reinterpret_cast<double *>(s_c);
            for (int j = threadIdx.x; j < ND; j += BLOCK) dst[j] = src[j];
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int s = 0; s < P; ++s) L[s] = log(sg[s]);
            const double *const w[2] = {cs.W0[i] + p, cs.W1[i] + p};
            streamed_time_loop<2>(w, ldw, cs.nb_steps[i], [&](const double(&v)[2]) {
                // the constants are RE-READ from LDS at every step, not hoisted into 26 P registers: an opaque zero in the
                // index (not an opaque pointer -- that would turn the reads into flat loads, which wait on the global
                // loads in flight as well and undo the prefetch)
                unsigned zero = 0;
                asm volatile("" : "+v"(zero));
#pragma unroll
                for (int s = 0; s < P; ++s) {
                    const LogsvConsts c = s_c[s + zero];
                    logsv_step(c, xv[s], L[s], sg[s], q[s], c.sdt * v[0], c.sdt * v[1]);          // :1028-1030
                }
            });
        }
#pragma unroll
        for (int s = 0; s < P; ++s) {
            const int row = s * cs.m + i;
            const SliceOut so = {x_snap + static_cast<size_t>(row) * n, q_snap ? q_snap + static_cast<size_t>(row) * n : nullptr,
                                 partials + 2 * static_cast<size_t>(row) * ((n + 63) >> 6), cs.forward[i], (n + 63) >> 6};
            slice_epilogue(so, p, active, xv[s], q[s]);
        }
    }
}

// The calibration chain WITHOUT resident randoms: P parameter sets stepped on randoms that are REGENERATED in registers
// from (seed, call_id) on every evaluation.  A counter-based stream is already "frozen by its seed": the fixed randoms of
// an MC calibration (pricers/logsv_pricer.py:244-265, :520-527 draw them once with RandomState and keep the arrays) need
// not exist anywhere -- the round-4 route drew 582 MB into HBM for 10^5 x 364 and streamed them back at every objective
// evaluation (5.3 TB/s, the kernel's floor).  Here a lane draws its path's normals once per step (one Philox call per
// two steps, the inversion per word: 28 of the single-set generator's 49 instructions per step) and advances ALL P states
// on them; the P chains of a lane are independent, so their exp-table round trips overlap and one wave per SIMD -- what a
// calibration-sized path set gives this chip -- keeps its SIMD busy.  No HBM term inside the time loop at all.
// Per set the arithmetic is logsv_chain_rng_kernel's, statement for statement (logsv_step_acc on the constants in log
// units, L re-derived with log_state at every slice start, logsv_fold_acc, slice_epilogue): set q of the launch is
// logsv_mc_chain_pricer(seed, call_id) with set q's parameters, bit for bit.  The constants of the (slice, set) pairs sit
// in LDS and are re-read at every trip (as logsv_chain_w_sets_kernel: 5 P doubles would not fit the scalar registers and
// in vector registers they would be spilled); x and qvar stay in registers (they are dead inside the loop, but a
// calibration-sized launch runs one or two waves per SIMD: there are registers to spare).
// consts: [m][P] LogsvFast in log units, init: [P] initial volatilities; snapshot rows and partial column pairs set-major.
struct ChainRngSetsSlices {
    double forward[MAX_CHAIN_SLICES];
    int nb_steps[MAX_CHAIN_SLICES];
    int m;
};
constexpr int LOGSV_FAST_DOUBLES = static_cast<int>(sizeof(LogsvFast) / sizeof(double));

//
// Latency, not issue, bounds a calibration-sized launch: 10^5 paths are 1563 waves for 1024 SIMDs, one or two per SIMD, and a
// step is a dependent chain of about twenty fp64 operations around an LDS round trip.  Hence (profiles/r05_frozen_*.txt):
//   * the register allocator is told the launch runs two waves per SIMD (amdgpu_waves_per_eu(2, 2): 256 registers) --
//     left at its default it schedules for eight, reuses a handful of registers for every LDS read and waits for each read
//     before issuing the next (185 full lgkmcnt waits per trip at P = 8);
//   * the step runs piece by piece across the P states (logsv_step_acc_sets_front / _back), all P exp-table reads in flight
//     together;
//   * the time loop is the generators' pipelined one (rng_time_loop_pipelined): the step in two halves around its P exp-table
//     reads, the next pair's cubics, the next Philox call and the issue of the pair after that between them -- which
//     (path, step) sees which word is rng_time_loop's rule, unchanged.  One / seven sets: 0.150 / 0.401 ms per evaluation
//     (profiles/r06_frozen_objective.jsonl); round 5's draw forms: profiles/r05_frozen_objective.jsonl;
//   * the (slice, set) constants are plain loads from the block's LDS copy: loop-invariant, the compiler keeps them in
//     registers across the time loop where the budget allows and re-reads them where it does not.
// The launch shape (block size, one block per CU) was measured NOT to matter: the dispatcher spreads 391 blocks evenly.
template <int P>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2)))
void logsv_chain_rng_sets_kernel(size_t n, ChainRngSetsSlices cs, const LogsvFast *__restrict__ consts,
                                 const double *__restrict__ init, int p_total, int s0, uint64_t seed, uint32_t c3,
                                 uint64_t path_offset, uint32_t step_offset, double *__restrict__ x_snap,
                                 double *__restrict__ q_snap, double *__restrict__ partials, uint64_t *probe)
{
    // this launch advances the sets s0 .. s0 + P - 1 of the call's p_total (eight sets run as two launches of four: eight
    // states per lane need more than the 256 registers two waves per SIMD leave)
    __shared__ RngTablesLds s_tab;
    __shared__ double s_exp[256];
    __shared__ LogsvFast s_c[P];
    // six and more sets: x and qvar -- dead inside the time loop, live across it -- are parked in LDS (lane t owns its own
    // 2 P words, no barrier), as the whole-chain generator does: with them the eight-set kernel needed 266 registers, one
    // wave per SIMD, and a 10^5-path launch then runs in two rounds
    constexpr bool PARK = P >= 6;
    __shared__ double s_park[PARK ? 2 * P * BLOCK : 1];
    const RngTables tab = stage_tables(s_tab, s_exp);
    clock_probe_stamp(probe, 0);
    const size_t p = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x;
    const bool active = p < n;
    // (spreading the sets over groups of blocks instead -- more waves of fewer states each -- was measured and is slower at
    // every set count: two sets 0.221 -> 0.289 ms, four 0.302 -> 0.363, six 0.386 -> 0.439; an extra state in a lane costs
    // 40 us, an extra wave of one state 107)
    double xv[P], sg[P], q[P];
#pragma unroll
    for (int s = 0; s < P; ++s) {
        xv[s] = 0.0;
        sg[s] = init[s0 + s];
        q[s] = 0.0;
        if constexpr (PARK) {
            s_park[(2 * s) * BLOCK + threadIdx.x] = 0.0;
            s_park[(2 * s + 1) * BLOCK + threadIdx.x] = 0.0;
        }
    }
    // every lane steps (the lanes past the last path on a real path's counter: their results are never stored)
    const PhiloxLane lane = philox_prepare(seed, c3, path_offset + p);
    uint32_t tg = step_offset;
    for (int i = 0; i < cs.m; ++i) {
        __syncthreads();                                   // everybody is done with the previous slice's constants
        {
            constexpr int ND = P * LOGSV_FAST_DOUBLES;
            const double *src = reinterpret_cast<const double *>(consts + static_cast<size_t>(i) * p_total + s0);
            double *dst = reinterpret_cast<double *>(s_c);
            for (int j = threadIdx.x; j < ND; j += BLOCK) dst[j] = src[j];
        }
        __syncthreads();
        const int nb = cs.nb_steps[i];
        double L[P], acc[P], xacc[P], s2_start[P], k1[P], k2[P], k3[P], kb[P], ke[P];
#pragma unroll
        for (int s = 0; s < P; ++s) {
            L[s] = log_state(sg[s]) * LOG_UNITS_PER_NAT;                                              // :1039
            s2_start[s] = square_rn(sg[s]);
            acc[s] = 0.0;
            xacc[s] = 0.0;
            k1[s] = s_c[s].c1;
            k2[s] = s_c[s].c2;
            k3[s] = s_c[s].c3;
            kb[s] = s_c[s].bs;
            ke[s] = s_c[s].es;
        }
        LogsvSetsInFlight<P> h;
        if constexpr (P <= 6) {
            // the tails in the middle region on coefficients in vector registers (seven sets have no registers left for them)
            const Exp2uTailV tail_k = exp2u_tail_consts();
            rng_time_loop_pipelined(
                lane, tg, nb, tab,
                [&](double z0, double z1) { logsv_step_acc_sets_front<P>(k1, k2, k3, kb, ke, xacc, L, sg, acc, z0, z1, s_exp, h); },
                [&]() { logsv_step_acc_sets_mid<P>(h, tail_k); }, [&]() { logsv_step_acc_sets_back<P, true>(sg, h); });
        } else {
            rng_time_loop_pipelined(
                lane, tg, nb, tab,
                [&](double z0, double z1) { logsv_step_acc_sets_front<P>(k1, k2, k3, kb, ke, xacc, L, sg, acc, z0, z1, s_exp, h); },
                [&]() { logsv_step_acc_sets_back<P>(sg, h); });
        }
        tg += static_cast<uint32_t>(nb);
#pragma unroll
        for (int s = 0; s < P; ++s) {
            const LogsvFast c = s_c[s];
            if constexpr (PARK) {
                xv[s] = s_park[(2 * s) * BLOCK + threadIdx.x];
                q[s] = s_park[(2 * s + 1) * BLOCK + threadIdx.x];
            }
            logsv_fold_acc(c, xv[s], q[s], xacc[s], acc[s], s2_start[s], square_rn(sg[s]));
            if constexpr (PARK) {
                s_park[(2 * s) * BLOCK + threadIdx.x] = xv[s];
                s_park[(2 * s + 1) * BLOCK + threadIdx.x] = q[s];
            }
            const int row = (s0 + s) * cs.m + i;
            slice_epilogue(slice_out_row(x_snap, q_snap, partials, static_cast<size_t>(row), n, cs.forward[i]), p, active, xv[s], q[s]);
        }
    }
    clock_probe_stamp(probe, 1);
}

__global__ __launch_bounds__(BLOCK) void fill_state_indirect_kernel(double *__restrict__ x, double *__restrict__ vol,
                                                                    double *__restrict__ qvar, size_t n,
                                                                    const double *__restrict__ vol0)
{
    const size_t p = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x;
    if (p < n) {
        x[p] = 0.0;
        vol[p] = *vol0;
        qvar[p] = 0.0;
    }
}

// Volatility paths on the full grid (pricers/logsv_pricer.py:930-945): 8 B written per path-step.
//
// Round 4 (profiles/r04_vol_paths.json, tools/r04/write_bw.hip, tools/ubench/ab_vol_paths.py; 2^20 paths x 1024 steps, 8.6 GB):
//   * what the chip does with this store pattern and NO arithmetic -- a wave owns 64 columns and walks the rows, 512 B per
//     wave-store -- is 5.7 TB/s (hipMemset: 6.3; 8- and 16-byte stores, plain / nt / sc1 policies all within 3 %, nt the
//     slowest); a copy in the same pattern (supplied brownians: 8 B read + 8 B written per path-step) runs at 4.84 TB/s of
//     total traffic, as does hipMemcpy -- the SUPPLIED instantiation sits on that roof (3.5-3.6 ms for 17.2 GB).
//   * the DRAWING instantiation is POWER-bound, not store-bound: its arithmetic alone (stores disabled) takes 1.27 ms at a
//     measured 2.0 GHz, its stores alone 1.5 ms -- but with both the shader clock inside the kernel falls to 1.45-1.5 GHz
//     (clock_probe_stamp: s_memtime against s_memrealtime) and the launch takes 1.95 ms = 4.4 TB/s.  Sixteen-byte stores
//     through a wave-private LDS transpose (half the store instructions) measured 4-6 % SLOWER -- the extra LDS traffic costs
//     more power than the store issue it saves -- and were removed again; so were non-temporal and write-through policies.
//   * what did help is a SHORTER step, the generators' form: ln sigma carried in units of ln2/256 so that exp2u_tab's
//     reduction is exact, the drift regrouped into four FMAs on host-scaled constants (logsv_step_acc's), rcp_1n for the
//     1/sigma term (near theta it enters L at 1e-3 of its size): 48 -> 33 VALU instructions per path-step, 2.10 -> 1.95 ms on
//     one box.  Identical in exact arithmetic to :942; rounding differs at the 1e-16 level per step.  Both instantiations are
//     held to the recursion in 256-bit arithmetic within the LogSV generator's margins (tests/test_gpu_vol_paths_steps.py),
//     starts at theta / 50 and theta / 1000 included, where the 1/sigma term moves ln sigma by 0.44 and 8.8 in one step and
//     the reciprocal's error enters at full size: measured there within 2.9 times the fp64 recursion's own error
//     (profiles/vol_paths_step_observed_tolerances.txt).
//   * supplied brownians are loaded a group of four steps ahead.
//   * round 6: the next call's reads ahead and four steps with their four stores back to back were measured and not kept
//     (profiles/r06_vol_paths_ab.jsonl).
struct VolPathConsts {
    double c1;      // kappa1 theta dt K          (K = 256 / ln2: L is carried in units of ln2 / 256)
    double c2;      // (adj - kappa2) dt K
    double c3;      // (kappa2 theta - kappa1 - vartheta^2 / 2) dt K
    double cz;      // vartheta K for supplied (already scaled) increments, vartheta sqrt(dt) K for the kernel's own N(0,1)
    double L0;      // ln(v0) K
};

#ifndef SVMC_VOLPATHS_RNG_BLOCK
#define SVMC_VOLPATHS_RNG_BLOCK 1024   // drawing instantiation: two blocks per CU share one copy each of the draw's table
#endif
constexpr int VOLPATHS_RNG_BLOCK = SVMC_VOLPATHS_RNG_BLOCK;
template <bool RNG>
__global__ __launch_bounds__(RNG ? VOLPATHS_RNG_BLOCK : BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8)))
void logsv_vol_paths_kernel(double *__restrict__ sigma_t, size_t ld, size_t n, int nb_steps, double v0, VolPathConsts c,
                            const double *__restrict__ brownians, size_t ldb, uint64_t seed, uint32_t c3, uint64_t path_offset,
                            uint64_t *probe)
{
    constexpr int TB = RNG ? VOLPATHS_RNG_BLOCK : BLOCK;
    __shared__ RngTablesLdsIf<RNG> s_tab;                  // the draw's table only where the kernel draws
    __shared__ double s_exp[256];
    const RngTables tab = stage_tables_if(s_tab, s_exp);
    clock_probe_stamp(probe, 0);
    const size_t p = static_cast<size_t>(blockIdx.x) * TB + threadIdx.x;
    if (p < n) {
        double s = v0, L = c.L0;
        sigma_t[p] = s;                                                                         // :937
        double *out = sigma_t + ld + p;                    // row t + 1 of this path
        const auto step = [&](double w) {                  // w: N(0,1) (RNG) or the scaled increment sqrt(dt) N(0,1)   :925
            const double y = rcp_1n(s);
            L = fma(c.c2, s, L);                                                                // :942, regrouped
            L = fma(c.c1, y, L);
            L = L + c.c3;
            L = fma(c.cz, w, L);
            s = exp2u_tab(L, s_exp);                                                            // :943
            *out = s;                                                                           // :944
            out += ld;
        };
        int t = 0;
        if (RNG) {
            // one Brownian per step: normal t is the inversion of word t & 3 of call t >> 2 (stream 2) -- a Philox call
            // serves four steps, so the loop runs call by call with no per-step selects
            const PhiloxLane pl = philox_prepare(seed, c3 | 2u, path_offset + p);
            uint32_t r[4];
            double a0, a1, b0, b1;
            for (; t + 4 <= nb_steps; t += 4) {
                philox_draw(pl, static_cast<uint32_t>(t >> 2), r);
                normals_from_words(r[0], r[1], tab, a0, a1);
                normals_from_words(r[2], r[3], tab, b0, b1);
                step(a0);
                step(a1);
                step(b0);
                step(b1);
            }
            if (t < nb_steps) {                            // the last, partial call (wave-uniform)
                philox_draw(pl, static_cast<uint32_t>(t >> 2), r);
                normals_from_words(r[0], r[1], tab, a0, a1);
                step(a0);
                if (t + 1 < nb_steps) step(a1);
                if (t + 2 < nb_steps) {
                    normals_from_words(r[2], r[3], tab, b0, b1);
                    step(b0);
                }
            }
        } else {
            const double *w = brownians + p;
            double a[4], b[4];
            if (nb_steps >= 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) a[u] = w[static_cast<size_t>(u) * ldb];
                for (; t + 8 <= nb_steps; t += 4) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) b[u] = w[static_cast<size_t>(t + 4 + u) * ldb];   // the next group, in flight
#pragma unroll
                    for (int u = 0; u < 4; ++u) step(a[u]);
#pragma unroll
                    for (int u = 0; u < 4; ++u) a[u] = b[u];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) step(a[u]);
                t += 4;
            }
            for (; t < nb_steps; ++t) step(w[static_cast<size_t>(t) * ldb]);
        }
    }
    clock_probe_stamp(probe, 1);
}

// ---- what the callers of simulate_vol_paths do with the array, done where the array is -------------------------------
// The reference's users of the [nb_steps + 1][nb_path] volatility paths reduce them over the PATH axis at every time step
// (papers/logsv_model_with_quadratic_drift/moments_vol_qvar.py:48 np.mean / np.std of (sigma_t - theta)^k along axis 1, :98
// of sigma_t and of the expanding time average of sigma_t^2): 8.6 GB over PCIe to keep 1025 x 8 numbers.  Two kernels on the
// resident array instead, both HBM-bound single passes:
//   row_power_sums_kernel      per row t: sums over the paths of (a[t][p] - center)^j, j = 1 .. 2 K  (mean and variance of the
//                              first K central-ish moments); one block per (row, segment), deterministic tree
//   expanding_mean_sq_kernel   per path p: out[t][p] = mean of a[u][p]^2 over u <= t  (pandas expanding().mean() of the squares)
constexpr int ROW_MOMENTS_MAX = 4;
constexpr int ROW_SEGMENTS = 4;        // blocks per row: 1025 rows x 4 fill the chip; their partial sums are added in order

// Round 6: both kernels read 16 bytes per lane and keep eight (row sums) / four (expanding mean) such loads in flight -- 32 KB
// per block, several blocks per CU -- where round 5's read 8 bytes four deep and stood at 5.0 / 4.5 TB/s (0.63 / 0.56 of the
// HBM peak; logsv_w_kernel, the same kind of pass, reaches 5.9).  The expanding mean also lost its fp64 DIVIDE per element
// (about forty instructions: 1.1 ms of issue for 2^30 elements beside 2.9 ms of memory time): the divisor of a row is the
// same for every path, so each block forms the reciprocals 1 / (t + 1) of a chunk of rows once, in LDS, by the correctly
// rounded division, and an element costs one multiplication -- within an ulp of the quotient.
constexpr int ROW_SUM_U = 8;           // 16-byte loads in flight per lane

template <int K>
__global__ __launch_bounds__(BLOCK) void row_power_sums_kernel(const double *__restrict__ a, size_t ld, size_t n_cols, double center,
                                                               double *__restrict__ partials /* [rows][ROW_SEGMENTS][2K] */)
{
    __shared__ double lds[4 * block_sum_padded(2 * K)];
    const size_t row = blockIdx.x, seg = blockIdx.y;
    const double *__restrict__ src = a + row * ld;
    size_t lo = n_cols * seg / ROW_SEGMENTS;
    const size_t hi = n_cols * (seg + 1) / ROW_SEGMENTS;
    double acc[2 * K];
#pragma unroll
    for (int j = 0; j < 2 * K; ++j) acc[j] = 0.0;
    const auto add = [&](double v) {
        const double d = v - center;
        double pw = d;
#pragma unroll
        for (int j = 0; j < 2 * K; ++j) {
            acc[j] += pw;
            pw *= d;
        }
    };
    // a segment that does not start on a 16-byte boundary gives its first element to thread 0 (block-uniform test)
    if (lo < hi && (reinterpret_cast<uintptr_t>(src + lo) & 15u) != 0u) {
        if (threadIdx.x == 0) add(src[lo]);
        ++lo;
    }
    const size_t pairs = (hi - lo) >> 1;                   // double2 elements of the aligned body
    const double2 *__restrict__ src2 = reinterpret_cast<const double2 *>(src + lo);
    size_t i = threadIdx.x;
    for (; i + (ROW_SUM_U - 1) * BLOCK < pairs; i += ROW_SUM_U * BLOCK) {
        double2 v[ROW_SUM_U];
#pragma unroll
        for (int u = 0; u < ROW_SUM_U; ++u) v[u] = src2[i + u * BLOCK];
#pragma unroll
        for (int u = 0; u < ROW_SUM_U; ++u) {
            add(v[u].x);
            add(v[u].y);
        }
    }
    for (; i < pairs; i += BLOCK) {
        const double2 v = src2[i];
        add(v.x);
        add(v.y);
    }
    if (((hi - lo) & 1u) != 0u && threadIdx.x == 0) add(src[hi - 1]);
    block_sum_store<2 * K>(acc, lds, partials + (row * ROW_SEGMENTS + seg) * (2 * K), 2 * K);
}

// out[t][p] = mean of a[u][p]^2 over u <= t.  PAIR: a lane owns the two adjacent columns 2 i, 2 i + 1 and moves 16 bytes per
// access (the caller checks that both arrays and leading dimensions allow it); otherwise one column, 8 bytes.
constexpr int EXPANDING_CHUNK = 1024;  // rows whose reciprocals a block holds in LDS at a time
template <bool PAIR>
__global__ __launch_bounds__(BLOCK) void expanding_mean_sq_kernel(const double *__restrict__ a, size_t ld, size_t n_rows, size_t n_cols,
                                                                  double *__restrict__ out, size_t ldo)
{
    __shared__ double s_inv[EXPANDING_CHUNK];
    using Vec = typename std::conditional<PAIR, double2, double>::type;
    constexpr size_t W = PAIR ? 2 : 1;
    const size_t p = (static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x) * W;
    const bool active = p < n_cols;                        // (PAIR: n_cols is even)
    double q0 = 0.0, q1 = 0.0;
    for (size_t t0 = 0; t0 < n_rows; t0 += EXPANDING_CHUNK) {
        const size_t nt = (n_rows - t0 < static_cast<size_t>(EXPANDING_CHUNK)) ? n_rows - t0 : EXPANDING_CHUNK;
        __syncthreads();                                   // everybody is done with the previous chunk's reciprocals
        for (size_t j = threadIdx.x; j < nt; j += BLOCK) s_inv[j] = 1.0 / static_cast<double>(t0 + j + 1);
        __syncthreads();
        if (!active) continue;
        const auto one = [&](const Vec &v, size_t j) {
            Vec o;
            if constexpr (PAIR) {
                q0 = fma(v.x, v.x, q0);
                q1 = fma(v.y, v.y, q1);
                o.x = q0 * s_inv[j];
                o.y = q1 * s_inv[j];
            } else {
                q0 = fma(v, v, q0);
                o = q0 * s_inv[j];
            }
            *reinterpret_cast<Vec *>(out + (t0 + j) * ldo + p) = o;
        };
        size_t j = 0;
        for (; j + 4 <= nt; j += 4) {                      // four rows in flight
            Vec v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const Vec *>(a + (t0 + j + u) * ld + p);
#pragma unroll
            for (int u = 0; u < 4; ++u) one(v[u], j + u);
        }
        for (; j < nt; ++j) one(*reinterpret_cast<const Vec *>(a + (t0 + j) * ld + p), j);
    }
}

// ---------------------------------------------------------------------------------------------------
// Payoff reduction (utils/mc_payoffs.py:61-88).  Deterministic two-stage sums: per-block partials in a
// fixed tree order, then one block per output column adds the partials -- no fp64 atomics, so a given
// (n_path, grid) always reproduces the same bits.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void spot_sums_kernel(const double *__restrict__ x, size_t n, double forward,
                                                          double *__restrict__ partials)
{
    __shared__ double lds[8];
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    double v[2] = {0.0, 0.0};
    for (size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x; i < n; i += stride) {
        const double sp = forward * exp_full(x[i]);        // full-range exp (user data may hold +-inf)     :61
        if (sp == sp) {                                                                         // nanmean :62
            v[0] += sp;
            v[1] += 1.0;
        }
    }
    block_sum_store<2>(v, lds, partials + 2 * static_cast<size_t>(blockIdx.x), 2);
}

// ---- per-strike payoff sums: ONE pass over the terminal values of an expiry for all of its strikes ---------------
// One block column (blockIdx.y) = one GROUP: up to KT strikes of ONE expiry (an expiry with more strikes is split
// into several groups); the group descriptor carries that expiry's snapshot pointers, forward and recentring sums.  A
// thread reads a path's x ONCE and exponentiates it ONCE for all the strikes of the group (round 1 took a pass and an
// exp per chunk of 8 strikes: three passes for the 21 strikes of the BASELINE chains).
//   plain payoffs (C / P):  pay = max(sg (u - K), 0), sg = +1 call / -1 put, computed as max(fma(sg, u, -sg K), 0) with sg
//     a wave-uniform (SGPR) operand of the FMA: fmax returns 0 for a NaN underlying, which is np.where(u > K, u - K, 0)
//     (:75-82) -- a plain payoff is never NaN, so nanmean / nanstd count EVERY path and the count column is the block's
//     path count, not an accumulator: 5 VALU instructions per strike per path (fma, max, subtract the shift, two
//     accumulates) and 4 doubles of vector state per strike (two accumulators, two constants: 192 VGPRs at 24
//     strikes).  The time loop has NO per-strike condition: the unused strikes of a group carry c = -inf.
//   inverse payoffs (IC / IP, HAS_INV): pay / spot can be NaN (0/0, inf/inf): per-strike NaN test and count kept.
constexpr int PAYOFF_GROUPS = 8;       // groups per launch: 8 x 440 B of descriptors stay inside the 4 KB kernarg segment
#ifndef SVMC_PAYOFF_PREFETCH
#define SVMC_PAYOFF_PREFETCH 4
#endif
constexpr int PAYOFF_PREFETCH = SVMC_PAYOFF_PREFETCH;     // trips between a path's load and its use (A/B: tools/ubench)
#ifndef SVMC_PAYOFF_BLOCKS
#define SVMC_PAYOFF_BLOCKS 1024
#endif
constexpr unsigned PAYOFF_BLOCKS = SVMC_PAYOFF_BLOCKS;    // path blocks per payoff launch, all groups together
constexpr int PAYOFF_KT = 22;          // strikes per group (the BASELINE chains have 21 per expiry); 23 and 24 spilled 20-44 B per lane at the 256 registers two waves per SIMD leave, so wider expiries split

struct PayoffGroup {
    const double *x, *qvar, *spot_sums;
    double forward, ttm;
    double c[PAYOFF_KT];       // -sg K; -inf for the unused strikes of a group (their payoff is 0 and their sums are dropped)
    double shift[PAYOFF_KT];   // sums are taken of (payoff - shift): removes the E[p^2] - E[p]^2 cancellation
    uint32_t inv_mask;         // bit k set: divide by the recentred spot (IC / IP)
    uint32_t put_mask;         // bit k set: put, sg = -1; clear: call, sg = +1: pay = max(fma(sg, u, c), 0)
    int k;                     // live strikes in this group
    int col;                   // first output column of the group within this launch (in strikes)
    // round 6: the expiry's spot sums formed IN this kernel from the generators' per-wave partial columns (column 0 at
    // spot_partials, column 1 spot_rows further on) instead of by a reduce launch ahead of it; null: read spot_sums
    const double *spot_partials;
    unsigned spot_rows;
};
struct PayoffGroupPack {
    PayoffGroup g[PAYOFF_GROUPS];
};
// parameter sets of one chain (the calibration's bumped evaluations) share every descriptor; their snapshots, spot sums and
// output rows lie at fixed distances, and blockIdx.z picks the set: doubles between consecutive sets (zeros for one set)
struct PayoffSetStrides {
    size_t x, q, spot;
};
static_assert(sizeof(PayoffGroupPack) + sizeof(PayoffSetStrides) + 64 <= 4096, "the payoff descriptors travel in the kernel arguments");

// number of indices i < n visited by block b of a grid-stride loop (stride = grid * BLOCK, BLOCK consecutive per block)
__device__ __forceinline__ double block_path_count(size_t n, unsigned b, unsigned grid)
{
    const size_t stride = static_cast<size_t>(grid) * BLOCK, lo = static_cast<size_t>(b) * BLOCK;
    const size_t full = n / stride, rem = n % stride;
    const size_t part = (rem > lo) ? ((rem - lo < static_cast<size_t>(BLOCK)) ? rem - lo : BLOCK) : 0;
    return static_cast<double>(full * BLOCK + part);
}

// waves per SIMD the register allocator must leave room for: the accumulators (4 or 6 registers per strike) set it
// waves per SIMD of a payoff instantiation, stated EXACTLY (min = max): left a range, the compiler aims for more waves than
// the accumulators leave registers for and spills (round 3: eleven instantiations carried 20-100 bytes of scratch per lane).
// The thresholds are the widest groups whose build metadata shows no scratch (libsvmc.isa.json "metadata";
// tests/test_host_logic.py holds every payoff instantiation to scratch_bytes == 0).
constexpr int payoff_min_waves(int kt, bool has_inv) { return kt <= (has_inv ? 5 : 12) ? 3 : 2; }

template <int KT, bool HAS_INV, bool NEED_Q>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(payoff_min_waves(KT, HAS_INV), payoff_min_waves(KT, HAS_INV)))) void payoff_group_kernel(PayoffGroupPack pack, size_t n, double *__restrict__ partials, int ld, PayoffSetStrides sets)
{
    constexpr int NACC = HAS_INV ? 3 : 2;
    __shared__ double lds[4 * block_sum_padded(NACC * KT)];
    const PayoffGroup &d = pack.g[blockIdx.y];
    const size_t set = blockIdx.z;                          // parameter set (one launch prices gridDim.z of them)
    const double *__restrict__ x = d.x + set * sets.x;
    const double *__restrict__ qvar = NEED_Q ? d.qvar + set * sets.q : nullptr;
    const double forward = d.forward, inv_ttm_arg = d.ttm;
    double spot0, spot1;
    if (d.spot_partials != nullptr) {                       // (block-uniform)
        // [sum F exp(x), count] of this expiry from the generators' per-wave rows, in block_column_sum's order: the bits of
        // reduce_columns_kernel, formed by every block for itself (a few rows per thread out of L2) instead of by a launch
        __shared__ double s_spot[2];
        const double *__restrict__ sp = d.spot_partials;   // (one-set launches only: payoff_sums_impl)
        double t0, t1;
        block_column_sum2(sp, sp + d.spot_rows, d.spot_rows, lds, t0, t1);
        if (threadIdx.x == 0) {
            s_spot[0] = t0;
            s_spot[1] = t1;
            if (blockIdx.x == 0 && d.spot_sums != nullptr) {        // ... and left where a separate reduce would have put them
                double *out = const_cast<double *>(d.spot_sums);
                out[0] = t0;
                out[1] = t1;
            }
        }
        __syncthreads();
        spot0 = s_spot[0];
        spot1 = s_spot[1];
    } else {
        const double *__restrict__ spot_sums = d.spot_sums + set * sets.spot;
        spot0 = spot_sums[0];
        spot1 = spot_sums[1];
    }
    const double corr = spot0 / spot1 - forward;                                                // :62
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    const int nk = d.k;
    const uint32_t inv_mask = d.inv_mask;
    constexpr int NSUM = block_sum_padded(NACC * KT);      // the block sum's halving tree takes multiples of 8: zeros fill up
    double acc[NSUM], sg[KT], c[KT], shift[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        sg[k] = ((d.put_mask >> k) & 1u) ? -1.0 : 1.0;     // stays wave-uniform: the scalar operand of the FMA
        // plain chains: payoff - shift = max(sg u + c, 0) - shift = max(sg u + (c - shift), -shift): the recentring rides
        // in the FMA's addend and the max's floor, four instructions per strike per path instead of five
        if constexpr (HAS_INV) {
            c[k] = d.c[k];
            shift[k] = d.shift[k];
            // these two live in VECTOR registers: left wave-uniform the compiler keeps all three constants in SGPRs, runs
            // out (3 x 24 doubles) and re-reads the spills with v_readlane_b32 -- VALU instructions on top of the ones
            // that do the work
            asm volatile("" : "+v"(c[k]), "+v"(shift[k]));
        } else {
            // ... and both are RESULTS of vector arithmetic: they stay in vector registers without a pin, and fmax()
            // knows them quiet (an opaque operand costs a second v_max per strike per path to quiet it)
            c[k] = d.c[k] - d.shift[k];
            shift[k] = 0.0 - d.shift[k];
        }
    }
#pragma unroll
    for (int j = 0; j < NSUM; ++j) acc[j] = 0.0;
    constexpr bool need_q = NEED_Q;                        // options on realised variance (SVMC_Q_VAR)

    // one path's contribution to every strike of the group
    const auto add_path = [&](double xi, double qi) {
        const double spot = forward * exp_full(xi) - corr;                                      // :61-63
        const double u = need_q ? qi / inv_ttm_arg : spot;                                      // :65-68
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            if constexpr (HAS_INV) {
                double pay = fmax(fma(sg[k], u, c[k]), 0.0);                                    // :75-82
                if (inv_mask & (1u << k)) pay = pay / spot;
                if (pay == pay) {                                                               // nanmean/nanstd
                    const double dd = pay - shift[k];
                    acc[k] += dd;
                    acc[KT + k] = fma(dd, dd, acc[KT + k]);
                    acc[2 * KT + k] += 1.0;
                }
            } else {
                const double dd = fmax(fma(sg[k], u, c[k]), shift[k]);                          // :75-82, recentred
                acc[k] += dd;
                acc[KT + k] = fma(dd, dd, acc[KT + k]);
            }
        }
    };
    // A trip is ~130 VALU instructions (~0.25 us) and the kernel runs two or three waves per SIMD (its accumulators fill the
    // register file): a load issued one trip ahead is not back in time.  The trips every lane of the block makes go
    // through the batched double buffer of the streamed generators (loads PAYOFF_PREFETCH trips ahead, no per-lane
    // branches, so the waits are counted ones); the last, ragged trip is taken on its own.
    const size_t i0 = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x;
    const size_t block_last = static_cast<size_t>(blockIdx.x) * BLOCK + (BLOCK - 1);
    const int full_trips = (n > block_last) ? static_cast<int>((n - 1 - block_last) / stride + 1) : 0;     // block-uniform
    constexpr int PF = (KT >= (HAS_INV ? 15 : 22)) ? 2 : PAYOFF_PREFETCH;      // the widest groups have no registers to spare
    if constexpr (need_q) {
        const double *const w[2] = {x + i0, qvar + i0};
        streamed_time_loop<2, PF>(w, stride, full_trips, [&](const double(&v)[2]) { add_path(v[0], v[1]); });
    } else {
        const double *const w[1] = {x + i0};
        streamed_time_loop<1, PF>(w, stride, full_trips, [&](const double(&v)[1]) { add_path(v[0], 0.0); });
    }
    for (size_t i = i0 + static_cast<size_t>(full_trips) * stride; i < n; i += stride) add_path(x[i], need_q ? qvar[i] : 0.0);
    // output row layout: [sum d, sum d^2, count] per strike, interleaved, at column 3 (col + k)
    // (sets interleave within a block row: partials[path block][set][column], so that one column reduce serves them all)
    double *row = partials + (static_cast<size_t>(blockIdx.x) * gridDim.z + set) * ld + 3 * d.col;
    const double cnt = block_path_count(n, blockIdx.x, gridDim.x);
    block_sum_apply<NSUM>(acc, lds, NACC * KT, [&](int j, double t) {
        const int which = j / KT, k = j - which * KT;
        if (k < nk) {
            row[3 * k + which] = t;
            if (!HAS_INV && which == 0) row[3 * k + 2] = cnt;
        }
    });
}

// out[j] = sum_r partials[r * ld + j]; one block per column j
// element (row r, column j) sits at partials[r * row_stride + j * col_stride]: row-major block partials pass (ld, 1), the
// generators' per-wave spot partials are column-major and pass (1, rows)
__global__ __launch_bounds__(BLOCK) void reduce_columns_kernel(const double *__restrict__ partials_base, unsigned n_rows,
                                                               size_t row_stride, size_t col_stride, double *__restrict__ out)
{
    __shared__ double lds[4];
    const int j = blockIdx.x;
    const double t = block_column_sum(partials_base + static_cast<size_t>(j) * col_stride, n_rows, row_stride, lds);
    if (threadIdx.x == 0) out[j] = t;
}

// what every other unit launches reduce_columns_kernel through: out[j] for j < n_cols, queued on `stream`; the caller checks the launch
void reduce_columns(unsigned n_cols, hipStream_t stream, const double *partials_base, unsigned n_rows, size_t row_stride,
                    size_t col_stride, double *out)
{
    hipLaunchKernelGGL(reduce_columns_kernel, dim3(n_cols), dim3(BLOCK), 0, stream, partials_base, n_rows, row_stride, col_stride, out);
}

static inline unsigned reduce_grid(size_t n)
{
    const size_t g = (n + BLOCK - 1) / BLOCK;
    return static_cast<unsigned>(g < 1 ? 1 : (g > MAX_REDUCE_GRID ? MAX_REDUCE_GRID : g));
}

int check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SVMC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return SVMC_OK;
}

int check_state(const char *fn, const double *x, const double *v, const double *q, int nb_steps, double dt)
{
    if (x == nullptr || v == nullptr || q == nullptr) return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": null state pointer");
    if (nb_steps < 0) return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": nb_steps < 0");
    if (!(dt > 0.0)) return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": dt must be positive");
    return SVMC_OK;
}

// allow_null_spot (the two on-device-RNG slice launchers, for their internal callers only -- the public entry points reject a null
// spot_sums first): with spot_sums == nullptr the launch leaves its per-wave partial columns in the workspace unreduced, and the
// payoff kernel of svmc_chain.hip's one-device tail sums them itself
int check_slice_args(const char *fn, size_t n_path, const double *x_snapshot, const double *spot_sums,
                     const void *workspace, size_t workspace_bytes, bool allow_null_spot)
{
    if (x_snapshot == nullptr || (spot_sums == nullptr && !allow_null_spot) || workspace == nullptr)
        return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": null snapshot / spot_sums / workspace");
    if (workspace_bytes < static_cast<size_t>(wave_rows(n_path)) * 2 * sizeof(double))
        return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": workspace too small (svmc_slice_workspace_bytes)");
    return SVMC_OK;
}

}  // namespace svmc

using namespace svmc;

extern "C" {

int svmc_fill_state(double *x, double *vol, double *qvar, size_t n_path, double x0, double vol0, double qvar0,
                    svmc_stream_t stream)
{
    SVMC_REQUIRE(x && vol && qvar, "svmc_fill_state: null state pointer");
    if (n_path == 0) return SVMC_OK;
    hipLaunchKernelGGL(fill_state_kernel, dim3(grid_for(n_path)), dim3(BLOCK), 0, as_stream(stream), x, vol, qvar,
                       n_path, x0, vol0, qvar0);
    return check_launch("svmc_fill_state");
}

int svmc_fill_normals(double *W0, double *W1, size_t ldw, size_t n_path, int nb_steps, uint64_t seed,
                      uint32_t call_id, uint64_t path_offset, uint32_t step_offset, svmc_stream_t stream)
{
    SVMC_REQUIRE(W0 && W1, "svmc_fill_normals: null output");
    SVMC_REQUIRE(ldw >= n_path && nb_steps >= 0, "svmc_fill_normals: ldw < n_path or nb_steps < 0");
    SVMC_REQUIRE(call_id < (1u << 24), "svmc_fill_normals: call_id must fit 24 bits");
    if (n_path == 0 || nb_steps == 0) return SVMC_OK;
    hipLaunchKernelGGL(fill_normals_kernel, dim3(rng_grid(n_path)), dim3(rng_block()), 0, as_stream(stream), W0, W1, ldw,
                       n_path, nb_steps, seed, make_c3(call_id), path_offset, step_offset);
    return check_launch("svmc_fill_normals");
}

int svmc_fill_uniforms(double *U, size_t ldw, size_t n_path, int nb_steps, uint64_t seed, uint32_t call_id,
                       uint64_t path_offset, uint32_t step_offset, svmc_stream_t stream)
{
    SVMC_REQUIRE(U, "svmc_fill_uniforms: null output");
    SVMC_REQUIRE(ldw >= n_path && nb_steps >= 0, "svmc_fill_uniforms: ldw < n_path or nb_steps < 0");
    SVMC_REQUIRE(call_id < (1u << 24), "svmc_fill_uniforms: call_id must fit 24 bits");
    if (n_path == 0 || nb_steps == 0) return SVMC_OK;
    hipLaunchKernelGGL(fill_uniforms_kernel, dim3(grid_for(n_path)), dim3(BLOCK), 0, as_stream(stream), U, ldw,
                       n_path, nb_steps, seed, make_c3(call_id), path_offset, step_offset);
    return check_launch("svmc_fill_uniforms");
}

static int logsv_rng_launch(const char *fn, double *x, double *sigma, double *qvar, size_t n_path, int nb_steps,
                            double dt, double theta, double kappa1, double kappa2, double beta, double volvol,
                            double vol_backbone_eta, int is_spot_measure, uint64_t seed, uint32_t call_id,
                            uint64_t path_offset, uint32_t step_offset, const SliceOut &so, svmc_stream_t stream,
                            const StateInit &init = StateInit())
{
    if (int rc = check_state(fn, x, sigma, qvar, nb_steps, dt)) return rc;
    if (call_id >= (1u << 24)) return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": call_id must fit 24 bits");
    if (n_path == 0) return SVMC_OK;
    LogsvFast c = logsv_fast_in_log_units(make_logsv_fast(
        make_logsv_consts(dt, theta, kappa1, kappa2, beta, volvol, vol_backbone_eta, is_spot_measure)));
    if (const LogsvLatVariant *v = logsv_lat_variant(n_path))
        hipLaunchKernelGGL(v->slice, dim3(lat_grid(n_path, v->block)), dim3(v->block), 0, as_stream(stream), x, sigma, qvar, n_path,
                           nb_steps, c, seed, make_c3(call_id), path_offset, step_offset, so, init, armed_probe());
    else
        hipLaunchKernelGGL(logsv_rng_kernel, dim3(rng_grid(n_path)), dim3(rng_block()), 0, as_stream(stream), x, sigma, qvar,
                           n_path, nb_steps, c, seed, make_c3(call_id), path_offset, step_offset, so, init, armed_probe());
    return check_launch(fn);
}

int svmc_logsv_terminal_rng(double *x, double *sigma, double *qvar, size_t n_path, int nb_steps, double dt,
                            double theta, double kappa1, double kappa2, double beta, double volvol,
                            double vol_backbone_eta, int is_spot_measure, uint64_t seed, uint32_t call_id,
                            uint64_t path_offset, uint32_t step_offset, svmc_stream_t stream)
{
    const SliceOut none = {nullptr, nullptr, nullptr, 0.0};
    return logsv_rng_launch("svmc_logsv_terminal_rng", x, sigma, qvar, n_path, nb_steps, dt, theta, kappa1, kappa2, beta,
                            volvol, vol_backbone_eta, is_spot_measure, seed, call_id, path_offset, step_offset, none,
                            stream);
}

}  // extern "C"

static int logsv_slice_rng_impl(const char *fn, const StateInit &init, double *x, double *sigma, double *qvar, size_t n_path, int nb_steps, double dt, double theta,
                         double kappa1, double kappa2, double beta, double volvol, double vol_backbone_eta,
                         int is_spot_measure, uint64_t seed, uint32_t call_id, uint64_t path_offset,
                         uint32_t step_offset, double forward, double *x_snapshot, double *qvar_snapshot,
                         double *spot_sums, void *workspace, size_t workspace_bytes, svmc_stream_t stream)
{
    if (int rc = check_slice_args(fn, n_path, x_snapshot, spot_sums, workspace, workspace_bytes, true)) return rc;
    SVMC_REQUIRE(n_path > 0 && nb_steps > 0, std::string(fn) + ": n_path and nb_steps must be positive");
    const SliceOut so = {x_snapshot, qvar_snapshot, static_cast<double *>(workspace), forward, wave_rows(n_path)};
    if (int rc = logsv_rng_launch(fn, x, sigma, qvar, n_path, nb_steps, dt, theta, kappa1, kappa2, beta, volvol,
                                  vol_backbone_eta, is_spot_measure, seed, call_id, path_offset, step_offset, so, stream, init))
        return rc;
    if (spot_sums == nullptr) return SVMC_OK;
    return reduce_spot_partials(workspace, n_path, 2, spot_sums, as_stream(stream));
}

extern "C" {

int svmc_logsv_slice_rng(double *x, double *sigma, double *qvar, size_t n_path, int nb_steps, double dt, double theta,
                         double kappa1, double kappa2, double beta, double volvol, double vol_backbone_eta,
                         int is_spot_measure, uint64_t seed, uint32_t call_id, uint64_t path_offset,
                         uint32_t step_offset, double forward, double *x_snapshot, double *qvar_snapshot,
                         double *spot_sums, void *workspace, size_t workspace_bytes, svmc_stream_t stream)
{
    SVMC_REQUIRE(spot_sums != nullptr, "svmc_logsv_slice_rng: null spot_sums");
    return logsv_slice_rng_impl("svmc_logsv_slice_rng", StateInit(), x, sigma, qvar, n_path, nb_steps, dt, theta, kappa1, kappa2,
                                beta, volvol, vol_backbone_eta, is_spot_measure, seed, call_id, path_offset, step_offset,
                                forward, x_snapshot, qvar_snapshot, spot_sums, workspace, workspace_bytes, stream);
}

int svmc_logsv_slice_rng_from(double x0, double sigma0, double qvar0, double *x, double *sigma, double *qvar, size_t n_path,
                              int nb_steps, double dt, double theta, double kappa1, double kappa2, double beta, double volvol,
                              double vol_backbone_eta, int is_spot_measure, uint64_t seed, uint32_t call_id,
                              uint64_t path_offset, uint32_t step_offset, double forward, double *x_snapshot,
                              double *qvar_snapshot, double *spot_sums, void *workspace, size_t workspace_bytes,
                              svmc_stream_t stream)
{
    SVMC_REQUIRE(spot_sums != nullptr, "svmc_logsv_slice_rng_from: null spot_sums");
    const StateInit init = {1, x0, sigma0, qvar0};
    return logsv_slice_rng_impl("svmc_logsv_slice_rng_from", init, x, sigma, qvar, n_path, nb_steps, dt, theta, kappa1, kappa2,
                                beta, volvol, vol_backbone_eta, is_spot_measure, seed, call_id, path_offset, step_offset,
                                forward, x_snapshot, qvar_snapshot, spot_sums, workspace, workspace_bytes, stream);
}

}  // extern "C"

static int logsv_chain_rng_impl(const char *fn, const StateInit &init, double *x, double *sigma, double *qvar, size_t n_path, int n_slices, const int *nb_steps_host,
                         const double *dts_host, const double *etas_host, const double *forwards_host, double theta,
                         double kappa1, double kappa2, double beta, double volvol, int is_spot_measure, uint64_t seed,
                         uint32_t call_id, uint64_t path_offset, uint32_t step_offset, double *x_snapshots,
                         double *qvar_snapshots, double *spot_sums, void *workspace, size_t workspace_bytes,
                         svmc_stream_t stream)
{
    const auto fill = [&](ChainSlices &cs, int i, int j) {
        cs.c[i] = logsv_fast_in_log_units(make_logsv_fast(make_logsv_consts(
            dts_host[j], theta, kappa1, kappa2, beta, volvol, etas_host ? etas_host[j] : 1.0, is_spot_measure)));
        cs.forward[i] = forwards_host[j];
        cs.total_steps += cs.nb_steps[i];
    };
    const auto launch = [&](const ChainSlices &cs, double *xs, double *qs, const StateInit &init_i, uint32_t step0) {
        double *const ws = static_cast<double *>(workspace);
        if (const LogsvLatVariant *v = logsv_lat_variant(n_path))
            hipLaunchKernelGGL(v->chain, dim3(lat_grid(n_path, v->block)), dim3(v->block), 0, as_stream(stream), x, sigma, qvar, n_path,
                               cs, seed, make_c3(call_id), path_offset, step0, xs, qs, ws, init_i, armed_probe());
        else
            hipLaunchKernelGGL(logsv_chain_rng_kernel, dim3(chain_grid(n_path)), dim3(CHAIN_BLOCK), 0, as_stream(stream), x, sigma, qvar,
                               n_path, cs, seed, make_c3(call_id), path_offset, step0, xs, qs, ws, init_i, armed_probe());
    };
    return step_chain<ChainSlices>(fn, init, x, sigma, qvar, n_path, n_slices, nb_steps_host, dts_host, forwards_host, call_id,
                                   step_offset, x_snapshots, qvar_snapshots, spot_sums, workspace, workspace_bytes, as_stream(stream),
                                   fill, launch);
}

extern "C" {

int svmc_logsv_chain_rng(double *x, double *sigma, double *qvar, size_t n_path, int n_slices, const int *nb_steps_host,
                         const double *dts_host, const double *etas_host, const double *forwards_host, double theta,
                         double kappa1, double kappa2, double beta, double volvol, int is_spot_measure, uint64_t seed,
                         uint32_t call_id, uint64_t path_offset, uint32_t step_offset, double *x_snapshots,
                         double *qvar_snapshots, double *spot_sums, void *workspace, size_t workspace_bytes,
                         svmc_stream_t stream)
{
    SVMC_REQUIRE(spot_sums != nullptr, "svmc_logsv_chain_rng: null spot_sums");
    return logsv_chain_rng_impl("svmc_logsv_chain_rng", StateInit(), x, sigma, qvar, n_path, n_slices, nb_steps_host, dts_host,
                                etas_host, forwards_host, theta, kappa1, kappa2, beta, volvol, is_spot_measure, seed, call_id,
                                path_offset, step_offset, x_snapshots, qvar_snapshots, spot_sums, workspace, workspace_bytes,
                                stream);
}

int svmc_logsv_chain_rng_from(double x0, double sigma0, double qvar0, double *x, double *sigma, double *qvar, size_t n_path,
                              int n_slices, const int *nb_steps_host, const double *dts_host, const double *etas_host,
                              const double *forwards_host, double theta, double kappa1, double kappa2, double beta,
                              double volvol, int is_spot_measure, uint64_t seed, uint32_t call_id, uint64_t path_offset,
                              uint32_t step_offset, double *x_snapshots, double *qvar_snapshots, double *spot_sums,
                              void *workspace, size_t workspace_bytes, svmc_stream_t stream)
{
    SVMC_REQUIRE(spot_sums != nullptr, "svmc_logsv_chain_rng_from: null spot_sums");
    const StateInit init = {1, x0, sigma0, qvar0};
    return logsv_chain_rng_impl("svmc_logsv_chain_rng_from", init, x, sigma, qvar, n_path, n_slices, nb_steps_host, dts_host,
                                etas_host, forwards_host, theta, kappa1, kappa2, beta, volvol, is_spot_measure, seed, call_id,
                                path_offset, step_offset, x_snapshots, qvar_snapshots, spot_sums, workspace, workspace_bytes,
                                stream);
}

static int logsv_w_launch(const char *fn, double *x, double *sigma, double *qvar, size_t n_path, int nb_steps, double dt,
                          double theta, double kappa1, double kappa2, double beta, double volvol,
                          double vol_backbone_eta, int is_spot_measure, const double *W0, const double *W1, size_t ldw,
                          const SliceOut &so, svmc_stream_t stream)
{
    if (int rc = check_state(fn, x, sigma, qvar, nb_steps, dt)) return rc;
    if (W0 == nullptr || W1 == nullptr) return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": null W0/W1");
    if (ldw < n_path) return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": ldw < n_path");
    if (n_path == 0 || (nb_steps == 0 && so.partials == nullptr)) return SVMC_OK;
    const LogsvConsts c = make_logsv_consts(dt, theta, kappa1, kappa2, beta, volvol, vol_backbone_eta, is_spot_measure);
    hipLaunchKernelGGL(logsv_w_kernel, dim3(grid_for(n_path)), dim3(BLOCK), 0, as_stream(stream), x, sigma, qvar,
                       n_path, nb_steps, c, W0, W1, ldw, so);
    return check_launch(fn);
}

int svmc_logsv_terminal_w(double *x, double *sigma, double *qvar, size_t n_path, int nb_steps, double dt,
                          double theta, double kappa1, double kappa2, double beta, double volvol,
                          double vol_backbone_eta, int is_spot_measure, const double *W0, const double *W1,
                          size_t ldw, svmc_stream_t stream)
{
    const SliceOut none = {nullptr, nullptr, nullptr, 0.0};
    return logsv_w_launch("svmc_logsv_terminal_w", x, sigma, qvar, n_path, nb_steps, dt, theta, kappa1, kappa2, beta,
                          volvol, vol_backbone_eta, is_spot_measure, W0, W1, ldw, none, stream);
}

int svmc_logsv_slice_w(double *x, double *sigma, double *qvar, size_t n_path, int nb_steps, double dt, double theta,
                       double kappa1, double kappa2, double beta, double volvol, double vol_backbone_eta,
                       int is_spot_measure, const double *W0, const double *W1, size_t ldw, double forward,
                       double *x_snapshot, double *qvar_snapshot, double *spot_sums, void *workspace,
                       size_t workspace_bytes, svmc_stream_t stream)
{
    const char *fn = "svmc_logsv_slice_w";
    if (int rc = check_slice_args(fn, n_path, x_snapshot, spot_sums, workspace, workspace_bytes)) return rc;
    SVMC_REQUIRE(n_path > 0 && nb_steps > 0, "svmc_logsv_slice_w: n_path and nb_steps must be positive");
    const SliceOut so = {x_snapshot, qvar_snapshot, static_cast<double *>(workspace), forward, wave_rows(n_path)};
    if (int rc = logsv_w_launch(fn, x, sigma, qvar, n_path, nb_steps, dt, theta, kappa1, kappa2, beta, volvol,
                                vol_backbone_eta, is_spot_measure, W0, W1, ldw, so, stream))
        return rc;
    return reduce_spot_partials(workspace, n_path, 2, spot_sums, as_stream(stream));
}

}  // extern "C"

namespace svmc {

// internal entry points of the graph-replayed chain driver (svmc_chain.hip); same checks as their C-ABI twins
int fill_state_indirect(double *x, double *vol, double *qvar, size_t n_path, const double *vol0_dev, hipStream_t stream)
{
    if (n_path == 0) return SVMC_OK;
    hipLaunchKernelGGL(fill_state_indirect_kernel, dim3(grid_for(n_path)), dim3(BLOCK), 0, stream, x, vol, qvar, n_path,
                       vol0_dev);
    return check_launch("fill_state_indirect");
}

int logsv_slice_w_indirect(double *x, double *sigma, double *qvar, size_t n_path, int nb_steps,
                           const double *consts_dev, const double *W0, const double *W1, size_t ldw, double forward,
                           double *x_snapshot, double *qvar_snapshot, double *spot_sums, void *workspace,
                           size_t workspace_bytes, hipStream_t stream)
{
    const char *fn = "logsv_slice_w_indirect";
    if (int rc = check_slice_args(fn, n_path, x_snapshot, spot_sums, workspace, workspace_bytes)) return rc;
    if (W0 == nullptr || W1 == nullptr || ldw < n_path || nb_steps <= 0 || n_path == 0)
        return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": bad randoms / sizes");
    const SliceOut so = {x_snapshot, qvar_snapshot, static_cast<double *>(workspace), forward, wave_rows(n_path)};
    hipLaunchKernelGGL(logsv_w_indirect_kernel, dim3(grid_for(n_path)), dim3(BLOCK), 0, stream, x, sigma, qvar, n_path,
                       nb_steps, reinterpret_cast<const LogsvConsts *>(consts_dev), W0, W1, ldw, so);
    if (int rc = check_launch(fn)) return rc;
    return reduce_spot_partials(workspace, n_path, 2, spot_sums, stream);
}

// every expiry of a chain on resident randoms in one launch + one column reduce (graph-replayed driver, svmc_chain.hip):
// consts_dev = [m] LogsvConsts, vol0_dev = the initial volatility (state is initialised in the kernel), x_snapshots [m][n],
// qvar_snapshots [m][n] or null, spot_sums [2m]
int logsv_chain_w_indirect(double *x, double *sigma, double *qvar, size_t n_path, int n_slices, const int *nb_steps_host,
                           const double *consts_dev, const double *vol0_dev, const double *const *W0s, const double *const *W1s,
                           size_t ldw, const double *forwards_host, double *x_snapshots, double *qvar_snapshots,
                           double *spot_sums, void *workspace, size_t workspace_bytes, hipStream_t stream)
{
    const char *fn = "logsv_chain_w_indirect";
    if (n_slices < 1 || n_slices > MAX_CHAIN_SLICES || n_path == 0 || ldw < n_path)
        return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": bad sizes");
    const unsigned g = grid_for(n_path);
    if (workspace_bytes < static_cast<size_t>(wave_rows(n_path)) * 2 * n_slices * sizeof(double))
        return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": workspace too small (svmc_slice_workspace_bytes)");
    ChainWSlices cs;
    cs.m = n_slices;
    for (int i = 0; i < MAX_CHAIN_SLICES; ++i) {
        const int j = (i < n_slices) ? i : 0;
        if (W0s[j] == nullptr || W1s[j] == nullptr || nb_steps_host[j] <= 0)
            return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": bad randoms / step counts");
        cs.W0[i] = W0s[j];
        cs.W1[i] = W1s[j];
        cs.forward[i] = forwards_host[j];
        cs.nb_steps[i] = (i < n_slices) ? nb_steps_host[j] : 0;
    }
    hipLaunchKernelGGL(logsv_chain_w_indirect_kernel, dim3(g), dim3(BLOCK), 0, stream, x, sigma, qvar, n_path, cs,
                       reinterpret_cast<const LogsvConsts *>(consts_dev), vol0_dev, ldw, x_snapshots, qvar_snapshots,
                       static_cast<double *>(workspace));
    reduce_columns(2 * n_slices, stream, static_cast<const double *>(workspace), wave_rows(n_path), size_t(1),
                   static_cast<size_t>(wave_rows(n_path)), spot_sums);
    return check_launch(fn);
}

// P parameter sets of a chain on resident randoms in one launch + one column reduce (svmc_logsv_chain_price_fixed_sets):
// consts_dev = [m][P] LogsvConsts, vol0_dev = [P]; snapshots [P m][n] set-major, spot_sums [P m][2]
template <int P>
static void launch_chain_w_sets(unsigned g, hipStream_t stream, size_t n_path, const ChainWSlices &cs, const double *consts_dev,
                                const double *vol0_dev, size_t ldw, double *x_snapshots, double *qvar_snapshots, void *workspace)
{
    hipLaunchKernelGGL(logsv_chain_w_sets_kernel<P>, dim3(g), dim3(BLOCK), 0, stream, n_path, cs,
                       reinterpret_cast<const LogsvConsts *>(consts_dev), vol0_dev, ldw, x_snapshots, qvar_snapshots,
                       static_cast<double *>(workspace));
}

int logsv_chain_w_sets(size_t n_path, int n_sets, int n_slices, const int *nb_steps_host, const double *consts_dev,
                       const double *vol0_dev, const double *const *W0s, const double *const *W1s, size_t ldw,
                       const double *forwards_host, double *x_snapshots, double *qvar_snapshots, double *spot_sums,
                       void *workspace, size_t workspace_bytes, hipStream_t stream)
{
    const char *fn = "logsv_chain_w_sets";
    if (n_slices < 1 || n_slices > MAX_CHAIN_SLICES || n_sets < 2 || n_sets > MAX_CHAIN_SETS || n_path == 0 || ldw < n_path)
        return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": bad sizes");
    const unsigned g = grid_for(n_path);
    const int cols = 2 * n_slices * n_sets;
    if (workspace_bytes < static_cast<size_t>(wave_rows(n_path)) * cols * sizeof(double))
        return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": workspace too small (svmc_slice_workspace_bytes)");
    ChainWSlices cs;
    cs.m = n_slices;
    for (int i = 0; i < MAX_CHAIN_SLICES; ++i) {
        const int j = (i < n_slices) ? i : 0;
        if (W0s[j] == nullptr || W1s[j] == nullptr || nb_steps_host[j] <= 0)
            return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": bad randoms / step counts");
        cs.W0[i] = W0s[j];
        cs.W1[i] = W1s[j];
        cs.forward[i] = forwards_host[j];
        cs.nb_steps[i] = (i < n_slices) ? nb_steps_host[j] : 0;
    }
    switch (n_sets) {
    case 2: launch_chain_w_sets<2>(g, stream, n_path, cs, consts_dev, vol0_dev, ldw, x_snapshots, qvar_snapshots, workspace); break;
    case 3: launch_chain_w_sets<3>(g, stream, n_path, cs, consts_dev, vol0_dev, ldw, x_snapshots, qvar_snapshots, workspace); break;
    case 4: launch_chain_w_sets<4>(g, stream, n_path, cs, consts_dev, vol0_dev, ldw, x_snapshots, qvar_snapshots, workspace); break;
    case 5: launch_chain_w_sets<5>(g, stream, n_path, cs, consts_dev, vol0_dev, ldw, x_snapshots, qvar_snapshots, workspace); break;
    case 6: launch_chain_w_sets<6>(g, stream, n_path, cs, consts_dev, vol0_dev, ldw, x_snapshots, qvar_snapshots, workspace); break;
    case 7: launch_chain_w_sets<7>(g, stream, n_path, cs, consts_dev, vol0_dev, ldw, x_snapshots, qvar_snapshots, workspace); break;
    default: launch_chain_w_sets<8>(g, stream, n_path, cs, consts_dev, vol0_dev, ldw, x_snapshots, qvar_snapshots, workspace); break;
    }
    reduce_columns(cols, stream, static_cast<const double *>(workspace), wave_rows(n_path), size_t(1),
                   static_cast<size_t>(wave_rows(n_path)), spot_sums);
    return check_launch(fn);
}

// P parameter sets of a chain on randoms regenerated from (seed, call_id) in one launch + one column reduce
// (svmc_logsv_chain_price_frozen_sets): consts_dev = [m][P] LogsvFast in log units (logsv_fast_to_doubles), vol0_dev = [P];
// snapshots [P m][n] set-major, spot_sums [P m][2]
template <int P>
static void launch_chain_rng_sets(unsigned g, hipStream_t stream, size_t n_path, const ChainRngSetsSlices &cs,
                                  const double *consts_dev, const double *vol0_dev, int p_total, int s0, uint64_t seed,
                                  uint32_t c3, uint64_t path_offset, double *x_snapshots, double *qvar_snapshots, void *workspace,
                                  uint64_t *probe)
{
    hipLaunchKernelGGL(logsv_chain_rng_sets_kernel<P>, dim3(g), dim3(BLOCK), 0, stream, n_path, cs,
                       reinterpret_cast<const LogsvFast *>(consts_dev), vol0_dev, p_total, s0, seed, c3, path_offset, 0u,
                       x_snapshots, qvar_snapshots, static_cast<double *>(workspace), probe);
}

int logsv_chain_rng_sets(size_t n_path, int n_sets, int n_slices, const int *nb_steps_host, const double *consts_dev,
                         const double *vol0_dev, const double *forwards_host, uint64_t seed, uint32_t call_id,
                         uint64_t path_offset, double *x_snapshots, double *qvar_snapshots, double *spot_sums, void *workspace,
                         size_t workspace_bytes, hipStream_t stream, bool allow_probe)
{
    const char *fn = "logsv_chain_rng_sets";
    if (n_slices < 1 || n_slices > MAX_CHAIN_SLICES || n_sets < 1 || n_sets > MAX_CHAIN_SETS || n_path == 0)
        return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": bad sizes");
    if (call_id >= (1u << 24)) return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": call_id must fit 24 bits");
    const int cols = 2 * n_slices * n_sets;
    if (workspace_bytes < static_cast<size_t>(wave_rows(n_path)) * cols * sizeof(double))
        return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": workspace too small (svmc_slice_workspace_bytes)");
    ChainRngSetsSlices cs;
    cs.m = n_slices;
    for (int i = 0; i < MAX_CHAIN_SLICES; ++i) {
        const int j = (i < n_slices) ? i : 0;
        if (nb_steps_host[j] <= 0) return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": bad step counts");
        cs.forward[i] = forwards_host[j];
        cs.nb_steps[i] = (i < n_slices) ? nb_steps_host[j] : 0;
    }
    const uint32_t c3 = make_c3(call_id);
    const unsigned g = grid_for(n_path);
    uint64_t *probe = allow_probe ? armed_probe() : nullptr;
#define SVMC_RNG_SETS_CASE(P, S0)                                                                                               \
    launch_chain_rng_sets<P>(g, stream, n_path, cs, consts_dev, vol0_dev, n_sets, S0, seed, c3, path_offset, x_snapshots,       \
                             qvar_snapshots, workspace, probe)
    switch (n_sets) {
    case 1: SVMC_RNG_SETS_CASE(1, 0); break;
    case 2: SVMC_RNG_SETS_CASE(2, 0); break;
    case 3: SVMC_RNG_SETS_CASE(3, 0); break;
    case 4: SVMC_RNG_SETS_CASE(4, 0); break;
    case 5: SVMC_RNG_SETS_CASE(5, 0); break;
    case 6: SVMC_RNG_SETS_CASE(6, 0); break;
    case 7: SVMC_RNG_SETS_CASE(7, 0); break;
    default:                                   // eight: two launches of four (register budget, see the kernel)
        SVMC_RNG_SETS_CASE(4, 0);
        SVMC_RNG_SETS_CASE(4, 4);
        break;
    }
#undef SVMC_RNG_SETS_CASE
    if (spot_sums != nullptr)                  // (null: the caller's payoff kernel sums the partial columns itself)
        reduce_columns(cols, stream, static_cast<const double *>(workspace), wave_rows(n_path), size_t(1),
                       static_cast<size_t>(wave_rows(n_path)), spot_sums);
    return check_launch(fn);
}

// the constants of one (slice, set) pair as the generators take them: LogsvFast in log units (what logsv_rng_launch passes)
void logsv_fast_to_doubles(double dt, double theta, double kappa1, double kappa2, double beta, double volvol, double eta,
                           int is_spot_measure, double *out)
{
    const LogsvFast c = logsv_fast_in_log_units(make_logsv_fast(make_logsv_consts(dt, theta, kappa1, kappa2, beta, volvol, eta, is_spot_measure)));
    static_assert(sizeof(LogsvFast) == LOGSV_FAST_CONSTS_DOUBLES * sizeof(double), "LogsvFast layout");
    memcpy(out, &c, sizeof(c));
}

// The price -> implied-vol step of a calibration objective on the device, where the payoff sums already are: one lane per
// quote finalises its price (utils/mc_payoffs.py:85-88) and inverts Black-76 (svmc_black.h, the host routine's solver).
// quotes[k] = {strike, payoff code, shift, forward, ttm, discfactor}: fixed for a chain, uploaded once by the caller.
constexpr int IV_QUOTE_DOUBLES = 6;
__global__ __launch_bounds__(64) void chain_implied_vols_kernel(const double *__restrict__ sums, const double *__restrict__ quotes,
                                                               size_t n_quotes, double n_path_total, double vol_lo,
                                                               double vol_hi, double *__restrict__ ivols,
                                                               double *__restrict__ sums_copy)
{
    const size_t k = static_cast<size_t>(blockIdx.x) * 64 + threadIdx.x;
    if (k >= n_quotes) return;
    const double *qd = quotes + IV_QUOTE_DOUBLES * k;
    double price, se;
    const double s0 = sums[3 * k], s1 = sums[3 * k + 1], s2 = sums[3 * k + 2];
    if (sums_copy != nullptr) {         // the caller's pinned host buffer: the sums go home from here, not by a copy node
        sums_copy[3 * k] = s0;
        sums_copy[3 * k + 1] = s1;
        sums_copy[3 * k + 2] = s2;
    }
    payoff_finalize_one(s0, s1, s2, qd[2], qd[5], n_path_total, &price, &se);
    const int code = static_cast<int>(qd[1]);
    // inverse quotes (IC / IP): the Black-76 value of (S - K)^+ / S is the vanilla value over the forward
    const bool call = code == SVMC_CALL || code == SVMC_INV_CALL;
    ivols[k] = black_implied_vol(code >= SVMC_INV_CALL ? price * qd[3] : price, qd[0], call, qd[3], qd[4], qd[5], vol_lo, vol_hi);
}

int chain_implied_vols(const double *sums_dev, const double *quotes_dev, size_t n_quotes, double n_path_total, double vol_lo,
                       double vol_hi, double *ivols_out, double *sums_copy, hipStream_t stream)
{
    if (n_quotes == 0) return SVMC_OK;
    hipLaunchKernelGGL(chain_implied_vols_kernel, dim3(static_cast<unsigned>((n_quotes + 63) / 64)), dim3(64), 0, stream, sums_dev,
                       quotes_dev, n_quotes, n_path_total, vol_lo, vol_hi, ivols_out, sums_copy);
    return check_launch("chain_implied_vols");
}

void logsv_consts_to_doubles(double dt, double theta, double kappa1, double kappa2, double beta, double volvol, double eta,
                             int is_spot_measure, double *out)
{
    const LogsvConsts c = make_logsv_consts(dt, theta, kappa1, kappa2, beta, volvol, eta, is_spot_measure);
    static_assert(sizeof(LogsvConsts) == LOGSV_CONSTS_DOUBLES * sizeof(double), "LogsvConsts layout");
    memcpy(out, &c, sizeof(c));
}

}  // namespace svmc

extern "C" {

int svmc_logsv_vol_paths(double *sigma_t, size_t ld, size_t n_path, int nb_steps, double dt, double v0, double theta,
                         double kappa1, double kappa2, double beta, double volvol, int is_spot_measure,
                         const double *brownians, size_t ldb, uint64_t seed, uint32_t call_id, uint64_t path_offset,
                         svmc_stream_t stream)
{
    SVMC_REQUIRE(sigma_t != nullptr, "svmc_logsv_vol_paths: null output");
    SVMC_REQUIRE(nb_steps >= 0 && dt > 0.0 && ld >= n_path, "svmc_logsv_vol_paths: bad nb_steps/dt/ld");
    SVMC_REQUIRE(brownians == nullptr || ldb >= n_path, "svmc_logsv_vol_paths: ldb < n_path");
    SVMC_REQUIRE(call_id < (1u << 24), "svmc_logsv_vol_paths: call_id must fit 24 bits");
    if (n_path == 0) return SVMC_OK;
    const double adj = is_spot_measure ? 0.0 : beta;                                            // :930-933
    const double vartheta2 = beta * beta + volvol * volvol;
    const double K = LOG_UNITS_PER_NAT;
    VolPathConsts c;
    c.c1 = kappa1 * theta * dt * K;
    c.c2 = (adj - kappa2) * dt * K;
    c.c3 = (kappa2 * theta - kappa1 - 0.5 * vartheta2) * dt * K;
    c.cz = sqrt(vartheta2) * K * (brownians != nullptr ? 1.0 : sqrt(dt));
    c.L0 = log(v0) * K;
    if (brownians != nullptr)
        hipLaunchKernelGGL(logsv_vol_paths_kernel<false>, dim3(grid_for(n_path)), dim3(BLOCK), 0, as_stream(stream),
                           sigma_t, ld, n_path, nb_steps, v0, c, brownians, ldb, seed, make_c3(call_id), path_offset, armed_probe());
    else
        hipLaunchKernelGGL(logsv_vol_paths_kernel<true>, dim3(static_cast<unsigned>((n_path + VOLPATHS_RNG_BLOCK - 1) / VOLPATHS_RNG_BLOCK)),
                           dim3(VOLPATHS_RNG_BLOCK), 0, as_stream(stream), sigma_t, ld, n_path, nb_steps, v0, c, brownians, ldb,
                           seed, make_c3(call_id), path_offset, armed_probe());
    return check_launch("svmc_logsv_vol_paths");
}

int svmc_row_power_sums(const double *a, size_t ld, size_t n_rows, size_t n_cols, double center, int n_moments,
                        double *sums, void *workspace, size_t workspace_bytes, svmc_stream_t stream)
{
    SVMC_REQUIRE(a != nullptr && sums != nullptr && workspace != nullptr, "svmc_row_power_sums: null pointer");
    SVMC_REQUIRE(n_moments >= 1 && n_moments <= ROW_MOMENTS_MAX, "svmc_row_power_sums: 1 <= n_moments <= 4");
    SVMC_REQUIRE(ld >= n_cols && n_cols > 0, "svmc_row_power_sums: ld < n_cols or no columns");
    SVMC_REQUIRE(n_rows < (1u << 30), "svmc_row_power_sums: too many rows");
    if (n_rows == 0) return SVMC_OK;
    const size_t need = n_rows * ROW_SEGMENTS * 2 * static_cast<size_t>(n_moments) * sizeof(double);
    if (workspace_bytes < need) return fail(SVMC_ERR_WORKSPACE, "svmc_row_power_sums: workspace too small (rows x 4 x 2 n_moments doubles)");
    double *partials = static_cast<double *>(workspace);
    const dim3 grid(static_cast<unsigned>(n_rows), ROW_SEGMENTS);
    switch (n_moments) {
    case 1: hipLaunchKernelGGL(row_power_sums_kernel<1>, grid, dim3(BLOCK), 0, as_stream(stream), a, ld, n_cols, center, partials); break;
    case 2: hipLaunchKernelGGL(row_power_sums_kernel<2>, grid, dim3(BLOCK), 0, as_stream(stream), a, ld, n_cols, center, partials); break;
    case 3: hipLaunchKernelGGL(row_power_sums_kernel<3>, grid, dim3(BLOCK), 0, as_stream(stream), a, ld, n_cols, center, partials); break;
    default: hipLaunchKernelGGL(row_power_sums_kernel<4>, grid, dim3(BLOCK), 0, as_stream(stream), a, ld, n_cols, center, partials); break;
    }
    // sums[row][j] = the four segments' partials added in segment order: partials is [rows x 2K outputs][4 addends] read as a
    // matrix whose "rows" are the addends -- element (r, c) at partials[r * 2K + c * 4 * 2K] would interleave; the layout
    // [row][seg][j] makes output (row, j) the column sum over seg with row stride 2K and column base row * 4 * 2K + j
    const int K2 = 2 * n_moments;
    for (int j = 0; j < K2; ++j)
        reduce_columns(static_cast<unsigned>(n_rows), as_stream(stream), partials + j, static_cast<unsigned>(ROW_SEGMENTS),
                       static_cast<size_t>(K2), static_cast<size_t>(ROW_SEGMENTS) * K2, sums + static_cast<size_t>(j) * n_rows);
    return check_launch("svmc_row_power_sums");
}

int svmc_expanding_mean_squares(const double *a, size_t ld, size_t n_rows, size_t n_cols, double *out, size_t ldo,
                                svmc_stream_t stream)
{
    SVMC_REQUIRE(a != nullptr && out != nullptr, "svmc_expanding_mean_squares: null pointer");
    SVMC_REQUIRE(ld >= n_cols && ldo >= n_cols, "svmc_expanding_mean_squares: leading dimension < n_cols");
    if (n_rows == 0 || n_cols == 0) return SVMC_OK;
    // two columns per lane (16-byte accesses) where the layout allows it: even column count and leading dimensions, 16-byte bases
    const bool pair = (n_cols % 2 == 0) && (ld % 2 == 0) && (ldo % 2 == 0) && (reinterpret_cast<uintptr_t>(a) % 16 == 0) &&
                      (reinterpret_cast<uintptr_t>(out) % 16 == 0);
    if (pair)
        hipLaunchKernelGGL(expanding_mean_sq_kernel<true>, dim3(grid_for(n_cols / 2)), dim3(BLOCK), 0, as_stream(stream), a, ld, n_rows,
                           n_cols, out, ldo);
    else
        hipLaunchKernelGGL(expanding_mean_sq_kernel<false>, dim3(grid_for(n_cols)), dim3(BLOCK), 0, as_stream(stream), a, ld, n_rows,
                           n_cols, out, ldo);
    return check_launch("svmc_expanding_mean_squares");
}

int svmc_clock_probe_arm(int enable)
{
    uint64_t *&p = armed_probe();
    if (enable && p == nullptr) {
        SVMC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&p), 8 * sizeof(uint64_t)));
        SVMC_HIP_TRY(hipMemset(p, 0, 8 * sizeof(uint64_t)));
    } else if (!enable && p != nullptr) {
        SVMC_HIP_TRY(hipDeviceSynchronize());               // no launch that still stamps it
        (void)hipFree(p);
        p = nullptr;
    }
    return SVMC_OK;
}

int svmc_clock_probe_read(uint64_t *stamps, svmc_stream_t stream)
{
    SVMC_REQUIRE(stamps != nullptr, "svmc_clock_probe_read: null output");
    SVMC_REQUIRE(armed_probe() != nullptr, "svmc_clock_probe_read: this thread has not armed the probe (svmc_clock_probe_arm)");
    SVMC_HIP_TRY(hipStreamSynchronize(as_stream(stream)));
    SVMC_HIP_TRY(hipMemcpy(stamps, armed_probe(), 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return SVMC_OK;
}

int svmc_payoff_workspace_bytes(size_t *bytes)
{
    SVMC_REQUIRE(bytes != nullptr, "svmc_payoff_workspace_bytes: null output");
    *bytes = static_cast<size_t>(MAX_REDUCE_GRID) * 3 * PAYOFF_KT * PAYOFF_GROUPS * sizeof(double);
    return SVMC_OK;
}

int svmc_slice_workspace_bytes(size_t n_path, size_t *bytes)
{
    SVMC_REQUIRE(bytes != nullptr, "svmc_slice_workspace_bytes: null output");
    const size_t fused = static_cast<size_t>(wave_rows(n_path)) * 2 * MAX_CHAIN_SLICES * sizeof(double);
    const size_t payoff = static_cast<size_t>(MAX_REDUCE_GRID) * 3 * PAYOFF_KT * PAYOFF_GROUPS * sizeof(double);
    *bytes = fused > payoff ? fused : payoff;
    return SVMC_OK;
}

int svmc_spot_sums(const double *x, size_t n_path, double forward, double *spot_sums, void *workspace,
                   size_t workspace_bytes, svmc_stream_t stream)
{
    SVMC_REQUIRE(x && spot_sums && workspace, "svmc_spot_sums: null pointer");
    const unsigned g = reduce_grid(n_path);
    if (workspace_bytes < static_cast<size_t>(g) * 2 * sizeof(double))
        return fail(SVMC_ERR_WORKSPACE, "svmc_spot_sums: workspace too small (svmc_payoff_workspace_bytes)");
    double *partials = static_cast<double *>(workspace);
    hipLaunchKernelGGL(spot_sums_kernel, dim3(g), dim3(BLOCK), 0, as_stream(stream), x, n_path, forward, partials);
    reduce_columns(2, as_stream(stream), partials, g, size_t(2), size_t(1), spot_sums);
    return check_launch("svmc_spot_sums");
}

}  // extern "C"

// the launches of svmc_payoff_sums / svmc_payoff_sums_chain: groups of <= PAYOFF_KT strikes of one expiry, <= PAYOFF_GROUPS
// groups per launch, every launch followed by its column reduce
// one kernel per group width: a chain's 21 (or 13) strikes per expiry are worked on as 21, not as the next multiple of 8
using PayoffKernel = void (*)(PayoffGroupPack, size_t, double *, int, PayoffSetStrides);
template <bool HAS_INV, bool NEED_Q, int... KS>
static PayoffKernel payoff_kernel_for(int kt, std::integer_sequence<int, KS...>)
{
    static const PayoffKernel table[] = {payoff_group_kernel<KS + 1, HAS_INV, NEED_Q>...};
    return table[kt - 1];
}
constexpr int PAYOFF_KT_INV = 16;      // inverse chains: three accumulators per strike, 24 would leave one wave per SIMD

// path blocks per strike group of a payoff launch: about a thousand blocks per launch in all (512 are resident at the kernel's
// two waves per SIMD) -- more groups, fewer and longer-running blocks each, so that a block's set-up (its constants) and
// wind-down (the 48-value block reduction) are amortised over more paths (C3's 4 groups: 118 -> 108 us) -- and no block with
// fewer than PAYOFF_MIN_TRIPS paths per lane: at a calibration's 10^5 paths 256 blocks per group made 1.5 trips each and the
// launch was set-up and wind-down only (4 groups 9.1 us; x 7 parameter sets 39 us).  A function of the path count and the
// group count alone -- never of the number of parameter sets -- so that every route adds the same partial sums.
#ifndef SVMC_PAYOFF_MIN_TRIPS
#define SVMC_PAYOFF_MIN_TRIPS 4
#endif
static inline unsigned payoff_path_blocks(size_t n_path, int n_groups)
{
    const unsigned g = reduce_grid(n_path);
    unsigned gx = (PAYOFF_BLOCKS + static_cast<unsigned>(n_groups) - 1u) / static_cast<unsigned>(n_groups);
    gx = (gx < 128u) ? 128u : gx;
    gx = (gx > g) ? g : gx;
    const size_t cap = (n_path + static_cast<size_t>(BLOCK) * SVMC_PAYOFF_MIN_TRIPS - 1) / (static_cast<size_t>(BLOCK) * SVMC_PAYOFF_MIN_TRIPS);
    if (cap < gx) gx = static_cast<unsigned>(cap < 1 ? 1 : cap);
    return gx;
}

template <bool HAS_INV>
static void launch_payoff_groups(int kt, dim3 grid, hipStream_t st, const PayoffGroupPack &pack, size_t n, int variable_type,
                                 double *partials, int ld, const PayoffSetStrides &sets)
{
    constexpr auto widths = std::make_integer_sequence<int, HAS_INV ? PAYOFF_KT_INV : PAYOFF_KT>();
    const PayoffKernel kern = (variable_type == SVMC_Q_VAR) ? payoff_kernel_for<HAS_INV, true>(kt, widths)
                                                            : payoff_kernel_for<HAS_INV, false>(kt, widths);
    hipLaunchKernelGGL(kern, grid, dim3(BLOCK), 0, st, pack, n, partials, ld, sets);
}

// spot_partials != null (one-set launches): the expiries' spot sums are formed inside the payoff kernel from the generators' per-wave
// partial columns (expiry i's pair 2 spot_rows i doubles in) -- no reduce launch ahead of this one, and
// spot_sums (nullable then) is only written.  partials_out != null: NO column reduce either -- the chain must fit one launch
// (payoff_sets_fit) and the caller ends it with chain_finish (one wave per quote: the column sums, the prices' implied vols,
// everything stored where the host reads it).
struct PayoffPartialsOut {
    unsigned rows = 0;      // path blocks of the launch = rows of the partials
    int cols = 0;           // strike columns per set
};
static int payoff_sums_impl(const char *fn, const double *const *xs, const double *const *qs, size_t n_path,
                            const double *forwards, const double *ttms, const double *spot_sums, int n_expiries,
                            const double *strikes, const int8_t *types, const double *shifts, const size_t *offsets,
                            int variable_type, double *sums, void *workspace, size_t workspace_bytes, svmc_stream_t stream,
                            int n_sets = 1, const PayoffSetStrides &sets = PayoffSetStrides{0, 0, 0},
                            const double *spot_partials = nullptr, unsigned spot_rows = 0, PayoffPartialsOut *partials_out = nullptr)
{
    // n_sets > 1: xs / qs / spot_sums / sums are those of set 0 and the others lie `sets` (and 3 x total sums) further on; the
    // chain must then fit ONE launch (payoff_sets_fit), whose path blocks are those of a one-set launch -- the same partial
    // sums added in the same order, hence the bits of n_sets calls
    const size_t total = offsets[n_expiries];
    if (spot_partials != nullptr && n_sets != 1)
        return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": spot sums inside the payoff kernel are for one-set launches");
    bool any_inv = false;
    for (size_t k = 0; k < total; ++k) {
        if (types[k] < SVMC_CALL || types[k] > SVMC_INV_PUT)
            return fail(SVMC_ERR_UNKNOWN_PAYOFF, "unknown option payoff code");
        any_inv = any_inv || types[k] >= SVMC_INV_CALL;
    }
    // strikes per group: 24 for plain chains (two accumulators per strike); 16 when the chain holds inverse options
    // (three accumulators per strike: 24 of them would leave one wave per SIMD)
    const size_t KG = any_inv ? PAYOFF_KT_INV : PAYOFF_KT;
    const unsigned g = reduce_grid(n_path);
    if (workspace_bytes < static_cast<size_t>(g) * 3 * PAYOFF_KT * PAYOFF_GROUPS * sizeof(double))
        return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": workspace too small (svmc_payoff_workspace_bytes)");
    if (n_path == 0 || total == 0) return SVMC_OK;
    double *partials = static_cast<double *>(workspace);
    PayoffGroupPack pack;
    memset(&pack, 0, sizeof(pack));
    int n_groups = 0, cols = 0, kt = 0;         // groups, strike columns and widest group of the pending launch
    size_t first_strike = 0;                    // global index of the pending launch's first strike
    bool has_inv = false;
    auto flush = [&]() -> int {
        if (n_groups == 0) return SVMC_OK;
        const unsigned gx = payoff_path_blocks(n_path, n_groups);
        const dim3 grid(gx, static_cast<unsigned>(n_groups), static_cast<unsigned>(n_sets));
        if (n_sets > 1 && (first_strike != 0 || static_cast<size_t>(cols) != total ||
                           static_cast<size_t>(gx) * n_sets * 3 * cols * sizeof(double) > workspace_bytes))
            return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": the parameter sets do not fit one payoff launch");
        if (partials_out != nullptr && (first_strike != 0 || static_cast<size_t>(cols) != total))
            return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": the chain does not fit one payoff launch");
        if (has_inv)
            launch_payoff_groups<true>(kt, grid, as_stream(stream), pack, n_path, variable_type, partials, 3 * cols, sets);
        else
            launch_payoff_groups<false>(kt, grid, as_stream(stream), pack, n_path, variable_type, partials, 3 * cols, sets);
        if (partials_out != nullptr) {
            partials_out->rows = gx;
            partials_out->cols = cols;
        } else {
            reduce_columns(3 * cols * n_sets, as_stream(stream), partials, static_cast<unsigned>(gx),
                           static_cast<size_t>(3 * cols) * n_sets, size_t(1), sums + 3 * first_strike);
        }
        first_strike += static_cast<size_t>(cols);
        n_groups = cols = kt = 0;
        has_inv = false;
        return check_launch(fn);
    };
    for (int i = 0; i < n_expiries; ++i) {
        if (xs[i] == nullptr) return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": null snapshot");
        for (size_t k0 = offsets[i]; k0 < offsets[i + 1]; k0 += KG) {
            PayoffGroup &d = pack.g[n_groups];
            d.x = xs[i];
            d.qvar = (variable_type == SVMC_Q_VAR) ? qs[i] : nullptr;
            d.spot_sums = spot_sums ? spot_sums + 2 * i : nullptr;
            d.spot_partials = spot_partials ? spot_partials + 2 * static_cast<size_t>(spot_rows) * i : nullptr;
            d.spot_rows = spot_rows;
            d.forward = forwards[i];
            d.ttm = ttms[i];
            const size_t left = offsets[i + 1] - k0;
            d.k = static_cast<int>(left < KG ? left : KG);
            d.col = cols;
            d.inv_mask = 0u;
            d.put_mask = 0u;
            for (int k = 0; k < PAYOFF_KT; ++k) {
                const bool on = k < d.k;
                const int ty = on ? types[k0 + k] : SVMC_CALL;
                const double sgn = (ty == SVMC_CALL || ty == SVMC_INV_CALL) ? 1.0 : -1.0;
                if (sgn < 0.0) d.put_mask |= 1u << k;
                d.c[k] = on ? -sgn * strikes[k0 + k] : -__builtin_huge_val();      // unused: pay = max(u - inf, 0) = 0
                d.shift[k] = (on && shifts != nullptr) ? shifts[k0 + k] : 0.0;
                if (on && (ty == SVMC_INV_CALL || ty == SVMC_INV_PUT)) d.inv_mask |= 1u << k;
            }
            has_inv = has_inv || d.inv_mask != 0u;
            cols += d.k;
            kt = (d.k > kt) ? d.k : kt;
            if (++n_groups == PAYOFF_GROUPS)
                if (int rc = flush()) return rc;
        }
    }
    return flush();
}

namespace svmc {

// whether payoff_sums_chain_sets can take this chain: all its strike groups in one launch, the sets' partials in the workspace
bool payoff_sets_fit(size_t n_path, int n_expiries, const size_t *offsets, const int8_t *types, int n_sets, size_t workspace_bytes)
{
    const size_t total = offsets[n_expiries];
    if (n_path == 0 || total == 0 || n_sets < 1 || n_sets > 65535) return false;
    bool any_inv = false;
    for (size_t k = 0; k < total; ++k) any_inv = any_inv || types[k] >= SVMC_INV_CALL;
    const size_t KG = any_inv ? PAYOFF_KT_INV : PAYOFF_KT;
    size_t n_groups = 0;
    for (int i = 0; i < n_expiries; ++i) n_groups += (offsets[i + 1] - offsets[i] + KG - 1) / KG;
    if (n_groups == 0 || n_groups > static_cast<size_t>(PAYOFF_GROUPS)) return false;
    const unsigned g = reduce_grid(n_path), gx = payoff_path_blocks(n_path, static_cast<int>(n_groups));
    return static_cast<size_t>(gx) * n_sets * 3 * total * sizeof(double) <= workspace_bytes &&
           static_cast<size_t>(g) * 3 * PAYOFF_KT * PAYOFF_GROUPS * sizeof(double) <= workspace_bytes;
}

// svmc_payoff_sums_chain for n_sets parameter sets at once: ONE payoff launch (blockIdx.z = set) and ONE column reduce
// instead of n_sets of each; sums[set][3 x total].  Bit-equal to n_sets calls of svmc_payoff_sums_chain.
int payoff_sums_chain_sets(const double *const *x_snapshots_host, const double *const *qvar_snapshots_host, size_t n_path,
                           const double *forwards_host, const double *ttms_host, const double *spot_sums, int n_expiries,
                           const double *strikes_host, const int8_t *types_host, const double *shifts_host,
                           const size_t *strike_offsets_host, int variable_type, double *sums, void *workspace,
                           size_t workspace_bytes, hipStream_t stream, int n_sets, size_t x_set_stride, size_t q_set_stride,
                           size_t spot_set_stride)
{
    return payoff_sums_impl("payoff_sums_chain_sets", x_snapshots_host, qvar_snapshots_host, n_path, forwards_host, ttms_host,
                            spot_sums, n_expiries, strikes_host, types_host, shifts_host, strike_offsets_host, variable_type, sums,
                            workspace, workspace_bytes, reinterpret_cast<svmc_stream_t>(stream), n_sets,
                            PayoffSetStrides{x_set_stride, q_set_stride, spot_set_stride});
}

// The tail of an on-device-RNG chain on ONE device (svmc_chain.hip, round 6): (1) the payoff launch -- with spot_partials, every
// block forms its expiry's spot sums itself from the generators' per-wave partial columns ([expiry][2][spot_rows]: one batched
// round trip of loads for up to 2048 rows), without, it reads spot_sums as ever; (2) chain_finish_kernel, a wave per quote: the
// three column sums of the quote in reduce_columns_kernel's order of additions (the same bits), stored at sums_out -- the
// caller's pinned host buffer: no copy node.  Measured (tools/r06/chain_call_breakdown.py, 4 x 13 chain): reduce 4.8 + payoff 5.0 +
// reduce 4.9 + copy 4.3 us at 2^16 paths became payoff 7.5 + finish 4.4.  What was measured and NOT kept: the spot sums inside
// the payoff kernel above 2048 rows (every block repeats two or three dependent round trips: payoff 10.2 -> 17.9 us at 2 x 10^5
// paths, more than the reduce launch it saves), the same tail for the calibration objective's parameter sets (payoff of seven
// sets 19 -> 31 us), and the implied vols inside the finish kernel (one lane of 52 waves on 13 CUs: 24.6 us against 5.0 + 12.2
// for reduce + chain_implied_vols_kernel, whose one wave inverts 64 quotes side by side) -- profiles/r06_frozen_trace.txt.
// The chain must fit one payoff launch (payoff_sets_fit).
// a virtual thread sums four rows: no payoff launch may produce more partial rows than that
static_assert(PAYOFF_BLOCKS <= 4u * BLOCK && MAX_REDUCE_GRID <= 4 * BLOCK, "chain_finish_kernel sums at most 4 x BLOCK rows");
__global__ __launch_bounds__(BLOCK) void chain_finish_kernel(const double *__restrict__ partials, unsigned n_rows, int cols,
                                                             double *__restrict__ sums_out)
{
    const size_t q = static_cast<size_t>(blockIdx.x) * (BLOCK / 64) + (threadIdx.x >> 6);        // this wave's quote
    if (q >= static_cast<size_t>(cols)) return;                                                 // (wave-uniform)
    const size_t ld = 3 * static_cast<size_t>(cols);         // partials[path block][3 x cols]: column 3 q + which
    // lane l plays the threads l, 64 + l, 128 + l, 192 + l of block_column_sum one after the other -- the same additions in the
    // same order, the same bits -- with the loads of all three columns (a payoff launch has at most 1024 path blocks: four rows
    // per virtual thread) in flight before the first addition: one round trip, not twelve
    const unsigned lane = threadIdx.x & 63u;
    double t[3][4][4], sm[3];
#pragma unroll
    for (int which = 0; which < 3; ++which)
#pragma unroll
        for (int vw = 0; vw < 4; ++vw) column_rows_load<4>(partials + 3 * q + which, vw * 64u + lane, n_rows, ld, t[which][vw]);
#pragma unroll
    for (int which = 0; which < 3; ++which) {
        double total = 0.0;
#pragma unroll
        for (int vw = 0; vw < 4; ++vw) {
            const double w = wave_sum(column_rows_add<4>(t[which][vw], vw * 64u + lane, n_rows));
            total = (vw == 0) ? w : total + w;
        }
        sm[which] = total;
    }
    if (lane != 0u) return;
    sums_out[3 * q] = sm[0];
    sums_out[3 * q + 1] = sm[1];
    sums_out[3 * q + 2] = sm[2];
}

int chain_payoff_and_finish(const double *const *x_snapshots_host, const double *const *qvar_snapshots_host, size_t n_path,
                            const double *forwards_host, const double *ttms_host, double *spot_sums, const double *spot_partials,
                            int n_expiries, const double *strikes_host, const int8_t *types_host, const double *shifts_host,
                            const size_t *strike_offsets_host, int variable_type, void *workspace, size_t workspace_bytes,
                            hipStream_t stream, double *sums_out)
{
    const char *fn = "chain_payoff_and_finish";
    const unsigned rows = wave_rows(n_path);
    PayoffPartialsOut po;
    if (int rc = payoff_sums_impl(fn, x_snapshots_host, qvar_snapshots_host, n_path, forwards_host, ttms_host, spot_sums, n_expiries,
                                  strikes_host, types_host, shifts_host, strike_offsets_host, variable_type, nullptr, workspace,
                                  workspace_bytes, reinterpret_cast<svmc_stream_t>(stream), 1, PayoffSetStrides{0, 0, 0}, spot_partials,
                                  rows, &po))
        return rc;
    if (po.cols == 0) return SVMC_OK;
    if (po.rows > 4u * BLOCK) return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": more path blocks than chain_finish_kernel sums");
    hipLaunchKernelGGL(chain_finish_kernel, dim3(static_cast<unsigned>((po.cols + BLOCK / 64 - 1) / (BLOCK / 64))), dim3(BLOCK), 0, stream,
                       static_cast<const double *>(workspace), po.rows, po.cols, sums_out);
    return check_launch(fn);
}

// ---------------------------------------------------------------------------------------------------
// Exponentially weighted payoff sums: Monte Carlo prices under the exponential risk-premia kernel (svmc_tilted_payoff_chain,
// include/svmc.h states the estimator and the keep rule).  payoff_group_kernel's sibling: a block column is a group of up to
// KT strikes of one expiry, blockIdx.z a gamma; a thread reads a path's x once, exponentiates it twice (spot, weight), applies
// the keep rule by zeroing the weight of a dropped path (no branch: a zero weight adds nothing to any sum) and adds, per strike,
// w d, (w d)^2 and w (w d) with d = payoff - shift -- the sums the ratio estimator's delta-method error is formed from without
// cancellation -- and per expiry the seven statistics columns below, shifted the same way (w - 1, spot - forward).  Sums are the
// payoff kernel's: per-block partials in the fixed tree order, partials[path block][gamma][column], no atomics.  The path blocks
// of a launch are a function of the path count ALONE (tilted_path_blocks), so that a gamma's and an expiry's sums are the same
// bits whatever else shares the launch.
// ---------------------------------------------------------------------------------------------------
constexpr int TILTED_KT = 22;          // strikes per group, as PAYOFF_KT
constexpr int TILTED_NSTAT = 7;        // [sum w, sum w^2, sum (w-1)^2, sum w ds, sum w^2 ds, sum (w ds)^2, kept], ds = spot - forward
constexpr int TILTED_STAT_COLS = 8;    // ... padded: the statistics columns of an expiry start at a multiple of 64 bytes
constexpr unsigned TILTED_BLOCKS = 512;        // path blocks at most: one resident round at the kernel's two waves per SIMD

struct TiltedGroup {
    const double *x, *spot_sums;       // spot_sums: [sum F exp(x), count] of the expiry for the recentring; null: corr = 0
    double forward;
    double c[TILTED_KT];               // -sg K - shift; -inf for the unused strikes of a group (d = 0)
    double nshift[TILTED_KT];          // -shift: d = max(sg spot - sg K, 0) - shift = max(fma(sg, spot, c), -shift)
    uint32_t put_mask;                 // bit k set: put, sg = -1
    int k;                             // live strikes in this group
    int col;                           // first strike column of the group within this launch
    int slot;                          // statistics columns of the group's expiry within this launch
    int expiry;                        // the expiry's index in the chain (output row of its statistics)
    int first;                         // the group that writes the statistics columns of its expiry in this launch
};
struct TiltedGroupPack {
    TiltedGroup g[PAYOFF_GROUPS];
};
struct TiltedGammas {
    double g[SVMC_TILTED_MAX_GAMMAS];
};
static_assert(sizeof(TiltedGroupPack) + sizeof(TiltedGammas) + 128 <= 4096, "the tilted descriptors travel in the kernel arguments");

// as payoff_min_waves: the widest groups whose build metadata shows no scratch at three waves per SIMD
constexpr int tilted_min_waves(int kt) { return kt <= 4 ? 3 : 2; }

template <int KT>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(tilted_min_waves(KT), tilted_min_waves(KT)))) void tilted_payoff_group_kernel(
    TiltedGroupPack pack, TiltedGammas gammas, size_t n, double *__restrict__ partials, int ld, int stats_col0)
{
    constexpr int NV = 3 * KT + TILTED_NSTAT;
    constexpr int NSUM = block_sum_padded(NV);
    __shared__ double lds[4 * NSUM];
    const TiltedGroup &d = pack.g[blockIdx.y];
    const double gamma = gammas.g[blockIdx.z];
    const double *__restrict__ x = d.x;
    const double forward = d.forward;
    const double corr = (d.spot_sums != nullptr) ? d.spot_sums[0] / d.spot_sums[1] - forward : 0.0;    // (block-uniform)
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    const int nk = d.k;
    double acc[NSUM], sg[KT], c[KT], nshift[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        sg[k] = ((d.put_mask >> k) & 1u) ? -1.0 : 1.0;     // stays wave-uniform: the scalar operand of the FMA
        c[k] = d.c[k];
        nshift[k] = d.nshift[k];
    }
#pragma unroll
    for (int j = 0; j < NSUM; ++j) acc[j] = 0.0;
    constexpr double INF = __builtin_huge_val();

    const auto add_path = [&](double xi) {
        double w = exp_full(gamma * xi);
        double spot = forward * exp_full(xi) - corr;
        const double ws = w * spot;
        // the keep rule: x, w^2 and (w spot)^2 all finite (a NaN fails every comparison)
        const bool keep = (fabs(xi) < INF) && (w * w < INF) && (ws * ws < INF);
        w = keep ? w : 0.0;
        spot = keep ? spot : 0.0;
        const double v = keep ? w - 1.0 : 0.0;
        const double wds = w * (spot - forward);
        acc[3 * KT] += w;
        acc[3 * KT + 1] = fma(w, w, acc[3 * KT + 1]);
        acc[3 * KT + 2] = fma(v, v, acc[3 * KT + 2]);
        acc[3 * KT + 3] += wds;
        acc[3 * KT + 4] = fma(w, wds, acc[3 * KT + 4]);
        acc[3 * KT + 5] = fma(wds, wds, acc[3 * KT + 5]);
        acc[3 * KT + 6] += keep ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            const double wd = w * fmax(fma(sg[k], spot, c[k]), nshift[k]);
            acc[k] += wd;
            acc[KT + k] = fma(wd, wd, acc[KT + k]);
            acc[2 * KT + k] = fma(w, wd, acc[2 * KT + k]);
        }
    };
    // the trips of payoff_group_kernel: the ones every lane of the block makes through the batched double buffer, the ragged last
    const size_t i0 = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x;
    const size_t block_last = static_cast<size_t>(blockIdx.x) * BLOCK + (BLOCK - 1);
    const int full_trips = (n > block_last) ? static_cast<int>((n - 1 - block_last) / stride + 1) : 0;     // block-uniform
    constexpr int PF = (KT > 16) ? 1 : PAYOFF_PREFETCH;        // 22 strikes: 66 accumulators; two trips of prefetch spilled 44 B per lane
    const double *const wsrc[1] = {x + i0};
    streamed_time_loop<1, PF>(wsrc, stride, full_trips, [&](const double(&v)[1]) { add_path(v[0]); });
    for (size_t i = i0 + static_cast<size_t>(full_trips) * stride; i < n; i += stride) add_path(x[i]);
    // row layout: [sum w d, sum (w d)^2, sum w^2 d] per strike at column 3 (col + k), the expiry's statistics from stats_col0 on
    double *row = partials + (static_cast<size_t>(blockIdx.x) * gridDim.z + blockIdx.z) * ld;
    const int col = d.col, slot = d.slot, first = d.first;
    block_sum_apply<NSUM>(acc, lds, NV, [&](int j, double t) {
        if (j < 3 * KT) {
            const int which = j / KT, k = j - which * KT;
            if (k < nk) row[3 * (col + k) + which] = t;
        } else if (first) {
            row[stats_col0 + TILTED_STAT_COLS * slot + (j - 3 * KT)] = t;
        }
    });
}

// the sums of NC columns by one wave, in block_column_sum's order of additions (chain_finish_kernel's way: lane l plays the
// threads l, 64 + l, 128 + l, 192 + l one after the other), the loads of all of them in flight before the first addition
template <int NC>
__device__ __forceinline__ void wave_column_sums(const double *__restrict__ first_col, unsigned n_rows, size_t ld, unsigned lane,
                                                 double (&out)[NC])
{
    double t[NC][4][4];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
#pragma unroll
        for (int vw = 0; vw < 4; ++vw) column_rows_load<4>(first_col + cc, vw * 64u + lane, n_rows, ld, t[cc][vw]);
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) {
        double total = 0.0;
#pragma unroll
        for (int vw = 0; vw < 4; ++vw) {
            const double w = wave_sum(column_rows_add<4>(t[cc][vw], vw * 64u + lane, n_rows));
            total = (vw == 0) ? w : total + w;
        }
        out[cc] = total;
    }
}

// the second and last launch: a wave per quote sums the quote's three columns and its expiry's [sum w, sum w^2] in row order
// and forms the price and its delta-method error; one more wave per expiry forms the statistics.  Block (7 g + s, gamma): the
// strikes 4 s .. 4 s + 3 of group g for s < 6 (TILTED_KT <= 24), the statistics of the group's expiry for s = 6.  The results
// are stored where the caller reads them (device memory, or the session's pinned host buffer).
constexpr int TILTED_FINISH_SUBS = 7;
static_assert(TILTED_KT <= 4 * (TILTED_FINISH_SUBS - 1) && TILTED_BLOCKS <= 4u * BLOCK, "tilted_finish_kernel's block map and row count");
__global__ __launch_bounds__(BLOCK) void tilted_finish_kernel(TiltedGroupPack pack, const double *__restrict__ partials, unsigned n_rows,
                                                              int ld, int stats_col0, double n_path, double *__restrict__ prices,
                                                              double *__restrict__ stderrs, double *__restrict__ stats,
                                                              size_t n_strikes, int n_expiries, size_t first_strike, int gamma0)
{
    const TiltedGroup &d = pack.g[blockIdx.x / TILTED_FINISH_SUBS];
    const int sub = blockIdx.x % TILTED_FINISH_SUBS;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t row_ld = static_cast<size_t>(gridDim.y) * ld;                   // partials[path block][gamma][column]
    const double *__restrict__ base = partials + static_cast<size_t>(blockIdx.y) * ld;
    const double *__restrict__ st = base + stats_col0 + TILTED_STAT_COLS * d.slot;
    const size_t g = static_cast<size_t>(gamma0) + blockIdx.y;                  // the gamma's index in the call
    if (sub < TILTED_FINISH_SUBS - 1) {
        const int k = 4 * sub + static_cast<int>(wave);
        if (k >= d.k) return;                                                   // (wave-uniform)
        double wq[2], s[3], kept[1];
        wave_column_sums<2>(st, n_rows, row_ld, lane, wq);
        wave_column_sums<1>(st + 6, n_rows, row_ld, lane, kept);
        wave_column_sums<3>(base + 3 * (d.col + k), n_rows, row_ld, lane, s);
        if (lane != 0u) return;
        // price = shift + sum w d / sum w; sum (w (pay - price))^2 = sum (w d)^2 - 2 e sum w^2 d + e^2 sum w^2, e = price - shift.
        // One kept path: the estimate IS that path's payoff and the squares about it are zero identically, where the sums would
        // leave the square root of their rounding
        const double e = s[0] / wq[0];
        const double var = (kept[0] > 1.0) ? fma(e, fma(e, wq[1], -2.0 * s[2]), s[1]) : 0.0;
        const size_t q = g * n_strikes + first_strike + static_cast<size_t>(d.col + k);
        prices[q] = e - d.nshift[k];
        stderrs[q] = sqrt(fmax(var, 0.0)) / wq[0];
        return;
    }
    if (!d.first || wave != 0u) return;
    double a[4], b[3];
    wave_column_sums<4>(st, n_rows, row_ld, lane, a);
    wave_column_sums<3>(st + 4, n_rows, row_ld, lane, b);
    if (lane != 0u) return;
    const double W = a[0], Q = a[1], V2 = a[2], D0 = a[3], D1 = b[0], D2 = b[1], kept = b[2];
    // normalizer n / sum w, a ratio of sums: error sqrt(sum (1 - N w)^2) / sum w = N sqrt(sum (w - mean w)^2) / sum w, the
    // squares about the mean from the sums of w - 1
    const double N = kept / W, sv = W - kept;
    const double dev2 = (kept > 1.0) ? V2 - sv * sv / kept : 0.0;                  // one kept path: zero identically, as above
    // gamma forward sum w spot / sum w = forward + sum w ds / sum w, its error as a strike's
    const double gd = D0 / W;
    const double varg = (kept > 1.0) ? fma(gd, fma(gd, Q, -2.0 * D1), D2) : 0.0;
    double *out = stats + (g * static_cast<size_t>(n_expiries) + static_cast<size_t>(d.expiry)) * SVMC_TILTED_STATS_DOUBLES;
    out[0] = N;
    out[1] = N * sqrt(fmax(dev2, 0.0)) / W;
    out[2] = d.forward + gd;
    out[3] = sqrt(fmax(varg, 0.0)) / W;
    out[4] = (W / Q) * W;                                                      // effective sample size (sum w)^2 / sum w^2
    out[5] = kept;
    out[6] = n_path - kept;
    out[7] = W;
}

// path blocks of a tilted launch: no block with fewer than SVMC_PAYOFF_MIN_TRIPS paths per lane, TILTED_BLOCKS at most -- a
// function of the path count alone
static inline unsigned tilted_path_blocks(size_t n_path)
{
    const size_t per = static_cast<size_t>(BLOCK) * SVMC_PAYOFF_MIN_TRIPS;
    const size_t g = (n_path + per - 1) / per;
    return static_cast<unsigned>(g < 1 ? 1 : (g > TILTED_BLOCKS ? TILTED_BLOCKS : g));
}

using TiltedKernel = void (*)(TiltedGroupPack, TiltedGammas, size_t, double *, int, int);
static TiltedKernel tilted_kernel_for(int kt)
{
    if (kt <= 4) return tilted_payoff_group_kernel<4>;
    if (kt <= 8) return tilted_payoff_group_kernel<8>;
    if (kt <= 16) return tilted_payoff_group_kernel<16>;
    return tilted_payoff_group_kernel<TILTED_KT>;
}

// the launches of svmc_tilted_payoff_chain (its arguments are checked there): up to PAYOFF_GROUPS groups per launch pair, and per
// pair as many gammas as the workspace holds partials for -- either split leaves every sum's bits alone
static int tilted_payoff_impl(const char *fn, const double *const *xs, size_t n_path, const double *forwards, int n_expiries,
                              const double *strikes, const int8_t *types, const double *shifts, const size_t *offsets,
                              const double *gammas, int n_gammas, const double *spot_sums, double *prices, double *stderrs,
                              double *stats, void *workspace, size_t workspace_bytes, hipStream_t stream)
{
    const size_t total = offsets[n_expiries];
    const unsigned gx = tilted_path_blocks(n_path);
    double *partials = static_cast<double *>(workspace);
    TiltedGroupPack pack;
    memset(&pack, 0, sizeof(pack));
    int n_groups = 0, cols = 0, kt = 0, slots = 0;
    size_t first_strike = 0;
    auto flush = [&]() -> int {
        if (n_groups == 0) return SVMC_OK;
        const int stats_col0 = (3 * cols + 7) / 8 * 8;
        const int ld = stats_col0 + TILTED_STAT_COLS * slots;
        const size_t per_gamma = static_cast<size_t>(gx) * ld * sizeof(double);
        if (per_gamma > workspace_bytes) return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": workspace too small (svmc_payoff_workspace_bytes)");
        const int batch = static_cast<int>(workspace_bytes / per_gamma < static_cast<size_t>(n_gammas) ? workspace_bytes / per_gamma : n_gammas);
        for (int g0 = 0; g0 < n_gammas; g0 += batch) {
            const int zb = (n_gammas - g0 < batch) ? n_gammas - g0 : batch;
            TiltedGammas gm;
            for (int z = 0; z < SVMC_TILTED_MAX_GAMMAS; ++z) gm.g[z] = (z < zb) ? gammas[g0 + z] : 0.0;
            hipLaunchKernelGGL(tilted_kernel_for(kt), dim3(gx, static_cast<unsigned>(n_groups), static_cast<unsigned>(zb)), dim3(BLOCK), 0,
                               stream, pack, gm, n_path, partials, ld, stats_col0);
            hipLaunchKernelGGL(tilted_finish_kernel, dim3(static_cast<unsigned>(n_groups * TILTED_FINISH_SUBS), static_cast<unsigned>(zb)),
                               dim3(BLOCK), 0, stream, pack, static_cast<const double *>(partials), gx, ld, stats_col0,
                               static_cast<double>(n_path), prices, stderrs, stats, total, n_expiries, first_strike, g0);
            if (int rc = check_launch(fn)) return rc;
        }
        first_strike += static_cast<size_t>(cols);
        n_groups = cols = kt = slots = 0;
        return SVMC_OK;
    };
    for (int i = 0; i < n_expiries; ++i) {
        bool first = true;                      // of this expiry in the pending launch
        size_t k0 = offsets[i];
        do {
            TiltedGroup &d = pack.g[n_groups];
            d.x = xs[i];
            d.spot_sums = spot_sums ? spot_sums + 2 * i : nullptr;
            d.forward = forwards[i];
            const size_t left = offsets[i + 1] - k0;
            d.k = static_cast<int>(left < static_cast<size_t>(TILTED_KT) ? left : TILTED_KT);
            d.col = cols;
            d.expiry = i;
            d.first = first ? 1 : 0;
            if (first) ++slots;
            d.slot = slots - 1;
            d.put_mask = 0u;
            for (int k = 0; k < TILTED_KT; ++k) {
                const bool on = k < d.k;
                const double sgn = (on && types[k0 + k] == SVMC_PUT) ? -1.0 : 1.0;
                const double shift = (on && shifts != nullptr) ? shifts[k0 + k] : 0.0;
                if (sgn < 0.0) d.put_mask |= 1u << k;
                d.c[k] = on ? -sgn * strikes[k0 + k] - shift : -__builtin_huge_val();
                d.nshift[k] = 0.0 - shift;
            }
            cols += d.k;
            kt = (d.k > kt) ? d.k : kt;
            k0 += static_cast<size_t>(d.k);
            first = false;
            if (++n_groups == PAYOFF_GROUPS) {
                if (int rc = flush()) return rc;
                first = true;                   // what is left of this expiry writes its statistics again, the same bits
            }
        } while (k0 < offsets[i + 1]);
    }
    return flush();
}

// ---------------------------------------------------------------------------------------------------
// Impermanent loss of a concentrated-liquidity range on the resident terminal state (svmc_il_payoff; include/svmc.h states the
// estimator and the keep rule).  Three launches: il_moment_kernel, one pass for [sum exp(x), kept] per path
// block; il_payoff_kernel, block (path block, group of IL_G cases): every block adds the moment rows in block_column_sum2's
// order -- the same bits in every block -- for the mean M, then per kept path and case the six pieces, d = pay - pay(p1) and d^2
// (the shift keeps the variance free of the cancellation of pay^2 against its mean); il_finish_kernel, a block per case: the
// case's eight columns in row order, then the value, its error, the piece means and the counts.  The path blocks are a function
// of the path count alone (il_path_blocks), a case's accumulators do not look at its neighbours' and the block sum's tree is the
// same for every accumulator index: a case's results are the same bits whichever other cases share the call.
// ---------------------------------------------------------------------------------------------------
constexpr int IL_G = 4;                 // cases per block: 32 accumulators; no scratch (the build's kernel metadata)
constexpr int IL_NV = 8;                // per case [sqrt, linear, put, call, digital put, digital call, d, d^2]
constexpr unsigned IL_BLOCKS = 256;     // path blocks at most: il_finish_kernel reads one row per thread
constexpr size_t IL_PATHS_PER_BLOCK = 2048;

static inline unsigned il_path_blocks(size_t n_path)
{
    const size_t g = (n_path + IL_PATHS_PER_BLOCK - 1) / IL_PATHS_PER_BLOCK;
    return static_cast<unsigned>(g < 1 ? 1 : (g > IL_BLOCKS ? IL_BLOCKS : g));
}

struct IlCase {                         // a row of the device table, SVMC_IL_CASE_DOUBLES doubles
    double p1, p0, pa, pb, notional;
};
static_assert(sizeof(IlCase) == SVMC_IL_CASE_DOUBLES * sizeof(double), "the case table's row");

struct IlConsts {
    double p0, pa, pb, sp0, inv_spa, inv_spb, two_spa, two_spb;
};

__device__ __forceinline__ IlConsts il_consts(const IlCase &c)
{
    const double sp0 = sqrt_pos(c.p0), spa = sqrt_pos(c.pa), spb = sqrt_pos(c.pb);
    return IlConsts{c.p0, c.pa, c.pb, sp0, 1.0 / spa, 1.0 / spb, 2.0 * spa, 2.0 * spb};
}

// the six pieces of a spot and the hold-minus-pool value they compose (the reference's order of terms)
__device__ __forceinline__ double il_pieces(const IlConsts &k, double spot, double (&pc)[6])
{
    const bool below = spot < k.pa, above = spot > k.pb;
    pc[0] = (below || above) ? 0.0 : sqrt_pos(spot);               // pa <= spot <= pb: a negative recentred spot never gets here
    pc[1] = k.sp0 * (spot / k.p0 + 1.0);
    pc[2] = fmax(k.pa - spot, 0.0);
    pc[3] = fmax(spot - k.pb, 0.0);
    pc[4] = below ? 1.0 : 0.0;
    pc[5] = above ? 1.0 : 0.0;
    return -2.0 * pc[0] + pc[1] + k.inv_spa * pc[2] - k.inv_spb * pc[3] - k.two_spa * pc[4] - k.two_spb * pc[5];
}

__global__ __launch_bounds__(BLOCK) void il_moment_kernel(const double *__restrict__ x, size_t n, double *__restrict__ moments)
{
    __shared__ double lds[4 * 2];
    constexpr double INF = __builtin_huge_val();
    double acc[2] = {0.0, 0.0};
    for (size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * BLOCK) {
        const double xi = x[i], e = exp_full(xi);
        const bool keep = (fabs(xi) < INF) && (e < INF);             // a NaN fails both
        acc[0] += keep ? e : 0.0;
        acc[1] += keep ? 1.0 : 0.0;
    }
    block_sum_apply<2>(acc, lds, 2, [&](int j, double t) { moments[static_cast<size_t>(j) * gridDim.x + blockIdx.x] = t; });
}

__global__ __launch_bounds__(BLOCK) void il_payoff_kernel(const double *__restrict__ x, size_t n, const IlCase *__restrict__ cases,
                                                          int n_cases, const double *__restrict__ moments, unsigned n_rows,
                                                          double *__restrict__ partials)
{
    constexpr int NSUM = IL_G * IL_NV;
    static_assert(NSUM % 8 == 0, "block_sum_apply's halving tree");
    __shared__ double lds[4 * NSUM];
    __shared__ double mean_exp;
    constexpr double INF = __builtin_huge_val();
    double s0, s1;
    block_column_sum2(moments, moments + n_rows, n_rows, lds, s0, s1);
    if (threadIdx.x == 0) mean_exp = s0 / s1;
    __syncthreads();                                                 // ... and lds may be written again
    const double M = mean_exp;
    IlConsts k[IL_G];
    double p1[IL_G], corr[IL_G], ref[IL_G], acc[NSUM];
#pragma unroll
    for (int g = 0; g < IL_G; ++g) {
        const int c = static_cast<int>(blockIdx.y) * IL_G + g;
        const IlCase cs = cases[c < n_cases ? c : n_cases - 1];      // a group's unused slots repeat the last case, unstored
        k[g] = il_consts(cs);
        p1[g] = cs.p1;
        corr[g] = cs.p1 * M - cs.p1;
        double pc[6];
        ref[g] = il_pieces(k[g], cs.p1, pc);
    }
#pragma unroll
    for (int j = 0; j < NSUM; ++j) acc[j] = 0.0;
    for (size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * BLOCK) {
        const double xi = x[i], e = exp_full(xi);
        const bool keep = (fabs(xi) < INF) && (e < INF);
        if (!keep) continue;
#pragma unroll
        for (int g = 0; g < IL_G; ++g) {
            double pc[6];
            const double d = il_pieces(k[g], p1[g] * e - corr[g], pc) - ref[g];
#pragma unroll
            for (int q = 0; q < 6; ++q) acc[IL_NV * g + q] += pc[q];
            acc[IL_NV * g + 6] += d;
            acc[IL_NV * g + 7] = fma(d, d, acc[IL_NV * g + 7]);
        }
    }
    // partials[path block][case][IL_NV]
    double *row = partials + static_cast<size_t>(blockIdx.x) * n_cases * IL_NV;
    block_sum_apply<NSUM>(acc, lds, NSUM, [&](int j, double t) {
        const int c = static_cast<int>(blockIdx.y) * IL_G + j / IL_NV;
        if (c < n_cases) row[static_cast<size_t>(c) * IL_NV + (j % IL_NV)] = t;
    });
}

__global__ __launch_bounds__(BLOCK) void il_finish_kernel(const IlCase *__restrict__ cases, int n_cases,
                                                          const double *__restrict__ moments, const double *__restrict__ partials,
                                                          unsigned n_rows, double n_path, double *__restrict__ out)
{
    __shared__ double lds[4];
    const int c = blockIdx.x;
    const size_t ld = static_cast<size_t>(n_cases) * IL_NV;
    double tot[IL_NV + 1];
#pragma unroll
    for (int q = 0; q <= IL_NV; ++q) {
        tot[q] = (q < IL_NV) ? block_column_sum(partials + static_cast<size_t>(c) * IL_NV + q, n_rows, ld, lds)
                             : block_column_sum(moments + n_rows, n_rows, 1, lds);
        __syncthreads();                                             // thread 0 has read the wave totals
    }
    if (threadIdx.x != 0) return;
    const IlCase cs = cases[c];
    const IlConsts k = il_consts(cs);
    double pc[6];
    const double ref = il_pieces(k, cs.p1, pc);
    const double kept = tot[IL_NV];
    const double spa = 0.5 * k.two_spa, spb = 0.5 * k.two_spb;                                      // exact halves
    const double scale = (1.0 / (2.0 * k.sp0 - cs.p0 / spb - spa)) * cs.notional;                   // notional0 notional
    const double md = tot[6] / kept;
    const double var = (kept > 1.0) ? fmax(tot[7] / kept - md * md, 0.0) : 0.0;     // one kept path: zero identically
    double *o = out + static_cast<size_t>(c) * SVMC_IL_OUT_DOUBLES;
    o[0] = -scale * (ref + md);
    o[1] = scale * sqrt(var / kept);
#pragma unroll
    for (int q = 0; q < 6; ++q) o[2 + q] = tot[q] / kept;
    o[8] = kept;
    o[9] = n_path - kept;
}

// the stepping of svmc_chain.hip's fused chains from the start state (0, sigma0 | var0, 0): svmc_*_chain_rng_from, or the slice
// kernel for a single expiry; spot_sums null leaves the per-wave partial columns in `workspace` for the one-device tail
int logsv_step_partials(double sigma0, double *x, double *sigma, double *qvar, size_t n_path, int n_slices, const int *nb_steps_host,
                        const double *dts_host, const double *etas_host, const double *forwards_host, double theta, double kappa1,
                        double kappa2, double beta, double volvol, int is_spot_measure, uint64_t seed, uint32_t call_id,
                        uint64_t path_offset, double *x_snapshots, double *qvar_snapshots, double *spot_sums, void *workspace,
                        size_t workspace_bytes, hipStream_t stream)
{
    const StateInit init = {1, 0.0, sigma0, 0.0};
    const svmc_stream_t st = reinterpret_cast<svmc_stream_t>(stream);
    if (n_slices == 1)
        return logsv_slice_rng_impl("logsv_step_partials", init, x, sigma, qvar, n_path, nb_steps_host[0], dts_host[0], theta, kappa1,
                                    kappa2, beta, volvol, etas_host ? etas_host[0] : 1.0, is_spot_measure, seed, call_id, path_offset, 0,
                                    forwards_host[0], x_snapshots, qvar_snapshots, spot_sums, workspace, workspace_bytes, st);
    return logsv_chain_rng_impl("logsv_step_partials", init, x, sigma, qvar, n_path, n_slices, nb_steps_host, dts_host, etas_host,
                                forwards_host, theta, kappa1, kappa2, beta, volvol, is_spot_measure, seed, call_id, path_offset, 0,
                                x_snapshots, qvar_snapshots, spot_sums, workspace, workspace_bytes, st);
}

// the largest launch whose payoff blocks form their spot sums themselves: 2048 rows = 131072 paths, ONE batched round trip of
// loads per block (block_column_sum2); above, the reduce launch is cheaper than what every block would repeat (see above)
bool spot_sums_in_payoff_kernel(size_t n_path) { return wave_rows(n_path) <= 8u * BLOCK; }

// reduce the generators' per-wave partial columns [n_cols][rows] into spot_sums[n_cols] (what the stepping entry points do
// themselves unless told not to)
int reduce_spot_partials(const void *workspace, size_t n_path, int n_cols, double *spot_sums, hipStream_t stream)
{
    if (n_cols <= 0) return SVMC_OK;
    hipLaunchKernelGGL(reduce_columns_kernel, dim3(static_cast<unsigned>(n_cols)), dim3(BLOCK), 0, stream,
                       static_cast<const double *>(workspace), wave_rows(n_path), size_t(1), static_cast<size_t>(wave_rows(n_path)),
                       spot_sums);
    return check_launch("reduce_spot_partials");
}

// ---- many jobs of one chain (svmc_chain.hip's svmc_*_chain_price_many)

// the job table of n_jobs jobs of n_slices expiries, whichever family's is the largest (one pinned and one device buffer serve
// every model)
size_t logsv_many_table_bytes(int n_jobs, int n_slices) { return many_table_bytes_of<LogsvFast>(n_jobs, n_slices); }
size_t many_table_bytes(int n_jobs, int n_slices)
{
    return std::max({logsv_many_table_bytes(n_jobs, n_slices), heston_many_table_bytes(n_jobs, n_slices),
                     hawkes_many_table_bytes(n_jobs, n_slices)});
}

ManySlices many_slices(int n_slices, const int *nb_steps_host, const double *forwards_host)
{
    ManySlices cs;
    cs.m = n_slices;
    for (int i = 0; i < MAX_CHAIN_SLICES; ++i) {
        cs.forward[i] = forwards_host[i < n_slices ? i : 0];
        cs.nb_steps[i] = i < n_slices ? nb_steps_host[i] : 0;
        cs.total_steps += cs.nb_steps[i];
    }
    return cs;
}

int check_many(const char *fn, size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
               const uint32_t *call_ids)
{
    SVMC_REQUIRE(n_path > 0 && n_jobs >= 1 && n_jobs <= MAX_MANY_JOBS && n_slices >= 1 && n_slices <= MAX_CHAIN_SLICES,
                 std::string(fn) + ": bad sizes");
    for (int i = 0; i < n_slices; ++i)
        SVMC_REQUIRE(nb_steps_host[i] > 0 && dts_host[i] > 0.0, std::string(fn) + ": nb_steps and dt must be positive");
    for (int j = 0; j < n_jobs; ++j) SVMC_REQUIRE(call_ids[j] < (1u << 24), std::string(fn) + ": call_id must fit 24 bits");
    return SVMC_OK;
}

int check_quotes(const char *fn, size_t n_path, const double *forwards_host, const double *discfactors_host, int n_expiries,
                 const double *strikes_host, const int8_t *types_host, const size_t *strike_offsets_host, size_t strike_limit,
                 size_t quotes_per_strike)
{
    SVMC_REQUIRE(forwards_host && strikes_host && types_host && strike_offsets_host, std::string(fn) + ": null pointer");
    SVMC_REQUIRE(n_path > 0 && n_expiries >= 1, std::string(fn) + ": n_path and n_expiries must be positive");
    for (int i = 0; i < n_expiries; ++i) {
        SVMC_REQUIRE(strike_offsets_host[i] <= strike_offsets_host[i + 1], std::string(fn) + ": strike offsets must not decrease");
        SVMC_REQUIRE(std::isfinite(forwards_host[i]) && forwards_host[i] > 0.0, std::string(fn) + ": a forward is not positive and finite");
        SVMC_REQUIRE(!discfactors_host || std::isfinite(discfactors_host[i]), std::string(fn) + ": a discount factor is not finite");
    }
    const size_t K = strike_offsets_host[n_expiries];
    SVMC_REQUIRE(quotes_per_strike * K < strike_limit, std::string(fn) + ": too many strikes");      // (before the loop over them)
    for (size_t k = 0; k < K; ++k) {
        if (types_host[k] != SVMC_CALL && types_host[k] != SVMC_PUT) return fail(SVMC_ERR_UNKNOWN_PAYOFF, "unknown option payoff code");
        SVMC_REQUIRE(std::isfinite(strikes_host[k]), std::string(fn) + ": a strike is not finite");
    }
    return SVMC_OK;
}

int check_steps(const char *fn, int n_params, const double *steps_host, int min_params)
{
    SVMC_REQUIRE(n_params >= min_params && n_params <= SVMC_GREEKS_MAX_PARAMS,
                 std::string(fn) + ": n_params must be in [" + std::to_string(min_params) + ", SVMC_GREEKS_MAX_PARAMS]");
    SVMC_REQUIRE(n_params == 0 || steps_host != nullptr, std::string(fn) + ": null steps");
    for (int p = 0; p < n_params; ++p)
        SVMC_REQUIRE(std::isfinite(steps_host[p]) && steps_host[p] > 0.0, std::string(fn) + ": a step is not positive and finite");
    return SVMC_OK;
}

int logsv_chain_rng_many(size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
                         const double *forwards_host, const double *params_host, int is_spot_measure, const uint64_t *seeds,
                         const uint32_t *call_ids, uint64_t path_offset, void *table_host, void *table_dev, double *x_snapshots,
                         double *qvar_snapshots, double *spot_partials, hipStream_t stream)
{
    const char *fn = "logsv_chain_rng_many";
    if (int rc = check_many(fn, n_path, n_jobs, n_slices, nb_steps_host, dts_host, call_ids)) return rc;
    const size_t row = 6 + static_cast<size_t>(n_slices);       // v0 theta kappa1 kappa2 beta volvol, etas
    hipError_t e = hipSuccess;
    const ManyJobs jobs = many_table<LogsvFast>(n_jobs, n_slices, seeds, call_ids, table_host, table_dev, stream,
                                                [&](int j, LogsvFast *c) {
        const double *p = params_host + row * static_cast<size_t>(j);
        for (int i = 0; i < n_slices; ++i)
            c[i] = logsv_fast_in_log_units(make_logsv_fast(make_logsv_consts(dts_host[i], p[1], p[2], p[3], p[4], p[5], p[6 + i],
                                                                             is_spot_measure)));
        return p[0];
    }, e);
    SVMC_HIP_TRY(e);
    const ManySlices cs = many_slices(n_slices, nb_steps_host, forwards_host);
    const unsigned J = static_cast<unsigned>(n_jobs);
    // the form is chosen by the launch's TOTAL path count: J jobs of n paths put J n / 64 waves on the device
    if (few_waves_launch(static_cast<size_t>(n_jobs) * n_path))
        hipLaunchKernelGGL((logsv_chain_rng_many_lat_kernel<GEN_LOOP_PIPE, 4, FEW_BLOCK>), dim3(lat_grid(n_path), J), dim3(FEW_BLOCK), 0,
                           stream, n_path, cs, jobs, path_offset, x_snapshots, qvar_snapshots, spot_partials, armed_probe());
    else
        hipLaunchKernelGGL(logsv_chain_rng_many_kernel, dim3(chain_grid(n_path), J), dim3(CHAIN_BLOCK), 0, stream, n_path, cs, jobs,
                           path_offset, x_snapshots, qvar_snapshots, spot_partials, armed_probe());
    return check_launch(fn);
}

// an upper bound of the payoff workspace chain_payoff_and_finish_sets needs for n_sets sets of total_strikes quotes
size_t payoff_sets_workspace_bytes(size_t n_path, size_t total_strikes, int n_sets)
{
    const size_t g = reduce_grid(n_path), a = g * 3 * PAYOFF_KT * PAYOFF_GROUPS, b = g * static_cast<size_t>(n_sets) * 3 * total_strikes;
    return (a > b ? a : b) * sizeof(double);
}

// the tail of n_sets jobs whose spot sums are in spot_sums [set][m][2]: ONE payoff launch (blockIdx.z = set, the path blocks of a
// one-set launch) and ONE chain_finish_kernel over the n_sets x cols quotes -- partials[path block][set][3 cols] are the columns
// of one [rows][3 n_sets cols] matrix -- into sums_out [set][3 cols]; a launch with more path blocks than that kernel sums takes
// the column reduce into sums_dev and a copy instead.  The chain must fit one payoff launch (payoff_sets_fit).
int chain_payoff_and_finish_sets(const double *const *x_snapshots_host, const double *const *qvar_snapshots_host, size_t n_path,
                                 const double *forwards_host, const double *ttms_host, const double *spot_sums, int n_expiries,
                                 const double *strikes_host, const int8_t *types_host, const double *shifts_host,
                                 const size_t *strike_offsets_host, int variable_type, void *workspace, size_t workspace_bytes,
                                 hipStream_t stream, int n_sets, size_t x_set_stride, size_t q_set_stride, size_t spot_set_stride,
                                 double *sums_dev, double *sums_out)
{
    const char *fn = "chain_payoff_and_finish_sets";
    PayoffPartialsOut po;
    if (int rc = payoff_sums_impl(fn, x_snapshots_host, qvar_snapshots_host, n_path, forwards_host, ttms_host, spot_sums, n_expiries,
                                  strikes_host, types_host, shifts_host, strike_offsets_host, variable_type, nullptr, workspace,
                                  workspace_bytes, reinterpret_cast<svmc_stream_t>(stream), n_sets,
                                  PayoffSetStrides{x_set_stride, q_set_stride, spot_set_stride}, nullptr, 0, &po))
        return rc;
    if (po.cols == 0) return SVMC_OK;
    const size_t cols = static_cast<size_t>(po.cols) * static_cast<size_t>(n_sets);
    if (po.rows <= 4u * BLOCK) {
        hipLaunchKernelGGL(chain_finish_kernel, dim3(static_cast<unsigned>((cols + BLOCK / 64 - 1) / (BLOCK / 64))), dim3(BLOCK), 0,
                           stream, static_cast<const double *>(workspace), po.rows, static_cast<int>(cols), sums_out);
    } else {
        reduce_columns(static_cast<unsigned>(3 * cols), stream, static_cast<const double *>(workspace), po.rows, 3 * cols, size_t(1),
                       sums_dev);
        SVMC_HIP_TRY(hipMemcpyAsync(sums_out, sums_dev, 3 * cols * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    return check_launch(fn);
}

}  // namespace svmc

extern "C" {

int svmc_payoff_sums(const double *x, const double *qvar, size_t n_path, double forward, double ttm,
                     const double *spot_sums, const double *strikes_host, const int8_t *types_host,
                     const double *shifts_host, size_t n_strikes, int variable_type, double *sums, void *workspace,
                     size_t workspace_bytes, svmc_stream_t stream)
{
    if (variable_type != SVMC_LOG_RETURN && variable_type != SVMC_Q_VAR)
        return fail(SVMC_ERR_UNSUPPORTED_VARIABLE, "svmc_payoff_sums: variable_type must be LOG_RETURN or Q_VAR");
    SVMC_REQUIRE(x && spot_sums && sums && workspace, "svmc_payoff_sums: null pointer");
    SVMC_REQUIRE(variable_type != SVMC_Q_VAR || qvar != nullptr, "svmc_payoff_sums: Q_VAR needs qvar");
    SVMC_REQUIRE(n_strikes == 0 || (strikes_host && types_host), "svmc_payoff_sums: null strikes/types");
    const size_t offsets[2] = {0, n_strikes};
    return payoff_sums_impl("svmc_payoff_sums", &x, &qvar, n_path, &forward, &ttm, spot_sums, 1, strikes_host, types_host,
                            shifts_host, offsets, variable_type, sums, workspace, workspace_bytes, stream);
}

int svmc_payoff_sums_chain(const double *const *x_snapshots_host, const double *const *qvar_snapshots_host, size_t n_path,
                           const double *forwards_host, const double *ttms_host, const double *spot_sums,
                           int n_expiries, const double *strikes_host, const int8_t *types_host,
                           const double *shifts_host, const size_t *strike_offsets_host, int variable_type,
                           double *sums, void *workspace, size_t workspace_bytes, svmc_stream_t stream)
{
    if (variable_type != SVMC_LOG_RETURN && variable_type != SVMC_Q_VAR)
        return fail(SVMC_ERR_UNSUPPORTED_VARIABLE, "svmc_payoff_sums_chain: variable_type must be LOG_RETURN or Q_VAR");
    SVMC_REQUIRE(x_snapshots_host && forwards_host && ttms_host && spot_sums && strike_offsets_host && sums && workspace,
                 "svmc_payoff_sums_chain: null pointer");
    SVMC_REQUIRE(n_expiries >= 1, "svmc_payoff_sums_chain: n_expiries < 1");
    SVMC_REQUIRE(variable_type != SVMC_Q_VAR || qvar_snapshots_host != nullptr, "svmc_payoff_sums_chain: Q_VAR needs qvar");
    const size_t total = strike_offsets_host[n_expiries];
    SVMC_REQUIRE(total == 0 || (strikes_host && types_host), "svmc_payoff_sums_chain: null strikes/types");
    return payoff_sums_impl("svmc_payoff_sums_chain", x_snapshots_host, qvar_snapshots_host, n_path, forwards_host, ttms_host,
                            spot_sums, n_expiries, strikes_host, types_host, shifts_host, strike_offsets_host, variable_type,
                            sums, workspace, workspace_bytes, stream);
}

int svmc_tilted_payoff_chain(const double *const *x_snapshots_host, size_t n_path, const double *forwards_host, int n_expiries,
                             const double *strikes_host, const int8_t *types_host, const double *shifts_host,
                             const size_t *strike_offsets_host, const double *gammas_host, int n_gammas, int recenter,
                             const double *spot_sums, double *prices, double *stderrs, double *stats, void *workspace,
                             size_t workspace_bytes, svmc_stream_t stream)
{
    const char *fn = "svmc_tilted_payoff_chain";
    SVMC_REQUIRE(x_snapshots_host && forwards_host && strike_offsets_host && gammas_host && prices && stderrs && stats && workspace,
                 std::string(fn) + ": null pointer");
    SVMC_REQUIRE(n_path >= 1 && n_expiries >= 1, std::string(fn) + ": n_path and n_expiries must be positive");
    SVMC_REQUIRE(n_gammas >= 1 && n_gammas <= SVMC_TILTED_MAX_GAMMAS, std::string(fn) + ": n_gammas outside 1 .. SVMC_TILTED_MAX_GAMMAS");
    SVMC_REQUIRE(!recenter || spot_sums != nullptr, std::string(fn) + ": recenter needs spot_sums");
    const size_t total = strike_offsets_host[n_expiries];
    SVMC_REQUIRE(total == 0 || (strikes_host && types_host), std::string(fn) + ": null strikes/types");
    for (int g = 0; g < n_gammas; ++g) SVMC_REQUIRE(std::isfinite(gammas_host[g]), std::string(fn) + ": a gamma is not finite");
    for (int i = 0; i < n_expiries; ++i) {
        SVMC_REQUIRE(x_snapshots_host[i] != nullptr, std::string(fn) + ": null snapshot");
        SVMC_REQUIRE(std::isfinite(forwards_host[i]), std::string(fn) + ": a forward is not finite");
        SVMC_REQUIRE(strike_offsets_host[i] <= strike_offsets_host[i + 1], std::string(fn) + ": strike offsets must not decrease");
    }
    for (size_t k = 0; k < total; ++k) {
        if (types_host[k] != SVMC_CALL && types_host[k] != SVMC_PUT) return fail(SVMC_ERR_UNKNOWN_PAYOFF, "unknown option payoff code");
        SVMC_REQUIRE(std::isfinite(strikes_host[k]) && (shifts_host == nullptr || std::isfinite(shifts_host[k])),
                     std::string(fn) + ": a strike or shift is not finite");
    }
    if (workspace_bytes < static_cast<size_t>(MAX_REDUCE_GRID) * 3 * PAYOFF_KT * PAYOFF_GROUPS * sizeof(double))
        return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": workspace too small (svmc_payoff_workspace_bytes)");
    return tilted_payoff_impl(fn, x_snapshots_host, n_path, forwards_host, n_expiries, strikes_host, types_host, shifts_host,
                              strike_offsets_host, gammas_host, n_gammas, recenter ? spot_sums : nullptr, prices, stderrs, stats,
                              workspace, workspace_bytes, as_stream(stream));
}

int svmc_il_payoff_workspace_bytes(size_t n_path, size_t n_cases, size_t *bytes)
{
    SVMC_REQUIRE(bytes, "svmc_il_payoff_workspace_bytes: null pointer");
    SVMC_REQUIRE(n_path >= 1 && n_cases >= 1 && n_cases <= SVMC_IL_MAX_CASES, "svmc_il_payoff_workspace_bytes: n_path or n_cases out of range");
    const size_t rows = il_path_blocks(n_path);
    // [moments 2 x rows | case table | results | partials rows x n_cases x 8]
    *bytes = sizeof(double) * (2 * rows + n_cases * (SVMC_IL_CASE_DOUBLES + SVMC_IL_OUT_DOUBLES) + rows * n_cases * IL_NV);
    return SVMC_OK;
}

int svmc_il_payoff(const double *x, size_t n_path, const double *cases_host, size_t n_cases, double *out_host, void *workspace,
                   size_t workspace_bytes, svmc_stream_t stream)
{
    const char *fn = "svmc_il_payoff";
    SVMC_REQUIRE(x && cases_host && out_host && workspace, std::string(fn) + ": null pointer");
    SVMC_REQUIRE(n_path >= 1 && n_path < (static_cast<size_t>(1) << 40), std::string(fn) + ": n_path must be in 1 .. 2^40 - 1");
    SVMC_REQUIRE(n_cases >= 1 && n_cases <= SVMC_IL_MAX_CASES, std::string(fn) + ": n_cases outside 1 .. SVMC_IL_MAX_CASES");
    for (size_t c = 0; c < n_cases; ++c) {
        const double *r = cases_host + SVMC_IL_CASE_DOUBLES * c;
        for (int q = 0; q < SVMC_IL_CASE_DOUBLES; ++q)
            SVMC_REQUIRE(r[q] > 0.0 && r[q] < HUGE_VAL, std::string(fn) + ": p1, p0, pa, pb and the notional must be positive and finite");
        SVMC_REQUIRE(r[2] < r[1] && r[1] < r[3], std::string(fn) + ": a case needs pa < p0 < pb");
    }
    size_t need = 0;
    svmc_il_payoff_workspace_bytes(n_path, n_cases, &need);
    if (workspace_bytes < need) return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": workspace too small (svmc_il_payoff_workspace_bytes)");
    const unsigned rows = il_path_blocks(n_path);
    double *moments = static_cast<double *>(workspace);
    IlCase *cases = reinterpret_cast<IlCase *>(moments + 2 * static_cast<size_t>(rows));
    double *out = reinterpret_cast<double *>(cases + n_cases);
    double *partials = out + n_cases * SVMC_IL_OUT_DOUBLES;
    hipStream_t s = as_stream(stream);
    SVMC_HIP_TRY(hipMemcpyAsync(cases, cases_host, sizeof(IlCase) * n_cases, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(il_moment_kernel, dim3(rows), dim3(BLOCK), 0, s, x, n_path, moments);
    hipLaunchKernelGGL(il_payoff_kernel, dim3(rows, static_cast<unsigned>((n_cases + IL_G - 1) / IL_G)), dim3(BLOCK), 0, s, x, n_path,
                       static_cast<const IlCase *>(cases), static_cast<int>(n_cases), static_cast<const double *>(moments), rows, partials);
    hipLaunchKernelGGL(il_finish_kernel, dim3(static_cast<unsigned>(n_cases)), dim3(BLOCK), 0, s, static_cast<const IlCase *>(cases),
                       static_cast<int>(n_cases), static_cast<const double *>(moments), static_cast<const double *>(partials), rows,
                       static_cast<double>(n_path), out);
    if (int rc = check_launch(fn)) return rc;
    SVMC_HIP_TRY(hipMemcpyAsync(out_host, out, sizeof(double) * n_cases * SVMC_IL_OUT_DOUBLES, hipMemcpyDeviceToHost, s));
    SVMC_HIP_TRY(hipStreamSynchronize(s));
    return SVMC_OK;
}

int svmc_payoff_finalize(const double *sums_host, const double *shifts_host, size_t n_strikes, double discfactor,
                         double n_path_total, double *prices_host, double *stderrs_host)
{
    SVMC_REQUIRE(sums_host && prices_host && stderrs_host, "svmc_payoff_finalize: null pointer");
    for (size_t k = 0; k < n_strikes; ++k)
        payoff_finalize_one(sums_host[3 * k], sums_host[3 * k + 1], sums_host[3 * k + 2], shifts_host ? shifts_host[k] : 0.0,
                            discfactor, n_path_total, prices_host + k, stderrs_host + k);
    return SVMC_OK;
}

int svmc_payoff_finalize_chain(const double *sums_host, const double *shifts_host, const double *discfactors_host,
                               size_t n_strikes, double n_path_total, double *prices_host, double *stderrs_host)
{
    SVMC_REQUIRE(sums_host && discfactors_host && prices_host && stderrs_host, "svmc_payoff_finalize_chain: null pointer");
    for (size_t k = 0; k < n_strikes; ++k)
        payoff_finalize_one(sums_host[3 * k], sums_host[3 * k + 1], sums_host[3 * k + 2], shifts_host ? shifts_host[k] : 0.0,
                            discfactors_host[k], n_path_total, prices_host + k, stderrs_host + k);
    return SVMC_OK;
}

}  // extern "C"
