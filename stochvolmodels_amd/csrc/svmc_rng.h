// svmc_rng.h -- counter-based randoms for the gfx950 kernels.
//
// Philox4x32-7 (Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11: seven rounds is
// the smallest Crush-resistant count of the 4x32 variant, ten the paper's safety default) keyed by the seed and
// indexed by (global path id, call index, stream, call id): a lane owns a path, so it derives every increment it
// needs in registers, no generator state lives in memory and the result is independent of how paths are sharded over
// GPUs.  Replaces the reference's serial MT19937+polar draw of two [nb_steps, nb_path] arrays
// (pricers/logsv_pricer.py:1025-1026, pricers/heston_pricer.py:369-370).
//
// Stream definition, version 4 (DESIGN.md "RNG"; CPU twin: oracle/svmc_oracle.c svo_draw_normals).  One call yields
// four 32-bit words = the two normals of TWO consecutive time steps, each word turned into ONE N(0,1) variate by
// inversion:
//   (r0, r1, r2, r3) = philox4x32_7(ctr = (path_lo, path_hi, step >> 1, stream | call_id << 8), key = seed)
//   (ra, rb) = (r0, r1) for an even chain-global step index, (r2, r3) for an odd one
//   z(r) = sign(t) P_j(|t| - c_j),  t = (int32) r  (version 3: + 1/2):  the piecewise cubic of -Phi^-1(|t| 2^-32) of
//          svmc_icdf_table.h (tools/gen_icdf_table.py; svmc_math.h normal_icdf32), |z| <= 6.23, z = 0 at t = 0 and |t| = 2^31
//   (w0, w1) = (z(ra), z(rb))
//   stream 1:  uniform = 52 bits of r1:r0 (one call per draw);  Heston QE: normals from stream 4 (as stream 0), the
//   exponential branch's uniform (r[step & 3] + 1/2) 2^-32 of stream 5's call step >> 2, drawn lazily.
//   Hawkes jump-diffusion (svmc_hawkes.hip): ONE call of stream 6 per step at index = the chain-global step (not step >> 1):
//   z(r0) the diffusion's normal, u_p = (r1 + 1/2) 2^-32, u_m = (r2 + 1/2) 2^-32, r3 unused; on a step where a side jumps (and
//   only there, lazily) stream 7's call at the same index: E_p = -ln((r0 + 1/2) 2^-32), E_m = -ln((r1 + 1/2) 2^-32).
//   Conditional Monte Carlo (svmc_cmc.hip): stream 8, ONE normal per step -- a call carries FOUR steps, laid out as stream 5's
//   uniforms are: step s (chain-global) takes z(r[s & 3]) of the call at index s >> 2, so a slice may begin or end anywhere inside
//   a call without changing what a (path, step) sees.  Streams 0 .. 7 are untouched: the stream version stays 4.
//   Conditional Monte Carlo for Hawkes (svmc_hawkes.hip hawkes_chain_cond_kernel): stream 9, the jump uniforms of TWO steps per call
//   -- step s takes u_p, u_m from words 2 (s & 1), 2 (s & 1) + 1 of the call at index s >> 1 -- and stream 10 as stream 7: the call
//   at index s, drawn lazily, E_p and E_m from words 0 and 1.  Streams 0 .. 8 are untouched.
// Resolution: a normal carries 32 random bits (as in version 2, whose Box-Muller pair spent 32 on the radius and 32 on
// the angle); the lattice is 2^-32 in probability, symmetric about 0 (every magnitude 1 .. 2^31 - 1 with both signs, two words
// at 0), largest |z| = -Phi^-1(2^-32) = 6.23 (truncated mass 4.7e-10 per normal).  The cubic deviates from the exact inverse CDF by at most SVMC_ICDF_MAX_ABS_ERROR (7.431e-10,
// svmc_icdf_table.h) -- a smooth deterministic distortion five orders below the Monte Carlo error of any chain priced here, pinned against
// scipy's Phi^-1 in tests/test_oracle_golden.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svmc_icdf_table.h"
#include "svmc_log_table.h"
#include "svmc_math.h"

namespace svmc {

// The tables, constant memory -> LDS once per block: the inverse-CDF pieces of the draw (SVMC_ICDF_SEGMENTS x 48 bytes,
// three arrays of 16-byte pieces), the 2 KB exp table of the kernels that call exp2u_tab() / exp_tab(), and -- Heston QE
// only -- the 8 KB log table of its martingale correction.
#if SVMC_ICDF_EDGE && SVMC_ICDF_DEG == 3
#define SVMC_ICDF_PIECES 2
__constant__ IcdfPiece g_icdf_table[2 * SVMC_ICDF_SEGMENTS] = {SVMC_ICDF_PIECE0_INIT, SVMC_ICDF_PIECE1_INIT};
#else
#define SVMC_ICDF_PIECES 3
__constant__ IcdfPiece g_icdf_table[3 * SVMC_ICDF_SEGMENTS] = {SVMC_ICDF_PIECE0_INIT, SVMC_ICDF_PIECE1_INIT, SVMC_ICDF_PIECE2_INIT};
#endif
__constant__ LogTabEntry g_log_table[512] = {SVMC_LOG_TABLE_INIT};
__constant__ double g_exp_table[256] = {SVMC_EXP_TABLE_INIT};

struct RngTables {
    const IcdfPiece *icdf;
    const LogTabEntry *log;        // null unless the kernel staged it (stage_rng_log_tables)
};

constexpr unsigned ICDF_PIECES = SVMC_ICDF_PIECES;
// (a 24-byte mixed-precision form of the table, another stream, measured LDS -22 %, VALU +24 %, 10 % slower on C2:
// profiles/r06_ab_icdf.jsonl)
struct RngTablesLds {
    IcdfPiece icdf[ICDF_PIECES * SVMC_ICDF_SEGMENTS];
};

// the log table alone (the streamed Heston QE kernel: its martingale correction takes logs, it draws nothing)
__device__ __forceinline__ const LogTabEntry *stage_log_table(LogTabEntry (&lds)[512])
{
    for (unsigned i = threadIdx.x; i < 512u; i += blockDim.x) lds[i] = g_log_table[i];
    __syncthreads();
    return lds;
}

__device__ __forceinline__ void copy_icdf_table(RngTablesLds &lds)
{
    for (unsigned i = threadIdx.x; i < ICDF_PIECES * SVMC_ICDF_SEGMENTS; i += blockDim.x) lds.icdf[i] = g_icdf_table[i];
}

__device__ __forceinline__ RngTables stage_rng_tables(RngTablesLds &lds)
{
    copy_icdf_table(lds);
    __syncthreads();
    return RngTables{lds.icdf, nullptr};
}

// Heston QE: the draw's table and the log table behind one barrier
__device__ __forceinline__ RngTables stage_rng_log_tables(RngTablesLds &lds, LogTabEntry (&lds_log)[512])
{
    copy_icdf_table(lds);
    for (unsigned i = threadIdx.x; i < 512u; i += blockDim.x) lds_log[i] = g_log_table[i];
    __syncthreads();
    return RngTables{lds.icdf, lds_log};
}

// a kernel template that draws in one instantiation and reads supplied normals in the other: the table's LDS only in the first
template <bool DRAWS>
struct RngTablesLdsIf {
    RngTablesLds t;
};
template <>
struct RngTablesLdsIf<false> {
    char unused;
};

template <bool DRAWS>
__device__ __forceinline__ RngTables stage_tables_if(RngTablesLdsIf<DRAWS> &lds, double (&lds_exp)[256])
{
    if constexpr (DRAWS) copy_icdf_table(lds.t);
    for (unsigned i = threadIdx.x; i < 256u; i += blockDim.x) lds_exp[i] = g_exp_table[i];
    __syncthreads();
    if constexpr (DRAWS) return RngTables{lds.t.icdf, nullptr};
    else return RngTables{nullptr, nullptr};
}

__device__ __forceinline__ RngTables stage_tables(RngTablesLds &lds, double (&lds_exp)[256])
{
    copy_icdf_table(lds);
    for (unsigned i = threadIdx.x; i < 256u; i += blockDim.x) lds_exp[i] = g_exp_table[i];
    __syncthreads();
    return RngTables{lds.icdf, nullptr};
}

// stage_tables for a kernel whose block size TB is a compile-time constant (the launch must use it): a thread's loads of both
// tables are all issued before its first LDS store, so a block pays ONE global round trip before the barrier, not one per
// piece (the loop above compiles to load, s_waitcnt vmcnt(0), ds_write per trip: five dependent trips at 512 threads)
template <unsigned TB>
__device__ __forceinline__ RngTables stage_tables(RngTablesLds &lds, double (&lds_exp)[256])
{
    constexpr unsigned N = ICDF_PIECES * SVMC_ICDF_SEGMENTS, TRIPS = (N + TB - 1) / TB, EXP_TRIPS = (256u + TB - 1) / TB;
    IcdfPiece piece[TRIPS];
    double e[EXP_TRIPS];
#pragma unroll
    for (unsigned k = 0; k < TRIPS; ++k) {
        const unsigned i = threadIdx.x + k * TB;
        if (N % TB == 0 || i < N) piece[k] = g_icdf_table[i];
    }
#pragma unroll
    for (unsigned k = 0; k < EXP_TRIPS; ++k) {
        const unsigned i = threadIdx.x + k * TB;
        if (i < 256u) e[k] = g_exp_table[i];
    }
#pragma unroll
    for (unsigned k = 0; k < TRIPS; ++k) {
        const unsigned i = threadIdx.x + k * TB;
        if (N % TB == 0 || i < N) lds.icdf[i] = piece[k];
    }
#pragma unroll
    for (unsigned k = 0; k < EXP_TRIPS; ++k) {
        const unsigned i = threadIdx.x + k * TB;
        if (i < 256u) lds_exp[i] = e[k];
    }
    __syncthreads();
    return RngTables{lds.icdf, nullptr};
}

#ifndef SVMC_PHILOX_ROUNDS
#define SVMC_PHILOX_ROUNDS 7
#endif
constexpr int PHILOX_ROUNDS = SVMC_PHILOX_ROUNDS;

__device__ __forceinline__ void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                           uint32_t k0, uint32_t k1, uint32_t (&r)[4])
{
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int i = 0; i < PHILOX_ROUNDS; ++i) {
        // one v_mad_u64_u32 per 32x32->64 product, one v_bitop3_b32 (xor3) per mixed word
        const uint64_t p0 = static_cast<uint64_t>(M0) * c0;
        const uint64_t p1 = static_cast<uint64_t>(M1) * c2;
        const uint32_t n0 = __builtin_amdgcn_bitop3_b32(static_cast<uint32_t>(p1 >> 32), c1, k0, 0x96);
        const uint32_t n2 = __builtin_amdgcn_bitop3_b32(static_cast<uint32_t>(p0 >> 32), c3, k1, 0x96);
        c1 = static_cast<uint32_t>(p1);
        c3 = static_cast<uint32_t>(p0);
        c0 = n0;
        c2 = n2;
        k0 += W0;
        k1 += W1;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// The same function with the work that does not depend on the step taken out of the time loop.  The counter is
// (path_lo, path_hi, call index, c3): in round 1 the product M0 * path_lo, the word path_hi ^ k0 and the whole new third word
// hi(M0 path_lo) ^ c3 ^ k1 are per-lane constants, M1 * step is wave-uniform (scalar unit), and round 2's product
// M1 * (third word) is a per-lane constant again.  Left to the compiler the xor3's of rounds 1-2 each needed a
// v_mov to get a second scalar operand in; here round 1 is one v_xor and round 2 one v_xor + one xor3.
struct PhiloxLane {
    uint32_t a;        // path_hi ^ k0
    uint32_t b;        // hi(M0 path_lo) ^ c3 ^ k1            (round-1 third word)
    uint32_t lo0;      // lo(M0 path_lo)                      (round-1 fourth word)
    uint32_t hi_b;     // hi(M1 b)
    uint32_t lo_b;     // lo(M1 b)                            (round-2 second word)
    uint32_t k0, k1;   // round-2 keys
};

__device__ __forceinline__ PhiloxLane philox_prepare(uint64_t seed, uint32_t c3, uint64_t path)
{
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
    const uint64_t p0 = static_cast<uint64_t>(M0) * static_cast<uint32_t>(path);
    PhiloxLane l;
    l.a = static_cast<uint32_t>(path >> 32) ^ k0;
    l.b = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    l.lo0 = static_cast<uint32_t>(p0);
    const uint64_t pb = static_cast<uint64_t>(M1) * l.b;
    l.hi_b = static_cast<uint32_t>(pb >> 32);
    l.lo_b = static_cast<uint32_t>(pb);
    l.k0 = k0 + W0;
    l.k1 = k1 + W1;
    // opaque to the optimiser: otherwise it re-splits a into (path_hi, k0) and pays the second xor inside the loop
    asm volatile("" : "+v"(l.a), "+v"(l.b), "+v"(l.lo0), "+v"(l.hi_b), "+v"(l.lo_b));
    return l;
}

template <bool HOIST_KEYS = false>
__device__ __forceinline__ void philox_draw(const PhiloxLane &l, uint32_t step, uint32_t (&r)[4])
{
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    // round 1: c = (hi(M1 step) ^ a, lo(M1 step), b, lo0)
    const uint64_t p1 = static_cast<uint64_t>(M1) * step;                  // wave-uniform
    uint32_t c0 = static_cast<uint32_t>(p1 >> 32) ^ l.a;
    const uint32_t c1_r1 = static_cast<uint32_t>(p1);                      // wave-uniform
    // round 2
    const uint64_t p0 = static_cast<uint64_t>(M0) * c0;
    uint32_t k0 = l.k0, k1 = l.k1;
    // the round keys are re-derived from (k0, k1) with scalar adds on every call: hoisted out of the time loop (what the
    // compiler does by itself) they would occupy a dozen SGPRs of a budget the loop already fills, and the spills come
    // back as v_readlane_b32 -- VALU instructions on the one port this loop is bound by
    // (HOIST_KEYS: the few-waves kernels, whose loop leaves two dozen SGPRs free -- there a wave issues one instruction of ANY
    // kind per ~4.5 cycles, so the twelve scalar adds of a call are twelve issue slots of the one wave a SIMD has)
    if constexpr (!HOIST_KEYS) asm volatile("" : "+s"(k0), "+s"(k1));
    c0 = l.hi_b ^ __builtin_amdgcn_readfirstlane(c1_r1 ^ k0);              // (uniform ^ uniform) stays on the scalar unit
    uint32_t c2 = __builtin_amdgcn_bitop3_b32(static_cast<uint32_t>(p0 >> 32), l.lo0, k1, 0x96);
    uint32_t c1 = l.lo_b;
    uint32_t c3 = static_cast<uint32_t>(p0);
    k0 += W0;
    k1 += W1;
#pragma unroll
    for (int i = 2; i < PHILOX_ROUNDS; ++i) {
        const uint64_t q0 = static_cast<uint64_t>(M0) * c0;
        const uint64_t q1 = static_cast<uint64_t>(M1) * c2;
        const uint32_t n0 = __builtin_amdgcn_bitop3_b32(static_cast<uint32_t>(q1 >> 32), c1, k0, 0x96);
        const uint32_t n2 = __builtin_amdgcn_bitop3_b32(static_cast<uint32_t>(q0 >> 32), c3, k1, 0x96);
        c1 = static_cast<uint32_t>(q1);
        c3 = static_cast<uint32_t>(q0);
        c0 = n0;
        c2 = n2;
        k0 += W0;
        k1 += W1;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// top 52 bits of hi:lo as the mantissa of a double in [1,2): two v_alignbit_b32
__device__ __forceinline__ double mantissa_1_2(uint32_t lo, uint32_t hi)
{
    const uint32_t mhi = __builtin_amdgcn_alignbit(0x3FFu, hi, 12);   // 0x3FF00000 | hi >> 12
    const uint32_t mlo = __builtin_amdgcn_alignbit(hi, lo, 12);       // (hi:lo) >> 12
    return __hiloint2double(static_cast<int>(mhi), static_cast<int>(mlo));
}

__device__ __forceinline__ void philox_draw(uint64_t seed, uint32_t c3, uint64_t path, uint32_t index, uint32_t (&r)[4])
{
    philox4x32(static_cast<uint32_t>(path), static_cast<uint32_t>(path >> 32), index, c3,
               static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), r);
}

// (k + 1/2) 2^-32 for a 32-bit word k: exact in fp64, in (0, 1)
__device__ __forceinline__ double uniform_32(uint32_t k)
{
    return fma(static_cast<double>(k), 0x1.0p-32, 0x1.0p-33);
}

// The two normals of a time step from two words, each by inversion (svmc_math.h normal_icdf32)
__device__ __forceinline__ void normals_from_words(uint32_t ra, uint32_t rb, const RngTables &t, double &w0, double &w1)
{
    w0 = normal_icdf32<SVMC_ICDF_M, SVMC_ICDF_SEGMENTS, SVMC_ICDF_DEG, SVMC_ICDF_EDGE != 0, SVMC_ICDF_RAW != 0>(ra, t.icdf);
    w1 = normal_icdf32<SVMC_ICDF_M, SVMC_ICDF_SEGMENTS, SVMC_ICDF_DEG, SVMC_ICDF_EDGE != 0, SVMC_ICDF_RAW != 0>(rb, t.icdf);
}

// The time loop of every on-device-RNG generator: time steps [0, nb) of a lane whose first step has the chain-global
// index step0.  One Philox call serves the two steps 2c, 2c + 1, so the loop runs over CALLS and each half is guarded by
// a wave-uniform (scalar) test -- a slice that starts or ends on an odd step simply uses one half of its edge call,
// and slicing a chain differently never changes which randoms a (path, step) sees.
// step(z0, z1) advances the model by one time step on UNSCALED N(0,1); tick(t) runs once per call, before it, with
// the local index of the call's first step in this range (the progress priorities).
template <class Step, class Tick>
__device__ __forceinline__ void rng_time_loop(const PhiloxLane &lane, uint32_t step0, int nb, const RngTables &tab,
                                              Step &&step, Tick &&tick)
{
    if (nb <= 0) return;
    const uint32_t first = step0, last = step0 + static_cast<uint32_t>(nb) - 1u;
    for (uint32_t c = first >> 1; c <= (last >> 1); ++c) {
        tick(static_cast<int>(2u * c - first));
        uint32_t r[4];
        philox_draw(lane, c, r);
        double z0, z1;
        if (2u * c >= first) {
            normals_from_words(r[0], r[1], tab, z0, z1);
            step(z0, z1);
        }
        if (2u * c + 1u <= last) {
            normals_from_words(r[2], r[3], tab, z0, z1);
            step(z0, z1);
        }
    }
}

template <class Step>
__device__ __forceinline__ void rng_time_loop(const PhiloxLane &lane, uint32_t step0, int nb, const RngTables &tab,
                                              Step &&step)
{
    rng_time_loop(lane, step0, nb, tab, step, [](int) {});
}

// The draw of ONE time step's pair of normals in three pieces (prepare: word -> t and table offset; read: the four
// ds_read_b128; finish: the two cubics), for the loops that keep one pair in flight under the step before it.  normal_icdf32's
// operations on the same operands: the same bits.
struct PairInFlight {
    double t[2];
    IcdfPiece e0[2], e1[2];
};
__device__ __forceinline__ void pair_issue(uint32_t ra, uint32_t rb, const RngTables &tab, PairInFlight &d)
{
    static_assert(SVMC_ICDF_RAW != 0, "the split draw is written for the raw form of the table");
    const uint32_t w[2] = {ra, rb};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        d.t[k] = icdf_lattice_point(w[k]);
        const uint32_t off = (double_hi(d.t[k]) >> (16 - SVMC_ICDF_M)) & ((static_cast<uint32_t>(SVMC_ICDF_SEGMENTS) - 1u) << 4);
        const char *base = reinterpret_cast<const char *>(tab.icdf) + off;
        d.e0[k] = *reinterpret_cast<const IcdfPiece *>(base);
        d.e1[k] = *reinterpret_cast<const IcdfPiece *>(base + 16 * SVMC_ICDF_SEGMENTS);
    }
}
__device__ __forceinline__ void pair_finish(const PairInFlight &d, double &z0, double &z1)
{
    double z[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double a = fabs(d.t[k]);
        double p = fma(d.e1[k].b, a, d.e1[k].a);
        p = fma(p, a, d.e0[k].b);
        p = fma(p, a, d.e0[k].a);
        z[k] = copysign(p, d.t[k]);
    }
    z0 = z[0];
    z1 = z[1];
}

// rng_time_loop with ONE PAIR ahead, for launches of a few waves per SIMD (up to seven; the reference's default 10^5 paths are
// 1.5), where no other wave hides an LDS round trip: the table reads of the next step's two normals are issued before this step
// runs and their cubics evaluated after it, so a wave overlaps its own draw with its own step.  Batching a call's eight reads
// before its cubics instead puts the waves of a CU in a common LDS phase and then a common VALU phase -- LDS time and VALU time
// add (1250 cycles per step at three waves per SIMD, against 620 of issue and 670 of LDS; the forms measured:
// profiles/r06_mid_waves_sweep.json).  The last trip draws a call nobody uses rather than branching inside the trip (a branch
// splits the scheduling region), and the round keys are hoisted out of the time loop (philox_draw<true>).  Same words, same
// operations: the same bits.
// tick(t) is rng_time_loop's: once per call whose steps run, before them, with the local index of the call's first step.
// HOIST_KEYS = false (the full-launch LogSV kernels, eight waves per SIMD: philox_draw's note on their SGPR budget) leaves the
// round keys re-derived in every trip.  There the loop is not for a lone wave's latency: with the pair's four reads landing under
// the wave's own step, of a step's three LDS round trips only the exp-table read is left for the other seven waves to cover.
template <bool HOIST_KEYS = true, class Step, class Tick>
__device__ __forceinline__ void rng_time_loop_pair_ahead(const PhiloxLane &lane, uint32_t step0, int nb, const RngTables &tab,
                                                         Step &&step, Tick &&tick)
{
    if (nb <= 0) return;
    const uint32_t first = step0, last = step0 + static_cast<uint32_t>(nb) - 1u;
    uint32_t c = first >> 1, r[4];
    double a0, a1;
    if (first & 1u) {
        tick(-1);
        philox_draw(lane, c, r);
        normals_from_words(r[2], r[3], tab, a0, a1);
        step(a0, a1);
        ++c;
    }
    const uint32_t c_end = (last + 1u) >> 1;               // the full calls are [c, c_end)
    if (c < c_end) {
        PairInFlight d;
        philox_draw(lane, c, r);
        pair_issue(r[0], r[1], tab, d);
        __builtin_amdgcn_sched_barrier(0);
        for (; c < c_end; ++c) {
            tick(static_cast<int>(2u * c - first));
            double z0, z1;
            pair_finish(d, z0, z1);
            pair_issue(r[2], r[3], tab, d);
            __builtin_amdgcn_sched_barrier(0);
            step(z0, z1);
            pair_finish(d, z0, z1);
            philox_draw<HOIST_KEYS>(lane, c + 1u, r);      // the last trip draws a call nobody uses (no branch in the trip)
            pair_issue(r[0], r[1], tab, d);
            __builtin_amdgcn_sched_barrier(0);
            step(z0, z1);
        }
    }
    if (!(last & 1u)) {
        tick(static_cast<int>(last - first));
        philox_draw(lane, last >> 1, r);
        normals_from_words(r[0], r[1], tab, a0, a1);
        step(a0, a1);
    }
}

template <class Step>
__device__ __forceinline__ void rng_time_loop_pair_ahead(const PhiloxLane &lane, uint32_t step0, int nb, const RngTables &tab,
                                                         Step &&step)
{
    rng_time_loop_pair_ahead(lane, step0, nb, tab, step, [](int) {});
}

// The same idea one level finer, for a step that itself waits on an LDS read (LogSV: the exp table): the step comes in two
// halves, front(z0, z1) -- everything up to and including the ISSUE of its table read -- and back() -- what consumes the
// value.  Between them runs work that does not depend on the state: the cubics of the NEXT step's pair (its reads are older
// than the step's own read, so they have landed when it has), the Philox call after this one, and the issue of the pair after
// that -- whose reads are younger than the step's own, so back() waits for the exp value only (s_waitcnt lgkmcnt(4)) and the
// pair's four reads stay in flight under back() and the next front().  A lone wave thus overlaps its own LDS round trips with
// its own arithmetic, and the waves of a CU cannot fall into a common LDS phase.  Same words, same operations: the same bits.
template <class Front, class Mid, class Back>
__device__ __forceinline__ void rng_time_loop_pipelined(const PhiloxLane &lane, uint32_t step0, int nb, const RngTables &tab,
                                                        Front &&front, Mid &&mid, Back &&back)
{
    if (nb <= 0) return;
    const uint32_t first = step0, last = step0 + static_cast<uint32_t>(nb) - 1u;
    uint32_t c = first >> 1, r[4];
    double a0, a1;
    if (first & 1u) {
        philox_draw(lane, c, r);
        normals_from_words(r[2], r[3], tab, a0, a1);
        front(a0, a1);
        mid();
        back();
        ++c;
    }
    const uint32_t c_end = (last + 1u) >> 1;               // the full calls are [c, c_end)
    if (c < c_end) {
        PairInFlight d;
        double z0, z1;
        philox_draw(lane, c, r);
        pair_issue(r[0], r[1], tab, d);
        pair_finish(d, z0, z1);
        pair_issue(r[2], r[3], tab, d);
        __builtin_amdgcn_sched_barrier(0);
        for (; c < c_end; ++c) {
            front(z0, z1);                                 // step 2c; its table read is now the youngest LDS operation
            __builtin_amdgcn_sched_barrier(0);
            pair_finish(d, z0, z1);                        // the normals of step 2c + 1
            philox_draw<true>(lane, c + 1u, r);            // the last trip draws a call nobody uses (no branch in the trip)
            pair_issue(r[0], r[1], tab, d);                // ... of step 2c + 2: in flight under back() and the next front()
            mid();                                         // what of the step needs neither the table value nor another wave's time
            __builtin_amdgcn_sched_barrier(0);
            back();
            front(z0, z1);                                 // step 2c + 1
            __builtin_amdgcn_sched_barrier(0);
            pair_finish(d, z0, z1);                        // the normals of step 2c + 2
            pair_issue(r[2], r[3], tab, d);                // ... of step 2c + 3
            mid();
            __builtin_amdgcn_sched_barrier(0);
            back();
        }
    }
    if (!(last & 1u)) {
        philox_draw(lane, last >> 1, r);
        normals_from_words(r[0], r[1], tab, a0, a1);
        front(a0, a1);
        mid();
        back();
    }
}

template <class Front, class Back>
__device__ __forceinline__ void rng_time_loop_pipelined(const PhiloxLane &lane, uint32_t step0, int nb, const RngTables &tab,
                                                        Front &&front, Back &&back)
{
    rng_time_loop_pipelined(lane, step0, nb, tab, front, []() {}, back);
}

// the forms of the generators' time loop, by launch size (few_waves_launch() in svmc_kernels.hip picks): full launches run
// rng_time_loop (the LogSV ones rng_time_loop_pair_ahead with un-hoisted keys: logsv_slice_full), the few-waves Heston generators
// rng_time_loop_pair_ahead, the few-waves LogSV ones rng_time_loop_pipelined.
// The values are template arguments of the kernels, part of their symbol names: they stay as they are.
enum GenLoop { GEN_LOOP_FULL = 0, GEN_LOOP_PAIR = 2, GEN_LOOP_PIPE = 4 };
template <int LOOP, class Step>
__device__ __forceinline__ void gen_time_loop(const PhiloxLane &lane, uint32_t step0, int nb, const RngTables &tab, Step &&step)
{
    static_assert(LOOP == GEN_LOOP_FULL || LOOP == GEN_LOOP_PAIR, "the pipelined loop takes the step in halves");
    if constexpr (LOOP == GEN_LOOP_PAIR) rng_time_loop_pair_ahead(lane, step0, nb, tab, step);
    else rng_time_loop(lane, step0, nb, tab, step);
}

// stream 0 for a single (path, step), from scratch: the step's two UNSCALED N(0,1)  (svmc_fill_normals)
__device__ __forceinline__ void draw_normals(uint64_t seed, uint32_t c3, uint64_t path, uint32_t step,
                                             const RngTables &t, double &w0, double &w1)
{
    uint32_t r[4];
    philox_draw(seed, c3, path, step >> 1, r);
    const bool odd = (step & 1u) != 0u;
    normals_from_words(odd ? r[2] : r[0], odd ? r[3] : r[1], t, w0, w1);
}

// Heston QE (streams 4 and 5).  The scheme needs two normals every step (z0 for the log-price, z1 for the quadratic branch)
// and a uniform only in the exponential branch: the normals come from stream 4 exactly like stream 0's (one call per two
// steps, rng_time_loop), the uniforms from stream 5 -- word step & 3 of call step >> 2, i.e. one call per FOUR steps --
// drawn LAZILY: only when some lane of the wave is in the exponential branch at that step (a wave-uniform decision, so
// every lane of the wave takes part in the call and keeps its four words for the rest of the group).  A parameter set
// that never leaves the quadratic branch (Feller-satisfying sets on any sane grid) pays 12.5 Philox instructions per
// step instead of 25; one that always does pays 18.75.
struct QeUniforms {
    uint32_t r[4];
    uint32_t group = 0xFFFFFFFFu;      // the call (step >> 2) the words belong to: wave-uniform
};

__device__ __forceinline__ double qe_uniform(const PhiloxLane &lane_u, uint32_t step, QeUniforms &cache)
{
    const uint32_t g = step >> 2;
    if (cache.group != g) {
        philox_draw(lane_u, g, cache.r);
        cache.group = g;
    }
    const uint32_t k = step & 3u;                                     // wave-uniform selects
    const uint32_t w = (k == 0u) ? cache.r[0] : (k == 1u) ? cache.r[1] : (k == 2u) ? cache.r[2] : cache.r[3];
    return uniform_32(w);
}

// stream 1: one uniform in (0,1) with 52 random bits
__device__ __forceinline__ double draw_uniform(uint64_t seed, uint32_t c3, uint64_t path, uint32_t step)
{
    uint32_t r[4];
    philox_draw(seed, c3 | 1u, path, step, r);
    return mantissa_1_2(r[0], r[1]) - (1.0 - 0x1.0p-53);
}

}  // namespace svmc
