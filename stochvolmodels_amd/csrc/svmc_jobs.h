// svmc_jobs.h -- where a whole-chain generator body's job comes from (svmc_kernels.hip: LogSV; svmc_heston.hip): the kernel
// arguments of a one-job launch (ChainArgs) or a row of the many-job device table (ManyTable), and the host side of that table.
// The model constants of a table entry are the family's own: ManyTable::consts finds the family's many_consts_load overload at
// instantiation.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "svmc.h"
#include "svmc_block.h"
#include "svmc_slice.h"

namespace svmc {

// ---- many independent jobs of one chain in ONE stepping launch (svmc_logsv_chain_price_many / svmc_heston_chain_price_many)
// blockIdx.y = job, blockIdx.x = block of that job's n paths; path p of job j draws philox_prepare(seed_j, c3_j, path_offset + p)
// and runs the body of the one-job kernels from the start state (0, vol0_j, 0), so job j's snapshots and per-wave
// spot partials are those of a single call with (seed_j, call_id_j), bit for bit.  Outputs go to row j m + i (expiry i of job j)
// in the set-major layout of logsv_chain_rng_sets_kernel: ONE payoff launch (blockIdx.z = job) and ONE finish launch serve
// every job.  The terminal state is not written back (no job owns the session's state arrays).
constexpr int MAX_MANY_JOBS = SVMC_MANY_MAX_JOBS;
struct ManySlices {
    double forward[MAX_CHAIN_SLICES];
    int nb_steps[MAX_CHAIN_SLICES];
    int m, total_steps = 0;
};
// the per-job device table, one upload per call: the (job, expiry) constants [J][m] (LogsvFast, or HestonManyConsts),
// then per job the start vol (variance for Heston), the Philox key and the call id's counter word
struct ManyJobs {
    const void *consts;
    const double *vol0;
    const uint64_t *seed;
    const uint32_t *c3;
};

// a job-uniform value read from the job table, word by word into scalar registers: the step takes its constants as scalar
// operands (fma_k's "s" constraint), which a table load the compiler issued as a vector load would not satisfy
template <class T>
__device__ __forceinline__ T uniform_load(const T *p)
{
    static_assert(sizeof(T) % 4 == 0, "whole 32-bit words");
    uint32_t w[sizeof(T) / 4];
    memcpy(w, p, sizeof(T));
#pragma unroll
    for (int k = 0; k < static_cast<int>(sizeof(T) / 4); ++k) w[k] = __builtin_amdgcn_readfirstlane(w[k]);
    T out;
    memcpy(&out, w, sizeof(T));
    return out;
}

// Where a whole-chain body's job comes from.  The LogSV and Heston chain bodies are written once over a job source and run the
// same statements -- hence give the same bits -- whichever one hands them the job:
//   ChainArgs<Slices>   the one-job kernels: everything is a kernel argument (Slices = ChainSlices | HestonChainSlices); the path
//                       starts from `init` or the state arrays at step `step_offset` of its stream, expiry i goes to row i, and
//                       the terminal state is written back
//   ManyTable<Consts>   the many-job kernels: job blockIdx.y of the device table (Consts = LogsvFast | HestonManyConsts); the path
//                       starts from (0, vol0_j, 0) at step 0, expiry i goes to row j m + i, nothing is written back
template <class Slices>
struct ChainArgs {
    const Slices &cs;
    uint64_t seed_;
    uint32_t c3_, step_offset;
    const StateInit &init;
    double *__restrict__ x, *__restrict__ vol, *__restrict__ qvar;

    __device__ __forceinline__ int m() const { return cs.m; }
    __device__ __forceinline__ int nb_steps(int i) const { return cs.nb_steps[i]; }
    __device__ __forceinline__ int total_steps() const { return cs.total_steps; }
    __device__ __forceinline__ double forward(int i) const { return cs.forward[i]; }
    __device__ __forceinline__ auto consts(int i) const { return cs.consts(i); }
    __device__ __forceinline__ uint64_t seed() const { return seed_; }
    __device__ __forceinline__ uint32_t c3() const { return c3_; }
    __device__ __forceinline__ uint32_t step_origin() const { return step_offset; }
    __device__ __forceinline__ size_t row(int i) const { return static_cast<size_t>(i); }
    // (the lanes past the last path get the uniform start too, or a dummy state: the LogSV bodies step them)
    __device__ __forceinline__ void start(size_t p, bool active, double &xv, double &v, double &q) const
    {
        xv = 0.0;
        v = 1.0;
        q = 0.0;
        if (init.uniform) {                               // wave-uniform
            xv = init.x0;
            v = init.vol0;
            q = init.qvar0;
        } else if (active) {
            xv = x[p];
            v = vol[p];
            q = qvar[p];
        }
    }
    __device__ __forceinline__ void finish(size_t p, double xv, double v, double q) const
    {
        x[p] = xv;
        vol[p] = v;
        qvar[p] = q;
    }
};

template <class Consts>
struct ManyTable {
    const ManySlices &cs;
    const ManyJobs &jobs;

    __device__ __forceinline__ int job() const { return blockIdx.y; }
    __device__ __forceinline__ int m() const { return cs.m; }
    __device__ __forceinline__ int nb_steps(int i) const { return cs.nb_steps[i]; }
    __device__ __forceinline__ int total_steps() const { return cs.total_steps; }
    __device__ __forceinline__ double forward(int i) const { return cs.forward[i]; }
    __device__ __forceinline__ Consts consts(int i) const
    {
        const Consts *__restrict__ cj = static_cast<const Consts *>(jobs.consts) + static_cast<size_t>(job()) * cs.m;
        return many_consts_load(cj + i);
    }
    __device__ __forceinline__ uint64_t seed() const { return uniform_load(jobs.seed + job()); }
    __device__ __forceinline__ uint32_t c3() const { return uniform_load(jobs.c3 + job()); }
    __device__ __forceinline__ uint32_t step_origin() const { return 0u; }
    __device__ __forceinline__ size_t row(int i) const { return static_cast<size_t>(job()) * cs.m + i; }
    __device__ __forceinline__ void start(size_t, bool, double &xv, double &v, double &q) const
    {
        xv = 0.0;
        v = uniform_load(jobs.vol0 + job());
        q = 0.0;
    }
    __device__ __forceinline__ void finish(size_t, double, double, double) const {}
};

// ---- the host side of the table

// bytes of the table many_table<Consts> fills for n_jobs jobs of n_slices expiries
template <class Consts>
size_t many_table_bytes_of(int n_jobs, int n_slices)
{
    const size_t J = static_cast<size_t>(n_jobs);
    return J * static_cast<size_t>(n_slices) * sizeof(Consts) + J * (sizeof(double) + sizeof(uint64_t) + sizeof(uint32_t));
}

// fills the pinned table_host (the table's byte layout, constants of CONSTS each), queues its upload and returns the device view
template <class Consts, class Fill>
ManyJobs many_table(int n_jobs, int n_slices, const uint64_t *seeds, const uint32_t *call_ids, void *table_host, void *table_dev,
                    hipStream_t stream, Fill &&fill, hipError_t &err)
{
    const size_t J = static_cast<size_t>(n_jobs), nc = J * static_cast<size_t>(n_slices);
    unsigned char *h = static_cast<unsigned char *>(table_host);
    Consts *consts = reinterpret_cast<Consts *>(h);
    double *vol0 = reinterpret_cast<double *>(h + nc * sizeof(Consts));
    uint64_t *seed = reinterpret_cast<uint64_t *>(vol0 + J);
    uint32_t *c3 = reinterpret_cast<uint32_t *>(seed + J);
    for (int j = 0; j < n_jobs; ++j) {
        vol0[j] = fill(j, consts + static_cast<size_t>(j) * n_slices);
        seed[j] = seeds[j];
        c3[j] = make_c3(call_ids[j]);
    }
    const size_t bytes = reinterpret_cast<unsigned char *>(c3 + J) - h;
    err = hipMemcpyAsync(table_dev, table_host, bytes, hipMemcpyHostToDevice, stream);
    const unsigned char *d = static_cast<const unsigned char *>(table_dev);
    const size_t o_vol = nc * sizeof(Consts), o_seed = o_vol + J * sizeof(double), o_c3 = o_seed + J * sizeof(uint64_t);
    return ManyJobs{d, reinterpret_cast<const double *>(d + o_vol), reinterpret_cast<const uint64_t *>(d + o_seed),
                    reinterpret_cast<const uint32_t *>(d + o_c3)};
}

}  // namespace svmc
