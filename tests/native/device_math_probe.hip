// Device build of the fp64 helpers for tests/test_gpu_device_math.py: svmc_math.h, uniform_32 of svmc_rng.h, the complex
// helpers of svmc_complex.h and the Black-76 routines of svmc_black.h, compiled with the product's own flags
// (stochvolmodels_amd.build.flags()) into tests/native/libsvmc_device_probe.so -- stochvolmodels_amd/build.py
// build_device_probe().  Test-only: nothing here is part of libsvmc.so or its C ABI.
//
// Every entry point has the form  int dprobe_<name>(const double *x, double *y, size_t n):  n items, x holding NX doubles
// per item and y receiving NY doubles per item, interleaved (a complex number is {re, im}, a multi-argument function reads
// its arguments one after the other); dprobe_shape_<name> reports NX and NY.  It copies x to the device, runs ONE launch of
// 256-thread blocks whose lanes check i < n, synchronises, copies y back and returns the hipError_t.  The exp, log and
// inverse-CDF tables are staged into LDS by the helpers of svmc_rng.h the stepping kernels use, so the table functions read
// LDS as in production.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "svmc.h"
#include "svmc_black.h"
#include "svmc_complex.h"
#include "svmc_math.h"
#include "svmc_rng.h"

namespace {

using namespace svmc;

constexpr unsigned BLOCK = 256;

enum Tables { NO_TABLE, EXP_TABLE, LOG_TABLE, ICDF_TABLE };

struct Tabs {
    const double *exp;
    const LogTabEntry *log;
    const IcdfPiece *icdf;
};

template <class Op>
__global__ __launch_bounds__(BLOCK) void probe_kernel(const double *__restrict__ x, double *__restrict__ y, size_t n)
{
    Tabs t{nullptr, nullptr, nullptr};
    // staged by every lane of the block before the bounds check: the helpers end in a barrier
    if constexpr (Op::TABLES == EXP_TABLE) {
        __shared__ RngTablesLdsIf<false> none;
        __shared__ double lds_exp[256];
        stage_tables_if<false>(none, lds_exp);
        t.exp = lds_exp;
    } else if constexpr (Op::TABLES == LOG_TABLE) {
        __shared__ LogTabEntry lds_log[512];
        t.log = stage_log_table(lds_log);
    } else if constexpr (Op::TABLES == ICDF_TABLE) {
        __shared__ RngTablesLds lds;
        t.icdf = stage_rng_tables(lds).icdf;
    }
    const size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x;
    if (i >= n) return;
    Op::run(x + Op::NX * i, y + Op::NY * i, t);
}

template <class Op>
int launch(const double *x, double *y, size_t n)
{
    if (n == 0) return hipSuccess;
    if (n > static_cast<size_t>(BLOCK) * 0x7fffffffu) return hipErrorInvalidValue;
    double *dx = nullptr, *dy = nullptr;
    hipError_t e = hipMalloc(&dx, Op::NX * n * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&dy, Op::NY * n * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(dx, x, Op::NX * n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(probe_kernel<Op>, dim3(static_cast<unsigned>((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, 0, dx, dy, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(y, dy, Op::NY * n * sizeof(double), hipMemcpyDeviceToHost);
    if (dx) (void)hipFree(dx);
    if (dy) (void)hipFree(dy);
    return static_cast<int>(e);
}

// a 32-bit word carried exactly in a double
__device__ __forceinline__ uint32_t word(double w) { return static_cast<uint32_t>(w); }
__device__ __forceinline__ cd load_cd(const double *p) { return cd{p[0], p[1]}; }
__device__ __forceinline__ void store_cd(double *p, cd z)
{
    p[0] = z.re;
    p[1] = z.im;
}

#define UNARY(NAME, TAB, EXPR)                                                               \
    struct Op_##NAME {                                                                       \
        static constexpr int TABLES = TAB, NX = 1, NY = 1;                                   \
        __device__ static void run(const double *x, double *y, const Tabs &t)                \
        {                                                                                    \
            (void)t;                                                                         \
            const double a = x[0];                                                           \
            y[0] = (EXPR);                                                                   \
        }                                                                                    \
    };

UNARY(exp, NO_TABLE, exp_fast(a))
UNARY(exp_full, NO_TABLE, exp_full(a))
UNARY(exp_tab, EXP_TABLE, exp_tab(a, t.exp))
UNARY(exp2u_tab, EXP_TABLE, exp2u_tab(a, t.exp))
UNARY(neg_log, NO_TABLE, neg_log(a))
UNARY(neg_log_tab, LOG_TABLE, neg_log_tab(a, t.log))
UNARY(log_state, NO_TABLE, log_state(a))
UNARY(sqrt_pos, NO_TABLE, sqrt_pos(a))
UNARY(sqrt_pos_1g, NO_TABLE, sqrt_pos_1g(a))
UNARY(sqrt_pos0, NO_TABLE, sqrt_pos0(a))
UNARY(sqrt_pos0_1g, NO_TABLE, sqrt_pos0_1g(a))
UNARY(rcp_fast, NO_TABLE, rcp_fast(a))
UNARY(rcp_1n, NO_TABLE, rcp_1n(a))
UNARY(rcp_seed, NO_TABLE, rcp_seed(a))
UNARY(rsq_seed, NO_TABLE, rsq_seed(a))
UNARY(uniform_32, NO_TABLE, uniform_32(word(a)))
UNARY(normal_icdf32, ICDF_TABLE,
      (normal_icdf32<SVMC_ICDF_M, SVMC_ICDF_SEGMENTS, SVMC_ICDF_DEG, SVMC_ICDF_EDGE != 0, SVMC_ICDF_RAW != 0>(word(a), t.icdf)))

// sqrt_pos_1g_h: y = {sqrt, half_rsq}
struct Op_sqrt_pos_1g_h {
    static constexpr int TABLES = NO_TABLE, NX = 1, NY = 2;
    __device__ static void run(const double *x, double *y, const Tabs &)
    {
        double h;
        y[0] = sqrt_pos_1g_h(x[0], h);
        y[1] = h;
    }
};

// exp2u_tab in its three pieces, as the several-states-per-lane kernels call it
struct Op_exp2u_split {
    static constexpr int TABLES = EXP_TABLE, NX = 1, NY = 1;
    __device__ static void run(const double *x, double *y, const Tabs &t)
    {
        int ni;
        double r;
        exp2u_reduce(x[0], ni, r);
        const double tv = t.exp[ni & 255];
        y[0] = exp2u_scale(tv, exp2u_tail(r), ni);
    }
};

// the same with the tail's coefficients in vector registers (exp2u_tail_v)
struct Op_exp2u_split_v {
    static constexpr int TABLES = EXP_TABLE, NX = 1, NY = 1;
    __device__ static void run(const double *x, double *y, const Tabs &t)
    {
        const Exp2uTailV c = exp2u_tail_consts();
        int ni;
        double r;
        exp2u_reduce(x[0], ni, r);
        const double tv = t.exp[ni & 255];
        y[0] = exp2u_scale(tv, exp2u_tail_v(r, c), ni);
    }
};

#define COMPLEX_UNARY(NAME, NOUT, BODY)                                                      \
    struct Op_##NAME {                                                                       \
        static constexpr int TABLES = NO_TABLE, NX = 2, NY = NOUT;                           \
        __device__ static void run(const double *x, double *y, const Tabs &)                 \
        {                                                                                    \
            const cd z = load_cd(x);                                                         \
            BODY;                                                                            \
        }                                                                                    \
    };

COMPLEX_UNARY(cabs, 1, y[0] = cabs_(z))
COMPLEX_UNARY(cexp, 2, store_cd(y, cexp_(z)))
COMPLEX_UNARY(csqrt, 2, store_cd(y, csqrt_(z)))
COMPLEX_UNARY(clog, 2, store_cd(y, clog_(z)))

// x = {a.re, a.im, b.re, b.im}: y = a / b
struct Op_cdiv {
    static constexpr int TABLES = NO_TABLE, NX = 4, NY = 2;
    __device__ static void run(const double *x, double *y, const Tabs &) { store_cd(y, load_cd(x) / load_cd(x + 2)); }
};

// x = {F, K, sqrt_t, vol, is_call}: y = {price, vega, d1 d2}
struct Op_black_undisc {
    static constexpr int TABLES = NO_TABLE, NX = 5, NY = 3;
    __device__ static void run(const double *x, double *y, const Tabs &)
    {
        y[0] = black_undisc(x[0], x[1], x[2], x[3], x[4] != 0.0, &y[1], &y[2]);
    }
};

// x = {price, K, option type code (SVMC_CALL .. SVMC_INV_PUT), F, ttm, discfactor, vol_lo, vol_hi}: y = implied vol, the
// quote as chain_implied_vols_kernel (svmc_kernels.hip) hands it to the solver
struct Op_black_implied_vol {
    static constexpr int TABLES = NO_TABLE, NX = 8, NY = 1;
    __device__ static void run(const double *x, double *y, const Tabs &)
    {
        const int code = static_cast<int>(x[2]);
        const bool call = code == SVMC_CALL || code == SVMC_INV_CALL;
        y[0] = black_implied_vol(code >= SVMC_INV_CALL ? x[0] * x[3] : x[0], x[1], call, x[3], x[4], x[5], x[6], x[7]);
    }
};

// x = {s, s2, cnt, shift, discfactor, n_path_total}: y = {price, stderr}
struct Op_payoff_finalize_one {
    static constexpr int TABLES = NO_TABLE, NX = 6, NY = 2;
    __device__ static void run(const double *x, double *y, const Tabs &)
    {
        payoff_finalize_one(x[0], x[1], x[2], x[3], x[4], x[5], &y[0], &y[1]);
    }
};

}  // namespace

// dprobe_shape_<name>(nx, ny): the doubles per item the entry point reads and writes, so that the caller sizes its arrays by them
#define EXPORT(NAME)                                                                                                          \
    extern "C" __attribute__((visibility("default"))) int dprobe_##NAME(const double *x, double *y, size_t n)              \
    {                                                                                                                         \
        return launch<Op_##NAME>(x, y, n);                                                                                    \
    }                                                                                                                         \
    extern "C" __attribute__((visibility("default"))) void dprobe_shape_##NAME(int *nx, int *ny)                          \
    {                                                                                                                         \
        *nx = Op_##NAME::NX;                                                                                                  \
        *ny = Op_##NAME::NY;                                                                                                  \
    }

EXPORT(exp)
EXPORT(exp_full)
EXPORT(exp_tab)
EXPORT(exp2u_tab)
EXPORT(exp2u_split)
EXPORT(exp2u_split_v)
EXPORT(neg_log)
EXPORT(neg_log_tab)
EXPORT(log_state)
EXPORT(sqrt_pos)
EXPORT(sqrt_pos_1g)
EXPORT(sqrt_pos_1g_h)
EXPORT(sqrt_pos0)
EXPORT(sqrt_pos0_1g)
EXPORT(rcp_fast)
EXPORT(rcp_1n)
EXPORT(rcp_seed)
EXPORT(rsq_seed)
EXPORT(uniform_32)
EXPORT(normal_icdf32)
EXPORT(cabs)
EXPORT(cexp)
EXPORT(csqrt)
EXPORT(clog)
EXPORT(cdiv)
EXPORT(black_undisc)
EXPORT(black_implied_vol)
EXPORT(payoff_finalize_one)
