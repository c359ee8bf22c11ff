// svmc_heston.hip -- the Heston generators on gfx950 (pricers/heston_pricer.py of the reference; the QE scheme is new): kernels,
// launchers and entry points of one family in one unit.
//
//   heston_rng_kernel / heston_rng_lat_kernel            one slice on the on-device Philox stream, full-launch / few-waves form,
//                                                        per kernel scheme (Euler with the reference's floor, QE, QE quadratic only)
//   heston_chain_rng_kernel / _lat_kernel                all expiries of a chain in one stepping launch
//   heston_chain_rng_many_kernel / _many_lat_kernel      the same body for J independent jobs (blockIdx.y = job)
//   heston_w_kernel, heston_qe_w_kernel                  the streamed-randoms forms
//
// None of them takes the clock probe.
#include "svmc_internal.h"

#include "svmc_block.h"
#include "svmc_jobs.h"
#include "svmc_models.h"
#include "svmc_rng.h"
#include "svmc_slice.h"

namespace svmc {

// ---------------------------------------------------------------------------------------------------
// Heston generators (pricers/heston_pricer.py:334-381; QE is new)
// ---------------------------------------------------------------------------------------------------
// LOOP: the form of the time loop (svmc_rng.h GenLoop): the full-launch kernels run GEN_LOOP_FULL, the few-waves ones GEN_LOOP_PAIR
// kernel-template scheme ids: the C ABI's two (SVMC_HESTON_EULER_FLOOR = 0, SVMC_HESTON_QE = 1) and QE specialised at compile
// time for parameter sets that never leave the quadratic branch and keep the martingale correction defined (QeConsts::quad_only
// && e_below_one; heston_qe_step<true>) -- the host picks it, the caller never sees it
constexpr int HESTON_QE_QUAD = 2;
constexpr bool heston_is_qe(int scheme) { return scheme == SVMC_HESTON_QE || scheme == HESTON_QE_QUAD; }
static inline int heston_kernel_scheme(int scheme, const QeConsts &qc)
{
    return (scheme == SVMC_HESTON_QE && qc.quad_only && qc.e_below_one) ? HESTON_QE_QUAD : scheme;
}

// a (job, expiry) entry of the table.  Heston's: the constants of one slice, also what a one-job source hands the Heston body
struct HestonManyConsts {
    HestonConsts c;
    QeConsts qc;
};
// ... read by the plain load: Heston's step has no scalar-operand constraint and the compiler issues the load of a job-uniform
// address as scalar loads on its own (forced through uniform_load the Heston kernels spill to scratch)
__device__ __forceinline__ HestonManyConsts many_consts_load(const HestonManyConsts *p) { return *p; }

template <int LOOP, class Step>
__device__ __forceinline__ void heston_time_loop(const PhiloxLane &lane, uint32_t step0, int nb, const RngTables &tab, Step &&step)
{
    gen_time_loop<LOOP>(lane, step0, nb, tab, step);
}

// ONE slice of a Heston path, the statements every on-device-RNG Heston generator runs (heston_rng_body, heston_chain_rng_body):
// nb steps from step `step` of the lane's stream, then the slice's fold into (x, v, q).  lane_u and uc serve SVMC_HESTON_QE's
// uniforms and are dead in the other schemes.
template <int SCHEME, int LOOP>
__device__ __forceinline__ void heston_slice(const PhiloxLane &lane, const PhiloxLane &lane_u, QeUniforms &uc, uint32_t step, int nb,
                                             const RngTables &tab, const HestonConsts c, const QeConsts qc, double &xv, double &v, double &q)
{
    const HestonEulerFast ef = make_heston_euler_fast(c);
    double xacc = 0.0, vacc = 0.0;
    if constexpr (SCHEME == HESTON_QE_QUAD) {
        double vsum = 0.0, ksum = 0.0;
        const double v_first = v;
        const QeVec qv = make_qe_vec(qc);
        heston_time_loop<LOOP>(lane, step, nb, tab, [&](double w0, double w1) {
            heston_qe_step<true>(qc, qv, tab.log, xv, v, vsum, ksum, w0, w1, []() { return 0.0; });
        });
        heston_qe_fold(qc, xv, q, vsum, ksum, v_first, v);
    } else if constexpr (SCHEME == SVMC_HESTON_QE) {
        double vsum = 0.0, ksum = 0.0;
        const double v_first = v;
        uint32_t st = step;
        const QeVec qv = make_qe_vec(qc);
        heston_time_loop<LOOP>(lane, step, nb, tab, [&](double w0, double w1) {
            heston_qe_step(qc, qv, tab.log, xv, v, vsum, ksum, w0, w1, [&]() { return qe_uniform(lane_u, st, uc); });
            ++st;
        });
        heston_qe_fold(qc, xv, q, vsum, ksum, v_first, v);
    } else {
        v = heston_euler_guard_zero(v);
        heston_time_loop<LOOP>(lane, step, nb, tab, [&](double w0, double w1) { heston_euler_step_acc(ef, xacc, v, vacc, w0, w1); });
        heston_fold_acc(ef, xv, q, v, xacc, vacc);
    }
}

template <int SCHEME, int LOOP>
__device__ __forceinline__ void heston_rng_body(double *__restrict__ x, double *__restrict__ var, double *__restrict__ qvar, size_t n,
                                                int nb_steps, HestonConsts c, QeConsts qc, uint64_t seed, uint32_t c3,
                                                uint64_t path_offset, uint32_t step_offset, SliceOut so, StateInit init)
{
    __shared__ RngTablesLds s_tab;
    __shared__ LogTabEntry s_log[heston_is_qe(SCHEME) ? 512 : 1];
    RngTables tab;
    if constexpr (heston_is_qe(SCHEME)) tab = stage_rng_log_tables(s_tab, s_log);
    else tab = stage_rng_tables(s_tab);
    const size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool active = p < n;
    double xv = 0.0, v = 1.0, q = 0.0;
    if (active) {
        if (init.uniform) {                                // wave-uniform
            xv = init.x0;
            v = init.vol0;
            q = init.qvar0;
        } else {
            xv = x[p];
            v = var[p];
            q = qvar[p];
        }
        const PhiloxLane lane = philox_prepare(seed, heston_is_qe(SCHEME) ? (c3 | 4u) : c3, path_offset + p);
        const PhiloxLane lane_u = philox_prepare(seed, c3 | 5u, path_offset + p);  // QE's uniforms (dead in the other schemes)
        QeUniforms uc;
        heston_slice<SCHEME, LOOP>(lane, lane_u, uc, step_offset, nb_steps, tab, c, qc, xv, v, q);
        x[p] = xv;
        var[p] = v;
        qvar[p] = q;
    }
    slice_epilogue(so, p, active, xv, q);
}

template <int SCHEME>
__global__ __launch_bounds__(RNG_BLOCK) void heston_rng_kernel(double *__restrict__ x, double *__restrict__ var,
                                                           double *__restrict__ qvar, size_t n, int nb_steps,
                                                           HestonConsts c, QeConsts qc, uint64_t seed,
                                                           uint32_t c3, uint64_t path_offset,
                                                           uint32_t step_offset, SliceOut so, StateInit init)
{
    heston_rng_body<SCHEME, GEN_LOOP_FULL>(x, var, qvar, n, nb_steps, c, qc, seed, c3, path_offset, step_offset, so, init);
}

// the same generator for a launch of a few waves per SIMD (few_waves_launch(); the reference's default is 10^5 paths): the
// statements -- and the bits -- of heston_rng_kernel, compiled for latency (see logsv_rng_lat_kernel)
template <int SCHEME, int LOOP, int WAVES, int TB>
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void heston_rng_lat_kernel(
    double *__restrict__ x, double *__restrict__ var, double *__restrict__ qvar, size_t n, int nb_steps, HestonConsts c, QeConsts qc,
    uint64_t seed, uint32_t c3, uint64_t path_offset, uint32_t step_offset, SliceOut so, StateInit init)
{
    heston_rng_body<SCHEME, LOOP>(x, var, qvar, n, nb_steps, c, qc, seed, c3, path_offset, step_offset, so, init);
}

// whole-chain variant, as logsv_chain_rng_kernel: the slice loop inside the kernel, one launch tail per chain
struct HestonChainSlices {
    HestonConsts c[MAX_CHAIN_SLICES];
    QeConsts qc[MAX_CHAIN_SLICES];
    double forward[MAX_CHAIN_SLICES];
    int nb_steps[MAX_CHAIN_SLICES];
    int m;
    __device__ __forceinline__ HestonManyConsts consts(int i) const { return {c[i], qc[i]}; }
};

// the body of the whole-chain kernels over a job source (ChainArgs<HestonChainSlices>: one job from the kernel arguments;
// ManyTable<HestonManyConsts>: job blockIdx.y of the many-job table, see logsv_chain_rng_many_kernel)
template <int SCHEME, int LOOP, class Source>
__device__ __forceinline__ void heston_chain_rng_body(size_t n, const Source &src, uint64_t path_offset, double *__restrict__ x_snap,
                                                      double *__restrict__ q_snap, double *__restrict__ partials)
{
    __shared__ RngTablesLds s_tab;
    __shared__ LogTabEntry s_log[heston_is_qe(SCHEME) ? 512 : 1];
    RngTables tab;
    if constexpr (heston_is_qe(SCHEME)) tab = stage_rng_log_tables(s_tab, s_log);
    else tab = stage_rng_tables(s_tab);
    const size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool active = p < n;
    double xv, v, q;
    src.start(p, active, xv, v, q);
    const uint64_t seed = src.seed();
    const uint32_t c3 = src.c3();
    const PhiloxLane lane = philox_prepare(seed, heston_is_qe(SCHEME) ? (c3 | 4u) : c3, path_offset + p);
    const PhiloxLane lane_u = philox_prepare(seed, c3 | 5u, path_offset + p);      // QE's uniforms (dead in the other schemes)
    QeUniforms uc;
    uint32_t step = src.step_origin();
    for (int i = 0; i < src.m(); ++i) {
        const int nb = src.nb_steps(i);
        if (active) {
            const HestonManyConsts k = src.consts(i);
            heston_slice<SCHEME, LOOP>(lane, lane_u, uc, step, nb, tab, k.c, k.qc, xv, v, q);
        }
        step += static_cast<uint32_t>(nb);
        slice_epilogue(slice_out_row(x_snap, q_snap, partials, src.row(i), n, src.forward(i)), p, active, xv, q);
    }
    if (active) src.finish(p, xv, v, q);
}

template <int SCHEME>
__global__ __launch_bounds__(RNG_BLOCK) void heston_chain_rng_kernel(double *__restrict__ x, double *__restrict__ var,
                                                                 double *__restrict__ qvar, size_t n,
                                                                 HestonChainSlices cs, uint64_t seed, uint32_t c3,
                                                                 uint64_t path_offset, uint32_t step_offset,
                                                                 double *__restrict__ x_snap, double *__restrict__ q_snap,
                                                                 double *__restrict__ partials, StateInit init)
{
    heston_chain_rng_body<SCHEME, GEN_LOOP_FULL>(n, ChainArgs<HestonChainSlices>{cs, seed, c3, step_offset, init, x, var, qvar}, path_offset,
                                                 x_snap, q_snap, partials);
}

template <int SCHEME, int LOOP, int WAVES, int TB>
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void heston_chain_rng_lat_kernel(
    double *__restrict__ x, double *__restrict__ var, double *__restrict__ qvar, size_t n, HestonChainSlices cs, uint64_t seed,
    uint32_t c3, uint64_t path_offset, uint32_t step_offset, double *__restrict__ x_snap, double *__restrict__ q_snap,
    double *__restrict__ partials, StateInit init)
{
    heston_chain_rng_body<SCHEME, LOOP>(n, ChainArgs<HestonChainSlices>{cs, seed, c3, step_offset, init, x, var, qvar}, path_offset, x_snap,
                                        q_snap, partials);
}

// many jobs of one chain in one launch: the same body on job blockIdx.y of the table
template <int SCHEME>
__global__ __launch_bounds__(RNG_BLOCK) void heston_chain_rng_many_kernel(size_t n, ManySlices cs, ManyJobs jobs, uint64_t path_offset,
                                                                      double *__restrict__ x_snap, double *__restrict__ q_snap,
                                                                      double *__restrict__ partials)
{
    heston_chain_rng_body<SCHEME, GEN_LOOP_FULL>(n, ManyTable<HestonManyConsts>{cs, jobs}, path_offset, x_snap, q_snap, partials);
}

template <int SCHEME, int LOOP, int WAVES, int TB>
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void heston_chain_rng_many_lat_kernel(
    size_t n, ManySlices cs, ManyJobs jobs, uint64_t path_offset, double *__restrict__ x_snap, double *__restrict__ q_snap,
    double *__restrict__ partials)
{
    heston_chain_rng_body<SCHEME, LOOP>(n, ManyTable<HestonManyConsts>{cs, jobs}, path_offset, x_snap, q_snap, partials);
}

__global__ __launch_bounds__(BLOCK) void heston_w_kernel(double *__restrict__ x, double *__restrict__ var,
                                                         double *__restrict__ qvar, size_t n, int nb_steps,
                                                         HestonConsts c, const double *__restrict__ W0,
                                                         const double *__restrict__ W1, size_t ldw)
{
    const size_t p = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x;
    if (p >= n) return;
    double xv = x[p], v = var[p], q = qvar[p];
    const double *const w[2] = {W0 + p, W1 + p};
    streamed_time_loop<2>(w, ldw, nb_steps, [&](const double(&z)[2]) {
        heston_euler_step(c, xv, v, q, c.sdt * z[0], c.sdt * z[1]);
    });
    x[p] = xv;
    var[p] = v;
    qvar[p] = q;
}

__global__ __launch_bounds__(BLOCK) void heston_qe_w_kernel(double *__restrict__ x, double *__restrict__ var,
                                                            double *__restrict__ qvar, size_t n, int nb_steps,
                                                            QeConsts qc, const double *__restrict__ Z0,
                                                            const double *__restrict__ Z1,
                                                            const double *__restrict__ U, size_t ldw)
{
    __shared__ LogTabEntry s_tab[512];
    const LogTabEntry *tab = stage_log_table(s_tab);
    const size_t p = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x;
    if (p >= n) return;
    double xv = x[p], v = var[p], q = qvar[p], vsum = 0.0, ksum = 0.0;
    const double v_first = v;
    const double *const w[3] = {Z0 + p, Z1 + p, U + p};
    const QeVec qv = make_qe_vec(qc);
    streamed_time_loop<3>(w, ldw, nb_steps, [&](const double(&z)[3]) {
        heston_qe_step(qc, qv, tab, xv, v, vsum, ksum, z[0], z[1], [&]() { return z[2]; });
    });
    heston_qe_fold(qc, xv, q, vsum, ksum, v_first, v);
    x[p] = xv;
    var[p] = v;
    qvar[p] = q;
}

}  // namespace svmc

using namespace svmc;

extern "C" {

// the few-waves forms of the Heston generators, per kernel scheme id (the forms they were measured against:
// profiles/r06_mid_waves_sweep.json).  The Euler step has no LDS read of its own, so one pair ahead hides the draw's round trip
// completely; QE (100 registers by itself) runs the same loop at the 128-register budget.
using HestonSliceKernel = void (*)(double *, double *, double *, size_t, int, HestonConsts, QeConsts, uint64_t, uint32_t, uint64_t, uint32_t,
                                   SliceOut, StateInit);
using HestonChainKernel = void (*)(double *, double *, double *, size_t, HestonChainSlices, uint64_t, uint32_t, uint64_t, uint32_t, double *,
                                   double *, double *, StateInit);
struct HestonLatVariant {
    HestonSliceKernel slice;
    HestonChainKernel chain;
    int block;
};
#define SVMC_HESTON_LAT(S, WAVES) \
    {heston_rng_lat_kernel<S, GEN_LOOP_PAIR, WAVES, FEW_BLOCK>, heston_chain_rng_lat_kernel<S, GEN_LOOP_PAIR, WAVES, FEW_BLOCK>, FEW_BLOCK}
static const HestonLatVariant HESTON_FEW_WAVES_KERNELS[3] = {
    SVMC_HESTON_LAT(SVMC_HESTON_EULER_FLOOR, 4),           // Euler with the reference's floor
    SVMC_HESTON_LAT(SVMC_HESTON_QE, 3),                    // QE
    SVMC_HESTON_LAT(HESTON_QE_QUAD, 4)};                   // QE, quadratic branch only
#undef SVMC_HESTON_LAT

// the full-launch kernels, per kernel scheme id (0, 1 or HESTON_QE_QUAD)
static const HestonLatVariant HESTON_FULL_KERNELS[3] = {
    {heston_rng_kernel<SVMC_HESTON_EULER_FLOOR>, heston_chain_rng_kernel<SVMC_HESTON_EULER_FLOOR>, RNG_BLOCK},
    {heston_rng_kernel<SVMC_HESTON_QE>, heston_chain_rng_kernel<SVMC_HESTON_QE>, RNG_BLOCK},
    {heston_rng_kernel<HESTON_QE_QUAD>, heston_chain_rng_kernel<HESTON_QE_QUAD>, RNG_BLOCK}};

// -> the kernels a launch of n_path paths of kernel scheme `scheme` runs: a few-waves form or the full-launch ones
static const HestonLatVariant *heston_variant(int scheme, size_t n_path)
{
    return few_waves_launch(n_path) ? &HESTON_FEW_WAVES_KERNELS[scheme] : &HESTON_FULL_KERNELS[scheme];
}

static int heston_rng_launch(const char *fn, double *x, double *var, double *qvar, size_t n_path, int nb_steps, double dt,
                             double theta, double kappa, double rho, double volvol, int scheme, uint64_t seed,
                             uint32_t call_id, uint64_t path_offset, uint32_t step_offset, const SliceOut &so,
                             svmc_stream_t stream, const StateInit &init = StateInit())
{
    if (int rc = check_state(fn, x, var, qvar, nb_steps, dt)) return rc;
    if (scheme != SVMC_HESTON_EULER_FLOOR && scheme != SVMC_HESTON_QE)
        return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": unknown scheme");
    if (call_id >= (1u << 24)) return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": call_id must fit 24 bits");
    if (n_path == 0) return SVMC_OK;
    const HestonConsts c = make_heston_consts(dt, theta, kappa, rho, volvol);
    const QeConsts qc = make_qe_consts(dt, theta, kappa, rho, volvol);
    const HestonLatVariant *v = heston_variant(heston_kernel_scheme(scheme, qc), n_path);
    hipLaunchKernelGGL(v->slice, dim3(lat_grid(n_path, v->block)), dim3(v->block), 0, as_stream(stream), x, var, qvar, n_path, nb_steps, c,
                       qc, seed, make_c3(call_id), path_offset, step_offset, so, init);
    return check_launch(fn);
}

int svmc_heston_terminal_rng(double *x, double *var, double *qvar, size_t n_path, int nb_steps, double dt,
                             double theta, double kappa, double rho, double volvol, int scheme, uint64_t seed,
                             uint32_t call_id, uint64_t path_offset, uint32_t step_offset, svmc_stream_t stream)
{
    const SliceOut none = {nullptr, nullptr, nullptr, 0.0};
    if (nb_steps == 0) return check_state("svmc_heston_terminal_rng", x, var, qvar, nb_steps, dt);
    return heston_rng_launch("svmc_heston_terminal_rng", x, var, qvar, n_path, nb_steps, dt, theta, kappa, rho, volvol,
                             scheme, seed, call_id, path_offset, step_offset, none, stream);
}

}  // extern "C"

static int heston_slice_rng_impl(const char *fn, const StateInit &init, double *x, double *var, double *qvar, size_t n_path, int nb_steps, double dt, double theta,
                          double kappa, double rho, double volvol, int scheme, uint64_t seed, uint32_t call_id,
                          uint64_t path_offset, uint32_t step_offset, double forward, double *x_snapshot,
                          double *qvar_snapshot, double *spot_sums, void *workspace, size_t workspace_bytes,
                          svmc_stream_t stream)
{
    if (int rc = check_slice_args(fn, n_path, x_snapshot, spot_sums, workspace, workspace_bytes, true)) return rc;
    SVMC_REQUIRE(n_path > 0 && nb_steps > 0, std::string(fn) + ": n_path and nb_steps must be positive");
    const SliceOut so = {x_snapshot, qvar_snapshot, static_cast<double *>(workspace), forward, wave_rows(n_path)};
    if (int rc = heston_rng_launch(fn, x, var, qvar, n_path, nb_steps, dt, theta, kappa, rho, volvol, scheme, seed,
                                   call_id, path_offset, step_offset, so, stream, init))
        return rc;
    if (spot_sums == nullptr) return SVMC_OK;
    return reduce_spot_partials(workspace, n_path, 2, spot_sums, as_stream(stream));
}

extern "C" {

int svmc_heston_slice_rng(double *x, double *var, double *qvar, size_t n_path, int nb_steps, double dt, double theta,
                          double kappa, double rho, double volvol, int scheme, uint64_t seed, uint32_t call_id,
                          uint64_t path_offset, uint32_t step_offset, double forward, double *x_snapshot,
                          double *qvar_snapshot, double *spot_sums, void *workspace, size_t workspace_bytes,
                          svmc_stream_t stream)
{
    SVMC_REQUIRE(spot_sums != nullptr, "svmc_heston_slice_rng: null spot_sums");
    return heston_slice_rng_impl("svmc_heston_slice_rng", StateInit(), x, var, qvar, n_path, nb_steps, dt, theta, kappa, rho,
                                 volvol, scheme, seed, call_id, path_offset, step_offset, forward, x_snapshot, qvar_snapshot,
                                 spot_sums, workspace, workspace_bytes, stream);
}

int svmc_heston_slice_rng_from(double x0, double var0, double qvar0, double *x, double *var, double *qvar, size_t n_path,
                               int nb_steps, double dt, double theta, double kappa, double rho, double volvol, int scheme,
                               uint64_t seed, uint32_t call_id, uint64_t path_offset, uint32_t step_offset, double forward,
                               double *x_snapshot, double *qvar_snapshot, double *spot_sums, void *workspace,
                               size_t workspace_bytes, svmc_stream_t stream)
{
    SVMC_REQUIRE(spot_sums != nullptr, "svmc_heston_slice_rng_from: null spot_sums");
    const StateInit init = {1, x0, var0, qvar0};
    return heston_slice_rng_impl("svmc_heston_slice_rng_from", init, x, var, qvar, n_path, nb_steps, dt, theta, kappa, rho,
                                 volvol, scheme, seed, call_id, path_offset, step_offset, forward, x_snapshot, qvar_snapshot,
                                 spot_sums, workspace, workspace_bytes, stream);
}

}  // extern "C"

static int heston_chain_rng_impl(const char *fn, const StateInit &init, double *x, double *var, double *qvar, size_t n_path, int n_slices, const int *nb_steps_host,
                          const double *dts_host, const double *forwards_host, double theta, double kappa, double rho,
                          double volvol, int scheme, uint64_t seed, uint32_t call_id, uint64_t path_offset,
                          uint32_t step_offset, double *x_snapshots, double *qvar_snapshots, double *spot_sums,
                          void *workspace, size_t workspace_bytes, svmc_stream_t stream)
{
    SVMC_REQUIRE(scheme == SVMC_HESTON_EULER_FLOOR || scheme == SVMC_HESTON_QE, std::string(fn) + ": unknown scheme");
    const auto fill = [&](HestonChainSlices &cs, int i, int j) {
        cs.c[i] = make_heston_consts(dts_host[j], theta, kappa, rho, volvol);
        cs.qc[i] = make_qe_consts(dts_host[j], theta, kappa, rho, volvol);
        cs.forward[i] = forwards_host[j];
    };
    const auto launch = [&](const HestonChainSlices &cs, double *xs, double *qs, const StateInit &init_i, uint32_t step0) {
        int ks = scheme;
        if (scheme == SVMC_HESTON_QE) {                    // the specialised kernel only if EVERY slice of the launch allows it
            ks = HESTON_QE_QUAD;
            for (int i = 0; i < cs.m; ++i)
                if (heston_kernel_scheme(scheme, cs.qc[i]) != HESTON_QE_QUAD) ks = scheme;
        }
        const HestonLatVariant *v = heston_variant(ks, n_path);
        hipLaunchKernelGGL(v->chain, dim3(lat_grid(n_path, v->block)), dim3(v->block), 0, as_stream(stream), x, var, qvar, n_path, cs, seed,
                           make_c3(call_id), path_offset, step0, xs, qs, static_cast<double *>(workspace), init_i);
    };
    return step_chain<HestonChainSlices>(fn, init, x, var, qvar, n_path, n_slices, nb_steps_host, dts_host, forwards_host, call_id,
                                         step_offset, x_snapshots, qvar_snapshots, spot_sums, workspace, workspace_bytes,
                                         as_stream(stream), fill, launch);
}

extern "C" {

int svmc_heston_chain_rng(double *x, double *var, double *qvar, size_t n_path, int n_slices, const int *nb_steps_host,
                          const double *dts_host, const double *forwards_host, double theta, double kappa, double rho,
                          double volvol, int scheme, uint64_t seed, uint32_t call_id, uint64_t path_offset,
                          uint32_t step_offset, double *x_snapshots, double *qvar_snapshots, double *spot_sums,
                          void *workspace, size_t workspace_bytes, svmc_stream_t stream)
{
    SVMC_REQUIRE(spot_sums != nullptr, "svmc_heston_chain_rng: null spot_sums");
    return heston_chain_rng_impl("svmc_heston_chain_rng", StateInit(), x, var, qvar, n_path, n_slices, nb_steps_host, dts_host,
                                 forwards_host, theta, kappa, rho, volvol, scheme, seed, call_id, path_offset, step_offset,
                                 x_snapshots, qvar_snapshots, spot_sums, workspace, workspace_bytes, stream);
}

int svmc_heston_chain_rng_from(double x0, double var0, double qvar0, double *x, double *var, double *qvar, size_t n_path,
                               int n_slices, const int *nb_steps_host, const double *dts_host, const double *forwards_host,
                               double theta, double kappa, double rho, double volvol, int scheme, uint64_t seed,
                               uint32_t call_id, uint64_t path_offset, uint32_t step_offset, double *x_snapshots,
                               double *qvar_snapshots, double *spot_sums, void *workspace, size_t workspace_bytes,
                               svmc_stream_t stream)
{
    SVMC_REQUIRE(spot_sums != nullptr, "svmc_heston_chain_rng_from: null spot_sums");
    const StateInit init = {1, x0, var0, qvar0};
    return heston_chain_rng_impl("svmc_heston_chain_rng_from", init, x, var, qvar, n_path, n_slices, nb_steps_host, dts_host,
                                 forwards_host, theta, kappa, rho, volvol, scheme, seed, call_id, path_offset, step_offset,
                                 x_snapshots, qvar_snapshots, spot_sums, workspace, workspace_bytes, stream);
}

int svmc_heston_terminal_w(double *x, double *var, double *qvar, size_t n_path, int nb_steps, double dt,
                           double theta, double kappa, double rho, double volvol, const double *W0,
                           const double *W1, size_t ldw, svmc_stream_t stream)
{
    if (int rc = check_state("svmc_heston_terminal_w", x, var, qvar, nb_steps, dt)) return rc;
    SVMC_REQUIRE(W0 && W1, "svmc_heston_terminal_w: null W0/W1");
    SVMC_REQUIRE(ldw >= n_path, "svmc_heston_terminal_w: ldw < n_path");
    if (n_path == 0 || nb_steps == 0) return SVMC_OK;
    const HestonConsts c = make_heston_consts(dt, theta, kappa, rho, volvol);
    hipLaunchKernelGGL(heston_w_kernel, dim3(grid_for(n_path)), dim3(BLOCK), 0, as_stream(stream), x, var, qvar,
                       n_path, nb_steps, c, W0, W1, ldw);
    return check_launch("svmc_heston_terminal_w");
}

int svmc_heston_qe_terminal_w(double *x, double *var, double *qvar, size_t n_path, int nb_steps, double dt,
                              double theta, double kappa, double rho, double volvol, const double *Z0,
                              const double *Z1, const double *U, size_t ldw, svmc_stream_t stream)
{
    if (int rc = check_state("svmc_heston_qe_terminal_w", x, var, qvar, nb_steps, dt)) return rc;
    SVMC_REQUIRE(Z0 && Z1 && U, "svmc_heston_qe_terminal_w: null Z0/Z1/U");
    SVMC_REQUIRE(ldw >= n_path, "svmc_heston_qe_terminal_w: ldw < n_path");
    if (n_path == 0 || nb_steps == 0) return SVMC_OK;
    const QeConsts qc = make_qe_consts(dt, theta, kappa, rho, volvol);
    hipLaunchKernelGGL(heston_qe_w_kernel, dim3(grid_for(n_path)), dim3(BLOCK), 0, as_stream(stream), x, var, qvar,
                       n_path, nb_steps, qc, Z0, Z1, U, ldw);
    return check_launch("svmc_heston_qe_terminal_w");
}

}  // extern "C"

namespace svmc {

// the stepping of svmc_chain.hip's fused chains from the start state (0, var0, 0): svmc_heston_chain_rng_from, or the slice
// kernel for a single expiry; spot_sums null leaves the per-wave partial columns in `workspace` for the one-device tail
int heston_step_partials(double var0, double *x, double *var, double *qvar, size_t n_path, int n_slices, const int *nb_steps_host,
                         const double *dts_host, const double *forwards_host, double theta, double kappa, double rho, double volvol,
                         int scheme, uint64_t seed, uint32_t call_id, uint64_t path_offset, double *x_snapshots,
                         double *qvar_snapshots, double *spot_sums, void *workspace, size_t workspace_bytes, hipStream_t stream)
{
    const StateInit init = {1, 0.0, var0, 0.0};
    const svmc_stream_t st = reinterpret_cast<svmc_stream_t>(stream);
    if (n_slices == 1)
        return heston_slice_rng_impl("heston_step_partials", init, x, var, qvar, n_path, nb_steps_host[0], dts_host[0], theta, kappa, rho,
                                     volvol, scheme, seed, call_id, path_offset, 0, forwards_host[0], x_snapshots, qvar_snapshots,
                                     spot_sums, workspace, workspace_bytes, st);
    return heston_chain_rng_impl("heston_step_partials", init, x, var, qvar, n_path, n_slices, nb_steps_host, dts_host, forwards_host,
                                 theta, kappa, rho, volvol, scheme, seed, call_id, path_offset, 0, x_snapshots, qvar_snapshots, spot_sums,
                                 workspace, workspace_bytes, st);
}

// ---- many jobs of one chain (svmc_chain.hip's svmc_heston_chain_price_many)

size_t heston_many_table_bytes(int n_jobs, int n_slices) { return many_table_bytes_of<HestonManyConsts>(n_jobs, n_slices); }

using HestonManyKernel = void (*)(size_t, ManySlices, ManyJobs, uint64_t, double *, double *, double *);
#define SVMC_HESTON_MANY_LAT(S, WAVES) heston_chain_rng_many_lat_kernel<S, GEN_LOOP_PAIR, WAVES, FEW_BLOCK>
static const HestonManyKernel HESTON_MANY_FEW_WAVES_KERNELS[3] = {
    SVMC_HESTON_MANY_LAT(SVMC_HESTON_EULER_FLOOR, 4), SVMC_HESTON_MANY_LAT(SVMC_HESTON_QE, 3), SVMC_HESTON_MANY_LAT(HESTON_QE_QUAD, 4)};
#undef SVMC_HESTON_MANY_LAT
static const HestonManyKernel HESTON_MANY_FULL_KERNELS[3] = {
    heston_chain_rng_many_kernel<SVMC_HESTON_EULER_FLOOR>, heston_chain_rng_many_kernel<SVMC_HESTON_QE>,
    heston_chain_rng_many_kernel<HESTON_QE_QUAD>};

int heston_chain_rng_many(size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
                          const double *forwards_host, const double *params_host, int scheme, const uint64_t *seeds,
                          const uint32_t *call_ids, uint64_t path_offset, void *table_host, void *table_dev, double *x_snapshots,
                          double *qvar_snapshots, double *spot_partials, hipStream_t stream)
{
    const char *fn = "heston_chain_rng_many";
    if (int rc = check_many(fn, n_path, n_jobs, n_slices, nb_steps_host, dts_host, call_ids)) return rc;
    SVMC_REQUIRE(scheme == SVMC_HESTON_EULER_FLOOR || scheme == SVMC_HESTON_QE, std::string(fn) + ": unknown scheme");
    // the QE specialisation only if EVERY (job, expiry) of the launch allows it (as heston_chain_rng_impl per launch)
    bool quad = scheme == SVMC_HESTON_QE;
    hipError_t e = hipSuccess;
    const ManyJobs jobs = many_table<HestonManyConsts>(n_jobs, n_slices, seeds, call_ids, table_host, table_dev, stream,
                                                       [&](int j, HestonManyConsts *c) {
        const double *p = params_host + 5 * static_cast<size_t>(j);    // v0 theta kappa rho volvol
        for (int i = 0; i < n_slices; ++i) {
            c[i].c = make_heston_consts(dts_host[i], p[1], p[2], p[3], p[4]);
            c[i].qc = make_qe_consts(dts_host[i], p[1], p[2], p[3], p[4]);
            quad = quad && heston_kernel_scheme(scheme, c[i].qc) == HESTON_QE_QUAD;
        }
        return p[0];
    }, e);
    SVMC_HIP_TRY(e);
    const ManySlices cs = many_slices(n_slices, nb_steps_host, forwards_host);
    const int ks = quad ? HESTON_QE_QUAD : scheme;
    const bool few = few_waves_launch(static_cast<size_t>(n_jobs) * n_path);
    const HestonManyKernel k = few ? HESTON_MANY_FEW_WAVES_KERNELS[ks] : HESTON_MANY_FULL_KERNELS[ks];
    const unsigned block = few ? FEW_BLOCK : RNG_BLOCK;
    hipLaunchKernelGGL(k, dim3(lat_grid(n_path, block), static_cast<unsigned>(n_jobs)), dim3(block), 0, stream, n_path, cs, jobs,
                       path_offset, x_snapshots, qvar_snapshots, spot_partials);
    return check_launch(fn);
}

}  // namespace svmc
