// svmc_rough.hip -- the rough LogSV model's Markovian lift on gfx950 (pricers/rough_logsv/split_simulation.py of the
// reference): its one kernel, the launchers and the entry points in one unit.  The kernel takes no clock probe.
#include "svmc_internal.h"

#include <cmath>
#include <string>
#include "svmc_block.h"
#include "svmc_models.h"
#include "svmc_rng.h"
#include "svmc_slice.h"

namespace svmc {

#ifndef SVMC_ROUGH_STREAM_U
#define SVMC_ROUGH_STREAM_U 4          // A/B hook: prefetch depth of the rough kernel's streamed normals
#endif

// ---------------------------------------------------------------------------------------------------
// Rough LogSV, Markovian lift with N <= 3 factors (pricers/rough_logsv/split_simulation.py:86-128, 228-356):
// Strang splitting D(h/2) S(h) D(h/2) per step -- RK4 on the factor drift, exact lognormal step of the weighted
// factor sum -- then the log-spot / quadratic-variance update.  One lane per path, the N factors in registers.
// ---------------------------------------------------------------------------------------------------
struct RoughConsts {
    double nodes[3], w[3], v0[3], wlam[3];
    double theta, kappa1, kappa2, rho, rho_comp, volvol, inv_volvol, h, inv_h, sqrt_h, wsum, w_inv, volvol_w, w_lam_v0;
    double ito, volvol_w_sqrt_h;   // -0.5 (volvol wsum)^2 h,  volvol wsum sqrt(h)
};

template <int N>
__device__ __forceinline__ void rough_rk4_drift(const RoughConsts &c, const double (&z0)[N], double h, double (&zh)[N])
{
    double s1[N], s2[N], s3[N], s4[N], zt[N], zw, g;
    zw = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) zw += c.w[i] * z0[i];
    g = (c.kappa1 + c.kappa2 * zw) * (c.theta - zw);
#pragma unroll
    for (int i = 0; i < N; ++i) s1[i] = -c.nodes[i] * (z0[i] - c.v0[i]) + g;                         // :101-103
    zw = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        zt[i] = z0[i] + 0.5 * h * s1[i];
        zw += c.w[i] * zt[i];
    }
    g = (c.kappa1 + c.kappa2 * zw) * (c.theta - zw);
#pragma unroll
    for (int i = 0; i < N; ++i) s2[i] = -c.nodes[i] * (zt[i] - c.v0[i]) + g;                         // :106-109
    zw = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        zt[i] = z0[i] + 0.5 * h * s2[i];
        zw += c.w[i] * zt[i];
    }
    g = (c.kappa1 + c.kappa2 * zw) * (c.theta - zw);
#pragma unroll
    for (int i = 0; i < N; ++i) s3[i] = -c.nodes[i] * (zt[i] - c.v0[i]) + g;                         // :112-115
    zw = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        zt[i] = z0[i] + h * s3[i];
        zw += c.w[i] * zt[i];
    }
    g = (c.kappa1 + c.kappa2 * zw) * (c.theta - zw);
#pragma unroll
    for (int i = 0; i < N; ++i) s4[i] = -c.nodes[i] * (zt[i] - c.v0[i]) + g;                         // :118-121
#pragma unroll
    for (int i = 0; i < N; ++i) zh[i] = z0[i] + (h / 6.0) * (s1[i] + 2.0 * s2[i] + 2.0 * s3[i] + s4[i]);
}

template <int N, class Exp>
__device__ __forceinline__ void rough_step(const RoughConsts &c, double (&v)[N], double &ls, double &y, double z0, double z1,
                                           Exp &&exp_of)
{
    double d[N], sn[N], vh[N];
    rough_rk4_drift<N>(c, v, 0.5 * c.h, d);                                                      // :273
    double yw = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) yw += c.w[i] * d[i];
    const double Yh = yw * exp_of(c.ito + c.volvol_w_sqrt_h * z0);   // :238-239
    const double Q = c.w_inv * (Yh - yw);
#pragma unroll
    for (int i = 0; i < N; ++i) sn[i] = d[i] + Q;
    rough_rk4_drift<N>(c, sn, 0.5 * c.h, vh);                                                    // :275
    double volw_h = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) volw_h += c.w[i] * vh[i];
    if (!(volw_h > 0.0)) {                                                                       // NaN or <= 0, :299-300
        volw_h = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            vh[i] = 1e-6;
            volw_h += c.w[i] * vh[i];
        }
    }
    double vw = 0.0, w_lam_vol = 0.0, w_lam_vol_h = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        vw += c.w[i] * v[i];
        w_lam_vol += c.wlam[i] * v[i];
        w_lam_vol_h += c.wlam[i] * vh[i];
    }
    const double sq_vw = vw * vw, sq_vhw = volw_h * volw_h;
    const double term1 = c.inv_volvol * (((volw_h - vw) * c.inv_h + 0.5 * w_lam_vol + 0.5 * w_lam_vol_h - c.w_lam_v0) * c.w_inv
                                         - c.kappa1 * c.theta + (c.kappa1 - c.kappa2 * c.theta) * (0.5 * vw + 0.5 * volw_h)
                                         + c.kappa2 * (0.5 * sq_vw + 0.5 * sq_vhw)) * c.h;       // :319-321
    const double term2 = 0.5 * c.h * sq_vw + 0.5 * c.h * sq_vhw;
    ls = ls - 0.5 * term2 + c.rho * term1 + c.rho_comp * sqrt_pos(term2) * z1;                         // :324
    y = y + 0.5 * c.h * (vw * vw + volw_h * volw_h);                                               // :326
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = vh[i];
}

// ALL expiries of a rough-LogSV chain in ONE launch: the reference re-simulates every expiry from time 0 on its own step
// (pricers/logsv_pricer.py:1206-1216), so the expiries are INDEPENDENT simulations -- blockIdx.y picks one.  A calibration-
// sized path set (4 000-10 000 paths: 63-157 waves) fills a sixteenth of the chip, and m such launches one after the other
// each pay their own latency-bound time loop; side by side they cost the longest one.  Per expiry the arithmetic is
// the same on the same constants (the step-dependent ones travel per expiry).  Snapshot row i / m + i and partial column pair i
// belong to expiry i; the state arrays receive the LAST expiry's terminal state, as the expiry-by-expiry loop leaves them.
// This is the ONLY rough kernel: a single expiry is grid.y = 1, and a continuation from the resident state (from_origin = 0,
// the draw's steps starting at step_offset) is the same launch reading the state first -- so one launch per expiry, all
// expiries in one launch and a run cut into continued halves execute the same code and agree to the bit by construction.
// RNG = false: Z0/Z1 supplied (the reference's only interface for this model); true: counter-based draw.
struct RoughExpiries {
    double h[MAX_CHAIN_SLICES], inv_h[MAX_CHAIN_SLICES], sqrt_h[MAX_CHAIN_SLICES], ito[MAX_CHAIN_SLICES],
        volvol_w_sqrt_h[MAX_CHAIN_SLICES], forward[MAX_CHAIN_SLICES];
    int nb_steps[MAX_CHAIN_SLICES];
    int m;
};

template <int N, bool RNG>
__global__ __launch_bounds__(RNG ? RNG_BLOCK : BLOCK) void rough_logsv_expiries_kernel(
    double *__restrict__ log_s, double *__restrict__ vol, double *__restrict__ yq, size_t n, RoughConsts c, RoughExpiries e,
    const double *__restrict__ Z0, const double *__restrict__ Z1, size_t ldw, uint64_t seed, uint32_t c3, uint64_t path_offset,
    uint32_t step_offset, int from_origin, double *__restrict__ x_snap, double *__restrict__ q_snap, double *__restrict__ partials)
{
    __shared__ RngTablesLdsIf<RNG> s_tab;                  // the draw's table only where the kernel draws
    __shared__ double s_exp[256];
    const RngTables tab = stage_tables_if(s_tab, s_exp);
    const auto exp_of = [&](double a) { return exp_tab(a, s_exp); };
    const int i = blockIdx.y;                              // the expiry: block-uniform
    c.h = e.h[i];
    c.inv_h = e.inv_h[i];
    c.sqrt_h = e.sqrt_h[i];
    c.ito = e.ito[i];
    c.volvol_w_sqrt_h = e.volvol_w_sqrt_h[i];
    const int nb_steps = e.nb_steps[i];
    const size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool active = p < n;
    double ls = 0.0, y = 0.0;
    if (active) {
        double v[N];
        if (from_origin) {                                 // (log_s, v, y) = (0, v0, 0)                   :1206-1208
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = c.v0[k];
        } else {                                           // continue from the resident state (single-expiry launches)
            ls = log_s[p];
            y = yq[p];
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = vol[static_cast<size_t>(k) * n + p];
        }
        if (RNG) {
            const PhiloxLane lane = philox_prepare(seed, c3, path_offset + p);
            rng_time_loop(lane, step_offset, nb_steps, tab, [&](double z0, double z1) { rough_step<N>(c, v, ls, y, z0, z1, exp_of); });
        } else {
            const double *const w[2] = {Z0 + p, Z1 + p};
            streamed_time_loop<2, SVMC_ROUGH_STREAM_U>(w, ldw, nb_steps,
                                                       [&](const double(&z)[2]) { rough_step<N>(c, v, ls, y, z[0], z[1], exp_of); });
        }
        if (i == e.m - 1) {
#pragma unroll
            for (int k = 0; k < N; ++k) vol[static_cast<size_t>(k) * n + p] = v[k];
            log_s[p] = ls;
            yq[p] = y;
        }
    }
    const SliceOut so = {x_snap + static_cast<size_t>(i) * n, q_snap ? q_snap + static_cast<size_t>(i) * n : nullptr,
                         partials + 2 * static_cast<size_t>(i) * ((n + 63) >> 6), e.forward[i], (n + 63) >> 6};
    slice_epilogue(so, p, active, ls, y);
}

}  // namespace svmc

using namespace svmc;

extern "C" {

// launch of rough_logsv_expiries_kernel: n_expiries simulations from time 0 side by side (grid.y).  EVERY from-origin launch of
// the rough model goes through this kernel -- the chain (svmc_rough_logsv_chain) and a single expiry (svmc_rough_logsv_slice /
// _terminal with from_origin != 0: grid.y = 1) -- so that one launch per expiry and all expiries in one launch are the same
// code on the same constants: identical bits by construction, not by how two kernels happen to be contracted.
static void launch_rough_expiries(const RoughConsts &c_in, int n_factors, int n_expiries, const int *nb_steps_host,
                                  const double *hs_host, const double *forwards_host, double *log_s, double *vol, double *qvar,
                                  size_t n_path, const double *Z0, const double *Z1, size_t ldw, uint64_t seed, uint32_t call_id,
                                  uint64_t path_offset, uint32_t step_offset, int from_origin, double *x_snapshots,
                                  double *qvar_snapshots, double *partials, hipStream_t st)
{
    RoughConsts c = c_in;
    RoughExpiries e{};
    e.m = n_expiries;
    for (int i = 0; i < MAX_CHAIN_SLICES; ++i) {
        const int j = i < n_expiries ? i : 0;
        const double h = hs_host[j];
        e.h[i] = h;
        e.inv_h[i] = 1.0 / h;
        e.sqrt_h[i] = sqrt(h);
        e.ito[i] = -0.5 * c.volvol_w * c.volvol_w * h;
        e.volvol_w_sqrt_h[i] = c.volvol_w * e.sqrt_h[i];
        e.forward[i] = forwards_host ? forwards_host[j] : 0.0;
        e.nb_steps[i] = nb_steps_host[j];
    }
    const bool draw = Z0 == nullptr;                        // the drawing kernels run the generators' block size
    const dim3 g(draw ? rng_grid(n_path) : grid_for(n_path), static_cast<unsigned>(n_expiries)), b(draw ? rng_block() : BLOCK);
    const uint32_t c3 = make_c3(call_id) | 3u;              // stream tag 3: the rough model's normals
#define SVMC_ROUGH_CHAIN_LAUNCH(NF)                                                                                          \
    do {                                                                                                                     \
        if (!draw)                                                                                                           \
            hipLaunchKernelGGL((rough_logsv_expiries_kernel<NF, false>), g, b, 0, st, log_s, vol, qvar, n_path, c, e, Z0, Z1, \
                               ldw, seed, c3, path_offset, step_offset, from_origin, x_snapshots, qvar_snapshots, partials); \
        else                                                                                                                 \
            hipLaunchKernelGGL((rough_logsv_expiries_kernel<NF, true>), g, b, 0, st, log_s, vol, qvar, n_path, c, e, Z0, Z1,  \
                               ldw, seed, c3, path_offset, step_offset, from_origin, x_snapshots, qvar_snapshots, partials); \
    } while (0)
    if (n_factors == 1) SVMC_ROUGH_CHAIN_LAUNCH(1);
    else if (n_factors == 2) SVMC_ROUGH_CHAIN_LAUNCH(2);
    else SVMC_ROUGH_CHAIN_LAUNCH(3);
#undef SVMC_ROUGH_CHAIN_LAUNCH
}

// the step-independent constants of the rough model
static RoughConsts make_rough_consts(int n_factors, const double *nodes_host, const double *weights_host, const double *v0_host,
                                     double theta, double kappa1, double kappa2, double rho, double volvol)
{
    RoughConsts c{};
    c.wsum = 0.0;
    c.w_lam_v0 = 0.0;
    for (int i = 0; i < n_factors; ++i) {
        c.nodes[i] = nodes_host[i];
        c.w[i] = weights_host[i];
        c.v0[i] = v0_host[i];
        c.wlam[i] = weights_host[i] * nodes_host[i];
        c.wsum += weights_host[i];
        c.w_lam_v0 += c.wlam[i] * v0_host[i];
    }
    c.theta = theta; c.kappa1 = kappa1; c.kappa2 = kappa2; c.rho = rho; c.rho_comp = sqrt(1.0 - rho * rho);
    c.volvol = volvol; c.inv_volvol = 1.0 / volvol; c.w_inv = 1.0 / c.wsum;
    c.volvol_w = volvol * c.wsum;
    return c;
}

static int rough_logsv_launch(const char *name, double *log_s, double *vol, double *qvar, size_t n_path, int nb_steps,
                              double h, int n_factors, const double *nodes_host, const double *weights_host,
                              const double *v0_host, double theta, double kappa1, double kappa2, double rho,
                              double volvol, const double *Z0, const double *Z1, size_t ldw, uint64_t seed,
                              uint32_t call_id, uint64_t path_offset, uint32_t step_offset, int from_origin,
                              const SliceOut &so, svmc_stream_t stream)
{
    const std::string fn(name);
    if (int rc = check_state(name, log_s, vol, qvar, nb_steps, h)) return rc;
    SVMC_REQUIRE(n_factors >= 1 && n_factors <= 3, fn + ": 1 <= n_factors <= 3");
    SVMC_REQUIRE(nodes_host && weights_host && v0_host, fn + ": null nodes/weights/v0");
    SVMC_REQUIRE((Z0 == nullptr) == (Z1 == nullptr), fn + ": Z0 and Z1 go together");
    SVMC_REQUIRE(Z0 == nullptr || ldw >= n_path, fn + ": ldw < n_path");
    SVMC_REQUIRE(call_id < (1u << 24), fn + ": call_id must fit 24 bits");
    SVMC_REQUIRE(volvol > 0.0 && rho * rho <= 1.0, fn + ": volvol > 0 and |rho| <= 1");
    if (n_path == 0 || (nb_steps == 0 && !from_origin && so.partials == nullptr)) return SVMC_OK;
    const RoughConsts c = make_rough_consts(n_factors, nodes_host, weights_host, v0_host, theta, kappa1, kappa2, rho, volvol);
    launch_rough_expiries(c, n_factors, 1, &nb_steps, &h, &so.forward, log_s, vol, qvar, n_path, Z0, Z1, ldw, seed, call_id,
                          path_offset, step_offset, from_origin, so.x_snap, so.q_snap, so.partials, as_stream(stream));
    return check_launch(name);
}

int svmc_rough_logsv_terminal(double *log_s, double *vol, double *qvar, size_t n_path, int nb_steps, double h,
                              int n_factors, const double *nodes_host, const double *weights_host,
                              const double *v0_host, double theta, double kappa1, double kappa2, double rho,
                              double volvol, const double *Z0, const double *Z1, size_t ldw, uint64_t seed,
                              uint32_t call_id, uint64_t path_offset, uint32_t step_offset, int from_origin,
                              svmc_stream_t stream)
{
    const SliceOut none = {nullptr, nullptr, nullptr, 0.0};
    return rough_logsv_launch("svmc_rough_logsv_terminal", log_s, vol, qvar, n_path, nb_steps, h, n_factors, nodes_host,
                              weights_host, v0_host, theta, kappa1, kappa2, rho, volvol, Z0, Z1, ldw, seed, call_id,
                              path_offset, step_offset, from_origin, none, stream);
}

int svmc_rough_logsv_slice(double *log_s, double *vol, double *qvar, size_t n_path, int nb_steps, double h,
                           int n_factors, const double *nodes_host, const double *weights_host, const double *v0_host,
                           double theta, double kappa1, double kappa2, double rho, double volvol, const double *Z0,
                           const double *Z1, size_t ldw, uint64_t seed, uint32_t call_id, uint64_t path_offset,
                           uint32_t step_offset, int from_origin, double forward, double *x_snapshot,
                           double *qvar_snapshot, double *spot_sums, void *workspace, size_t workspace_bytes,
                           svmc_stream_t stream)
{
    const char *fn = "svmc_rough_logsv_slice";
    if (int rc = check_slice_args(fn, n_path, x_snapshot, spot_sums, workspace, workspace_bytes)) return rc;
    SVMC_REQUIRE(n_path > 0 && nb_steps > 0, "svmc_rough_logsv_slice: n_path and nb_steps must be positive");
    const SliceOut so = {x_snapshot, qvar_snapshot, static_cast<double *>(workspace), forward, wave_rows(n_path)};
    if (int rc = rough_logsv_launch(fn, log_s, vol, qvar, n_path, nb_steps, h, n_factors, nodes_host, weights_host,
                                    v0_host, theta, kappa1, kappa2, rho, volvol, Z0, Z1, ldw, seed, call_id,
                                    path_offset, step_offset, from_origin, so, stream))
        return rc;
    return reduce_spot_partials(workspace, n_path, 2, spot_sums, as_stream(stream));
}

int svmc_rough_logsv_chain(double *log_s, double *vol, double *qvar, size_t n_path, int n_expiries, const int *nb_steps_host,
                           const double *hs_host, const double *forwards_host, int n_factors, const double *nodes_host,
                           const double *weights_host, const double *v0_host, double theta, double kappa1, double kappa2,
                           double rho, double volvol, const double *Z0, const double *Z1, size_t ldw, uint64_t seed,
                           uint32_t call_id, uint64_t path_offset, double *x_snapshots, double *qvar_snapshots,
                           double *spot_sums, void *workspace, size_t workspace_bytes, svmc_stream_t stream)
{
    const std::string fn("svmc_rough_logsv_chain");
    SVMC_REQUIRE(log_s && vol && qvar && x_snapshots && spot_sums && workspace, fn + ": null state / snapshot / spot_sums / workspace");
    SVMC_REQUIRE(nb_steps_host && hs_host && forwards_host, fn + ": null step counts / steps / forwards");
    SVMC_REQUIRE(n_expiries >= 1 && n_expiries <= MAX_CHAIN_SLICES, fn + ": 1 <= n_expiries <= 16");
    SVMC_REQUIRE(n_factors >= 1 && n_factors <= 3, fn + ": 1 <= n_factors <= 3");
    SVMC_REQUIRE(nodes_host && weights_host && v0_host, fn + ": null nodes/weights/v0");
    SVMC_REQUIRE((Z0 == nullptr) == (Z1 == nullptr), fn + ": Z0 and Z1 go together");
    SVMC_REQUIRE(Z0 == nullptr || ldw >= n_path, fn + ": ldw < n_path");
    SVMC_REQUIRE(call_id < (1u << 24), fn + ": call_id must fit 24 bits");
    SVMC_REQUIRE(volvol > 0.0 && rho * rho <= 1.0, fn + ": volvol > 0 and |rho| <= 1");
    SVMC_REQUIRE(n_path > 0, fn + ": n_path must be positive");
    if (workspace_bytes < static_cast<size_t>(wave_rows(n_path)) * 2 * n_expiries * sizeof(double))
        return fail(SVMC_ERR_WORKSPACE, fn + ": workspace too small (svmc_slice_workspace_bytes)");
    for (int i = 0; i < n_expiries; ++i)
        SVMC_REQUIRE(hs_host[i] > 0.0 && nb_steps_host[i] > 0, fn + ": steps and step counts must be positive");
    const RoughConsts c = make_rough_consts(n_factors, nodes_host, weights_host, v0_host, theta, kappa1, kappa2, rho, volvol);
    const hipStream_t st = as_stream(stream);
    launch_rough_expiries(c, n_factors, n_expiries, nb_steps_host, hs_host, forwards_host, log_s, vol, qvar, n_path, Z0, Z1, ldw,
                          seed, call_id, path_offset, 0u, 1, x_snapshots, qvar_snapshots, static_cast<double *>(workspace), st);
    reduce_columns(2 * n_expiries, st, static_cast<const double *>(workspace), wave_rows(n_path), size_t(1),
                   static_cast<size_t>(wave_rows(n_path)), spot_sums);
    return check_launch("svmc_rough_logsv_chain");
}

}  // extern "C"
