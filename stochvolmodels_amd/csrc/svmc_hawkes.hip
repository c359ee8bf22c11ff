// svmc_hawkes.hip -- the Hawkes jump-diffusion on gfx950 (pricers/hawkes_jd_pricer.py of the reference; F. Liu, N. Packham,
// A. Sepp 2025): the Monte Carlo generator and the coefficient-ODE transform grid.
//
//   hawkesjd_chain_rng_kernel  one lane per path, the state (x, lambda_p, lambda_m) in fp64 registers, ALL expiries of a chain in
//                              one launch: the step of simulate_hawkesjd_terminal (:715-779) in its order, the slice epilogue of
//                              svmc_slice.h per expiry (snapshot + per-wave spot partials for the chain payoff tail)
//   hawkesjd_rng_kernel        the same body for one slice on caller-owned state (simulate_hawkesjd_terminal)
//   hawkesjd_chain_rng_many_kernel  the same body for J independent jobs of one chain (blockIdx.y = job): each job's model, start
//                              intensities, step constants and Philox key from a device table, its expiries to snapshot rows
//                              j m + i; job j's bits are those of hawkesjd_chain_rng_kernel on its parameters and stream
//   hawkes_chain_cond_kernel   conditional Monte Carlo: the same step without the diffusion's normal on the state
//                              (mu, lambda_p, lambda_m), streams 9 and 10, no table and no LDS; per expiry a mu row and a cv row
//   hawkes_mgf_grid_batch_kernel  one lane per transform-grid point of up to 16 parameter sets per launch (blockIdx.y = set;
//                              one set, or the base point and bumped vectors of a calibration's finite-difference gradient):
//                              the three complex Riccati ODEs of solve_ode_for_a (:582-640) with the DOP853 pair of
//                              svmc_dop853.h and per-point step control; log E = a0 + a1 lp + a2 lm
//   hawkes_risk_forwards_kernel  the risk-premia kernel's normalizers and gamma forwards (:487-515): one lane pair per expiry,
//                              one wave per set, each lane the same ODEs from zero over the whole ttm at a real phi
//   mgf_gamma_slice_kernel     one block per (strike, set): the slice inversion under the risk-premia kernel
//                              (utils/mgf_pricer.py:273-321), the price finished on the device from the forwards kernel's output
//
// Randoms (svmc_rng.h, streams 6 and 7): step s of path p is ONE Philox call of stream 6 at counter index s (the chain-global
// step): word 0 -> the N(0,1) of the diffusion (normal_icdf32), words 1 and 2 -> u_p, u_m = (r + 1/2) 2^-32, word 3 unused.
// A side jumps iff lambda dt > -ln u (the reference's lambda > -log(u)/dt); -ln u >= 1 - u screens the test, so the fp64
// logarithm runs only where 1 - u < lambda dt.  Only on a step where a side jumped is stream 7's call at the same index drawn:
// E_p = -ln((r0 + 1/2) 2^-32), E_m = -ln((r1 + 1/2) 2^-32), J_P = shift_p + mean_p E_p, J_M = shift_m - (-mean_m) E_m.
// The intensities follow the reference's Euler step with no floor: they may go negative exactly as there.
#include "svmc_internal.h"

#include <cmath>
#include <string>

#include "svmc_rng.h"
#include "svmc_slice.h"
#include "svmc_complex.h"
#include "svmc_ode.h"
#include "svmc_dop853.h"
#include "svmc_mgf_slice.h"

namespace svmc {

namespace {

constexpr int HAWKES_BLOCK = 512;          // a block stages the draw's table in LDS once for its eight waves
constexpr int HAWKES_MAX_SLICES = MAX_FUSED_SLICES;
constexpr uint32_t HAWKES_STREAM = 6u, HAWKES_JUMP_STREAM = 7u;

// the per-path constants of the model (params order of include/svmc.h SVMC_HAWKESJD_PARAMS)
struct HawkesModel {
    double shift_p, mean_p, shift_m, neg_mean_m;
    double theta_p, beta1_p, beta2_p, theta_m, beta1_m, beta2_m;
};

// the constants of one slice's step (:753-764)
struct HawkesStep {
    double dt, drift_dt, comp_p_dt, comp_m_dt, sigma_sqrt_dt, kappa_p_dt, kappa_m_dt;
};

struct HawkesChainSlices {
    HawkesStep c[HAWKES_MAX_SLICES];
    double forward[HAWKES_MAX_SLICES];
    int nb_steps[HAWKES_MAX_SLICES];
    int m;
};

enum { P_MU, P_SIGMA, P_SHIFT_P, P_MEAN_P, P_SHIFT_M, P_MEAN_M, P_LAMBDA_P, P_THETA_P, P_KAPPA_P, P_BETA1_P, P_BETA2_P,
       P_LAMBDA_M, P_THETA_M, P_KAPPA_M, P_BETA1_M, P_BETA2_M };
static_assert(P_BETA2_M + 1 == SVMC_HAWKESJD_PARAMS, "include/svmc.h and the parameter block must agree");

HawkesModel make_hawkes_model(const double *p)
{
    return HawkesModel{p[P_SHIFT_P], p[P_MEAN_P], p[P_SHIFT_M], -p[P_MEAN_M], p[P_THETA_P], p[P_BETA1_P], p[P_BETA2_P],
                       p[P_THETA_M], p[P_BETA1_M], p[P_BETA2_M]};
}

HawkesStep make_hawkes_step(double dt, const double *p)
{
    HawkesStep c;
    c.dt = dt;
    c.drift_dt = (p[P_MU] - 0.5 * p[P_SIGMA] * p[P_SIGMA]) * dt;                                     // :764
    c.comp_p_dt = dt * (std::exp(p[P_SHIFT_P]) / (1.0 - p[P_MEAN_P]) - 1.0);                       // :761
    c.comp_m_dt = dt * (std::exp(p[P_SHIFT_M]) / (1.0 - p[P_MEAN_M]) - 1.0);                       // :762
    c.sigma_sqrt_dt = p[P_SIGMA] * std::sqrt(dt);
    c.kappa_p_dt = p[P_KAPPA_P] * dt;
    c.kappa_m_dt = p[P_KAPPA_M] * dt;
    return c;
}

// one time step (:765-774) at the chain-global step index s (wave-uniform)
__device__ __forceinline__ void hawkes_step(const HawkesModel &md, const HawkesStep &c, const PhiloxLane &lane,
                                            const PhiloxLane &lane_j, uint32_t s, const RngTables &tab, double &x, double &lp,
                                            double &lm)
{
    uint32_t r[4];
    philox_draw(lane, s, r);
    const double z = normal_icdf32<SVMC_ICDF_M, SVMC_ICDF_SEGMENTS, SVMC_ICDF_DEG, SVMC_ICDF_EDGE != 0, SVMC_ICDF_RAW != 0>(r[0], tab.icdf);
    const double up = uniform_32(r[1]), um = uniform_32(r[2]);
    const double hp = lp * c.dt, hm = lm * c.dt;
    bool jp = (1.0 - up) < hp, jm = (1.0 - um) < hm;          // -ln u >= 1 - u: no jump without this (1 - u is exact)
    if (jp) jp = neg_log(up) < hp;                             // :768, fp64
    if (jm) jm = neg_log(um) < hm;                             // :769
    double jump_p = 0.0, jump_m = 0.0;
    if (jp || jm) {                                            // rare and divergent: the jump sizes of this step, stream 7
        uint32_t e[4];
        philox_draw(lane_j, s, e);
        if (jp) jump_p = md.shift_p + md.mean_p * neg_log(uniform_32(e[0]));          // :757
        if (jm) jump_m = md.shift_m - md.neg_mean_m * neg_log(uniform_32(e[1]));      // :758
    }
    // :766 with the intensities at the start of the step, then :770-774
    const double diffusion = ((c.drift_dt - c.comp_p_dt * lp) - c.comp_m_dt * lm) + c.sigma_sqrt_dt * z;
    x = ((x + diffusion) + jump_p) + jump_m;
    const double load_p = md.beta1_p * jump_p + md.beta2_p * jump_m;
    const double load_m = md.beta1_m * jump_p + md.beta2_m * jump_m;
    lp = (lp + c.kappa_p_dt * (md.theta_p - lp)) + load_p;
    lm = (lm + c.kappa_m_dt * (md.theta_m - lm)) + load_m;
}

// ---- many independent jobs of one chain in ONE stepping launch (svmc_hawkesjd_chain_price_many): blockIdx.y = job,
// blockIdx.x = block of that job's n paths.  The per-job device table, one upload per call: [J] HawkesJob, then the
// (job, expiry) step constants [J][m].
struct HawkesJob {
    HawkesModel md;
    double lambda_p, lambda_m;             // both start intensities
    uint64_t seed;
    uint32_t c3, pad;                      // the call id's counter word
};
struct HawkesManySlices {
    double forward[HAWKES_MAX_SLICES];
    int nb_steps[HAWKES_MAX_SLICES];
    int m;
};

// Where hawkes_body's job comes from (as ChainArgs / ManyTable of svmc_jobs.h).  The body is written once over a job source
// and runs the same statements -- hence gives the same bits -- whichever one hands it the job:
//   HawkesArgs   the one-job kernels: everything is a kernel argument; the path starts from `init` or the state arrays at step
//                `step_offset` of its streams, expiry i goes to row i, and the terminal state is written back
//   HawkesTable  the many-job kernel: job blockIdx.y of the device table; the path starts from (0, lambda_p_j, lambda_m_j) at
//                step 0, expiry i goes to row j m + i, nothing is written back.  The job's constants are job-uniform and the
//                table is read-only for the launch (__restrict__ const): the compiler issues these plain loads as scalar loads
struct HawkesArgs {
    const HawkesChainSlices &cs;
    const HawkesModel &md;
    uint64_t seed_;
    uint32_t c3_, step_offset;
    const StateInit &init;
    double *__restrict__ x, *__restrict__ lam_p, *__restrict__ lam_m;

    __device__ __forceinline__ int m() const { return cs.m; }
    __device__ __forceinline__ int nb_steps(int i) const { return cs.nb_steps[i]; }
    __device__ __forceinline__ double forward(int i) const { return cs.forward[i]; }
    __device__ __forceinline__ HawkesStep step(int i) const { return cs.c[i]; }
    __device__ __forceinline__ HawkesModel model() const { return md; }
    __device__ __forceinline__ uint64_t seed() const { return seed_; }
    __device__ __forceinline__ uint32_t c3() const { return c3_; }
    __device__ __forceinline__ uint32_t step_origin() const { return step_offset; }
    __device__ __forceinline__ size_t row(int i) const { return static_cast<size_t>(i); }
    __device__ __forceinline__ void start(size_t p, double &xv, double &lp, double &lm) const
    {
        if (init.uniform) {                                    // wave-uniform
            xv = init.x0;
            lp = init.vol0;
            lm = init.qvar0;
        } else {
            xv = x[p];
            lp = lam_p[p];
            lm = lam_m[p];
        }
    }
    __device__ __forceinline__ void finish(size_t p, double xv, double lp, double lm) const
    {
        x[p] = xv;
        lam_p[p] = lp;
        lam_m[p] = lm;
    }
};

struct HawkesTable {
    const HawkesManySlices &cs;
    const HawkesJob *__restrict__ jobs;
    const HawkesStep *__restrict__ steps;

    __device__ __forceinline__ int job() const { return blockIdx.y; }
    __device__ __forceinline__ int m() const { return cs.m; }
    __device__ __forceinline__ int nb_steps(int i) const { return cs.nb_steps[i]; }
    __device__ __forceinline__ double forward(int i) const { return cs.forward[i]; }
    __device__ __forceinline__ HawkesStep step(int i) const { return steps[static_cast<size_t>(job()) * cs.m + i]; }
    __device__ __forceinline__ HawkesModel model() const { return jobs[job()].md; }
    __device__ __forceinline__ uint64_t seed() const { return jobs[job()].seed; }
    __device__ __forceinline__ uint32_t c3() const { return jobs[job()].c3; }
    __device__ __forceinline__ uint32_t step_origin() const { return 0u; }
    __device__ __forceinline__ size_t row(int i) const { return static_cast<size_t>(job()) * cs.m + i; }
    __device__ __forceinline__ void start(size_t, double &xv, double &lp, double &lm) const
    {
        xv = 0.0;
        lp = jobs[job()].lambda_p;
        lm = jobs[job()].lambda_m;
    }
    __device__ __forceinline__ void finish(size_t, double, double, double) const {}
};

// x_snap / partials null: a single slice on caller-owned state (no epilogue)
template <class Source>
__device__ __forceinline__ void hawkes_body(size_t n, const Source &src, uint64_t path_offset, double *__restrict__ x_snap,
                                            double *__restrict__ partials)
{
    __shared__ RngTablesLds s_tab;
    const RngTables tab = stage_rng_tables(s_tab);
    const size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool active = p < n;
    const HawkesModel md = src.model();
    double xv = 0.0, lp = 0.0, lm = 0.0;
    if (active) src.start(p, xv, lp, lm);
    const PhiloxLane lane = philox_prepare(src.seed(), src.c3() | HAWKES_STREAM, path_offset + p);
    const PhiloxLane lane_j = philox_prepare(src.seed(), src.c3() | HAWKES_JUMP_STREAM, path_offset + p);
    uint32_t step = src.step_origin();
    const int m = src.m();
    for (int i = 0; i < m; ++i) {
        const uint32_t end = step + static_cast<uint32_t>(src.nb_steps(i));
        if (active) {
            const HawkesStep c = src.step(i);
            for (uint32_t s = step; s < end; ++s) hawkes_step(md, c, lane, lane_j, s, tab, xv, lp, lm);
        }
        step = end;
        if (x_snap != nullptr) {
            const size_t rows = (n + 63) >> 6, row = src.row(i);
            const SliceOut so = {x_snap + row * n, nullptr, partials + 2 * row * rows, src.forward(i), rows};
            slice_epilogue(so, p, active, xv, 0.0);
        }
    }
    if (active) src.finish(p, xv, lp, lm);
}

__global__ __launch_bounds__(HAWKES_BLOCK) void hawkesjd_chain_rng_kernel(double *__restrict__ x, double *__restrict__ lam_p,
                                                                         double *__restrict__ lam_m, size_t n, HawkesChainSlices cs,
                                                                         HawkesModel md, uint64_t seed, uint32_t c3,
                                                                         uint64_t path_offset, uint32_t step_offset,
                                                                         double *__restrict__ x_snap, double *__restrict__ partials,
                                                                         StateInit init)
{
    hawkes_body(n, HawkesArgs{cs, md, seed, c3, step_offset, init, x, lam_p, lam_m}, path_offset, x_snap, partials);
}

__global__ __launch_bounds__(HAWKES_BLOCK) void hawkesjd_rng_kernel(double *__restrict__ x, double *__restrict__ lam_p,
                                                                   double *__restrict__ lam_m, size_t n, HawkesChainSlices cs,
                                                                   HawkesModel md, uint64_t seed, uint32_t c3, uint64_t path_offset,
                                                                   uint32_t step_offset)
{
    const StateInit init;
    hawkes_body(n, HawkesArgs{cs, md, seed, c3, step_offset, init, x, lam_p, lam_m}, path_offset, nullptr, nullptr);
}

__global__ __launch_bounds__(HAWKES_BLOCK) void hawkesjd_chain_rng_many_kernel(size_t n, HawkesManySlices cs,
                                                                              const HawkesJob *__restrict__ jobs,
                                                                              const HawkesStep *__restrict__ steps,
                                                                              uint64_t path_offset, double *__restrict__ x_snap,
                                                                              double *__restrict__ partials)
{
    hawkes_body(n, HawkesTable{cs, jobs, steps}, path_offset, x_snap, partials);
}

// ---- conditional Monte Carlo (include/svmc.h).  The diffusion sigma w0 is independent of both jump processes
// and both intensities, so given a path's jumps its discretised log-return is N(mu, cv) with ONE cv for every path: the lane
// carries (mu, lambda_p, lambda_m), draws no normal, stages no table and uses no LDS; cv_i is a kernel argument per slice, formed
// on the host.  Streams 9 and 10 (svmc_rng.h): the jump uniforms of TWO steps per call of stream 9, the jump sizes as stream 7's.
#ifndef SVMC_HAWKES_COND_BLOCK
#define SVMC_HAWKES_COND_BLOCK 256         // nothing is staged per block; an A/B build at 512: profiles/hawkes_cmc_bench.json
#endif
constexpr int HAWKES_COND_BLOCK = SVMC_HAWKES_COND_BLOCK;
constexpr uint32_t HAWKES_COND_STREAM = 9u, HAWKES_COND_JUMP_STREAM = 10u;

struct HawkesCondSlices {
    HawkesStep c[HAWKES_MAX_SLICES];       // sigma_sqrt_dt is not read
    double cv[HAWKES_MAX_SLICES];          // the conditional variance at the end of slice i
    int nb_steps[HAWKES_MAX_SLICES];
    int m;
};

// one time step on the words (wp, wm) of stream 9: hawkes_step's statements without the diffusion's normal
__device__ __forceinline__ void hawkes_cond_step(const HawkesModel &md, const HawkesStep &c, const PhiloxLane &lane_j, uint32_t s,
                                                 uint32_t wp, uint32_t wm, double &mu, double &lp, double &lm)
{
    // no implicit contraction: the step is inlined as the first and the second step of a call and as a slice's head and tail, and
    // which products the compiler would fuse with a following add depends on the code around each copy -- a chain must give the
    // same bits however it is cut into slices and launches
#pragma clang fp contract(off)
    const double up = uniform_32(wp), um = uniform_32(wm);
    const double hp = lp * c.dt, hm = lm * c.dt;
    bool jp = (1.0 - up) < hp, jm = (1.0 - um) < hm;          // -ln u >= 1 - u: no jump without this (1 - u is exact)
    if (jp) jp = neg_log(up) < hp;
    if (jm) jm = neg_log(um) < hm;
    double jump_p = 0.0, jump_m = 0.0;
    if (jp || jm) {                                            // rare and divergent: the jump sizes of this step, stream 10
        uint32_t e[4];
        philox_draw(lane_j, s, e);
        if (jp) jump_p = md.shift_p + md.mean_p * neg_log(uniform_32(e[0]));
        if (jm) jump_m = md.shift_m - md.neg_mean_m * neg_log(uniform_32(e[1]));
    }
    const double drift = (c.drift_dt - c.comp_p_dt * lp) - c.comp_m_dt * lm;
    mu = ((mu + drift) + jump_p) + jump_m;
    const double load_p = md.beta1_p * jump_p + md.beta2_p * jump_m;
    const double load_m = md.beta1_m * jump_p + md.beta2_m * jump_m;
    lp = (lp + c.kappa_p_dt * (md.theta_p - lp)) + load_p;
    lm = (lm + c.kappa_m_dt * (md.theta_m - lm)) + load_m;
}

// All slices of a launch.  Chain-global step s reads words 2 (s & 1), 2 (s & 1) + 1 of stream 9's call s >> 1; every branch on s
// is wave-uniform.  A slice that begins on an odd step takes the second pair of the call its predecessor's tail drew -- carried
// in r when that slice ran in this launch, re-drawn when the launch itself begins on the odd step.
__global__ __launch_bounds__(HAWKES_COND_BLOCK) void hawkes_chain_cond_kernel(double *__restrict__ mu_state, double *__restrict__ lam_p,
                                                                             double *__restrict__ lam_m, size_t n, HawkesCondSlices cs,
                                                                             HawkesModel md, uint64_t seed, uint32_t c3,
                                                                             uint64_t path_offset, uint32_t step_offset,
                                                                             double *__restrict__ mu_snap, double *__restrict__ cv_snap,
                                                                             StateInit init)
{
    const size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= n) return;                                        // no barrier and no cross-lane traffic below
    double mu, lp, lm;
    if (init.uniform) {                                        // wave-uniform
        mu = init.x0;
        lp = init.vol0;
        lm = init.qvar0;
    } else {
        mu = mu_state[p];
        lp = lam_p[p];
        lm = lam_m[p];
    }
    const PhiloxLane lane = philox_prepare(seed, c3 | HAWKES_COND_STREAM, path_offset + p);
    const PhiloxLane lane_j = philox_prepare(seed, c3 | HAWKES_COND_JUMP_STREAM, path_offset + p);
    uint32_t r[4] = {0u, 0u, 0u, 0u};
    uint32_t s = step_offset;
    for (int i = 0; i < cs.m; ++i) {
        const uint32_t end = s + static_cast<uint32_t>(cs.nb_steps[i]);
        const HawkesStep c = cs.c[i];
        if (s < end && (s & 1u)) {                             // head: the second pair of call s >> 1
            if (s == step_offset) philox_draw(lane, s >> 1, r);
            hawkes_cond_step(md, c, lane_j, s, r[2], r[3], mu, lp, lm);
            ++s;
        }
        for (; s + 1u < end; s += 2u) {                        // the hot loop: one call, its two steps
            philox_draw(lane, s >> 1, r);
            hawkes_cond_step(md, c, lane_j, s, r[0], r[1], mu, lp, lm);
            hawkes_cond_step(md, c, lane_j, s + 1u, r[2], r[3], mu, lp, lm);
        }
        if (s < end) {                                         // tail: the first pair; the second waits in r for the next slice
            philox_draw(lane, s >> 1, r);
            hawkes_cond_step(md, c, lane_j, s, r[0], r[1], mu, lp, lm);
            ++s;
        }
        if (mu_snap != nullptr) mu_snap[static_cast<size_t>(i) * n + p] = mu;
        if (cv_snap != nullptr) cv_snap[static_cast<size_t>(i) * n + p] = cs.cv[i];
    }
    mu_state[p] = mu;
    lam_p[p] = lp;
    lam_m[p] = lm;
}

int check_params(const char *fn, const double *p)
{
    SVMC_REQUIRE(p != nullptr, std::string(fn) + ": null params");
    for (int i = 0; i < SVMC_HAWKESJD_PARAMS; ++i)
        SVMC_REQUIRE(std::isfinite(p[i]), std::string(fn) + ": non-finite parameter");
    SVMC_REQUIRE(p[P_SIGMA] >= 0.0, std::string(fn) + ": sigma must be non-negative");
    SVMC_REQUIRE(p[P_MEAN_P] >= 0.0 && p[P_MEAN_P] < 1.0, std::string(fn) + ": need 0 <= mean_p < 1");
    SVMC_REQUIRE(p[P_MEAN_M] <= 0.0, std::string(fn) + ": need mean_m <= 0");
    return SVMC_OK;
}

unsigned hawkes_grid(size_t n) { return static_cast<unsigned>((n + HAWKES_BLOCK - 1) / HAWKES_BLOCK); }

// ---- the transform grid ------------------------------------------------------------------------------------------------
struct HawkesOde {
    double sigma2, kappa_p, kappa_m, kth_p, kth_m, comp_p, comp_m;
    double shift_p, mean_p, shift_m, mean_m, beta1_p, beta2_p, beta1_m, beta2_m;
};

HawkesOde make_hawkes_ode(const double *p)
{
    HawkesOde o;
    o.sigma2 = p[P_SIGMA] * p[P_SIGMA];
    o.kappa_p = p[P_KAPPA_P];
    o.kappa_m = p[P_KAPPA_M];
    o.kth_p = p[P_KAPPA_P] * p[P_THETA_P];
    o.kth_m = p[P_KAPPA_M] * p[P_THETA_M];
    o.comp_p = std::exp(p[P_SHIFT_P]) / (1.0 - p[P_MEAN_P]) - 1.0;                                  // :69
    o.comp_m = std::exp(p[P_SHIFT_M]) / (1.0 - p[P_MEAN_M]) - 1.0;                                  // :70
    o.shift_p = p[P_SHIFT_P];
    o.mean_p = p[P_MEAN_P];
    o.shift_m = p[P_SHIFT_M];
    o.mean_m = p[P_MEAN_M];
    o.beta1_p = p[P_BETA1_P];
    o.beta2_p = p[P_BETA2_P];
    o.beta1_m = p[P_BETA1_M];
    o.beta2_m = p[P_BETA2_M];
    return o;
}

// func_rhs of solve_ode_for_a (:607-626); h0 = sigma^2 (phi (phi + 1) / 2 - psi) is the same for every evaluation
__device__ __forceinline__ void hawkes_rhs(const HawkesOde &o, cd phi, cd h0, const cd (&a)[3], cd (&out)[3])
{
    const cd zp = (phi - o.beta1_p * a[1]) - o.beta1_m * a[2];
    const cd zm = (phi - o.beta2_p * a[1]) - o.beta2_m * a[2];
    const cd j_p = cexp_(-(o.shift_p * zp)) / (1.0 + o.mean_p * zp) - 1.0;                  // e_p, :594-601
    const cd j_m = cexp_(-(o.shift_m * zm)) / (1.0 + o.mean_m * zm) - 1.0;                  // e_m, :603-605
    out[0] = (o.kth_p * a[1] + o.kth_m * a[2]) + h0;
    out[1] = (j_p - o.kappa_p * a[1]) + o.comp_p * phi;
    out[2] = (j_m - o.kappa_m * a[2]) + o.comp_m * phi;
}

// DOP853 on the three components, the controller of svmc_analytic.hip's dop853 (SciPy's), error normed over n = 3
__device__ void hawkes_dop853(const HawkesOde &o, cd phi, cd h0, double ttm, cd (&y)[3], double rtol, double atol)
{
    constexpr double STEP_FLOOR = 0x1.0p-46;
    constexpr int MAX_TRIES = 1 << 15;
    cd K1[3], K2[3] = {}, K3[3] = {}, K4[3] = {}, K5[3] = {}, K6[3] = {}, K7[3] = {}, K8[3] = {}, K9[3] = {}, K10[3] = {},
       K11[3] = {}, K12[3] = {}, yt[3], yn[3], kn[3];
    double t = 0.0, h = ttm / 8.0;
    int tries = 0;
    bool rejected = false;
    hawkes_rhs(o, phi, h0, y, K1);
#define SVMC_HK_STAGE(S, KS)                                                                                                 \
    _Pragma("unroll") for (int i = 0; i < 3; ++i)                                                                            \
    {                                                                                                                        \
        const cd k1 = K1[i], k2 = K2[i], k3 = K3[i], k4 = K4[i], k5 = K5[i], k6 = K6[i], k7 = K7[i], k8 = K8[i], k9 = K9[i],  \
                 k10 = K10[i], k11 = K11[i];                                                                                 \
        (void)k2; (void)k3; (void)k4; (void)k5; (void)k6; (void)k7; (void)k8; (void)k9; (void)k10; (void)k11;               \
        yt[i] = y[i] + h * (SVMC_D853_STAGE_##S);                                                                            \
    }                                                                                                                        \
    hawkes_rhs(o, phi, h0, yt, KS)
    while (t < ttm && tries < MAX_TRIES) {
        ++tries;
        if (!(h >= STEP_FLOOR * ttm)) break;
        if (t + h > ttm) h = ttm - t;
        SVMC_HK_STAGE(2, K2);
        SVMC_HK_STAGE(3, K3);
        SVMC_HK_STAGE(4, K4);
        SVMC_HK_STAGE(5, K5);
        SVMC_HK_STAGE(6, K6);
        SVMC_HK_STAGE(7, K7);
        SVMC_HK_STAGE(8, K8);
        SVMC_HK_STAGE(9, K9);
        SVMC_HK_STAGE(10, K10);
        SVMC_HK_STAGE(11, K11);
        SVMC_HK_STAGE(12, K12);
        double e5 = 0.0, e3 = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const cd k1 = K1[i], k6 = K6[i], k7 = K7[i], k8 = K8[i], k9 = K9[i], k10 = K10[i], k11 = K11[i], k12 = K12[i];
            yn[i] = y[i] + h * (SVMC_D853_B);
            const cd err5 = SVMC_D853_E5, err3 = SVMC_D853_E3;
            const double m2 = fmax(y[i].re * y[i].re + y[i].im * y[i].im, yn[i].re * yn[i].re + yn[i].im * yn[i].im);
            const double sc = atol + rtol * sqrt(m2);
            const double inv = 1.0 / (sc * sc);
            e5 += (err5.re * err5.re + err5.im * err5.im) * inv;
            e3 += (err3.re * err3.re + err3.im * err3.im) * inv;
        }
        const double denom = e5 + 0.01 * e3;
        const bool finite = denom < 0x1.0p+1000;               // false for inf and NaN: an overflowed trial step
        const double err_sq = !finite ? __builtin_huge_val() : ((denom > 0.0) ? (h * h) * (e5 * e5) / (denom * 3.0) : 0.0);
        const bool accept = err_sq < 1.0;
        double fac = !finite ? 0.2 : ((err_sq > 0.0) ? 0.9 * pow(err_sq, -0.0625) : 10.0);
        if (accept) {
            hawkes_rhs(o, phi, h0, yn, kn);
            t += h;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                y[i] = yn[i];
                K1[i] = kn[i];
            }
            fac = fmin(rejected ? 1.0 : 10.0, fac);
            rejected = false;
        } else {
            fac = fmax(0.2, fmin(fac, 1.0));
            rejected = true;
        }
        h *= fac;
    }
#undef SVMC_HK_STAGE
    if (!(t >= ttm)) {                                         // given up: NaN, dropped by the inversion's nansum
#pragma unroll
        for (int i = 0; i < 3; ++i) y[i] = cd{__builtin_nan(""), __builtin_nan("")};
    }
}

constexpr int HK_AB = 64;
constexpr int HK_MAX_SETS = 16;        // parameter sets per batched launch (kernel-argument block: 16 x 136 B)

// one transform-grid point: a_t0 in, a_t1 and log E = a0 + a1 lambda_p + a2 lambda_m (:545) out
__device__ __forceinline__ void hawkes_grid_point(const cd *__restrict__ phi, const cd *__restrict__ psi, size_t j, double ttm,
                                                  const HawkesOde &o, double lambda_p, double lambda_m, cd *__restrict__ a,
                                                  cd *__restrict__ log_mgf, double rtol, double atol)
{
    const cd ph = phi[j];
    const cd h0 = o.sigma2 * ((0.5 * ((ph + 1.0) * ph)) - psi[j]);                                 // :623
    cd y[3] = {a[3 * j], a[3 * j + 1], a[3 * j + 2]};                                              // a_t0, chained across expiries
    hawkes_dop853(o, ph, h0, ttm, y, rtol, atol);
    a[3 * j] = y[0];
    a[3 * j + 1] = y[1];
    a[3 * j + 2] = y[2];
    log_mgf[j] = (y[0] + lambda_p * y[1]) + lambda_m * y[2];                                       // :545
}

// The parameter sets of one launch.  blockIdx.y picks the set, so a block's one wave belongs to one set and its constants
// are read from the kernel arguments at a wave-uniform index (scalar loads).  Each set has its own transform grid (the grid
// scale follows its sigma), coefficients and output.  svmc_hawkesjd_mgf_grid is this kernel at one set: a separate
// single-set kernel built from the same lines was scheduled differently enough to differ in the last bit at 3 % of the
// points, and the batch must equal one call per set bit for bit.
struct HawkesOdeSet {
    HawkesOde o;
    double lambda_p, lambda_m;
};
struct HawkesOdeBatch {
    HawkesOdeSet s[HK_MAX_SETS];
};

__global__ __launch_bounds__(HK_AB) void hawkes_mgf_grid_batch_kernel(const cd *__restrict__ phi, const cd *__restrict__ psi,
                                                                     size_t n_grid, double ttm, HawkesOdeBatch sets,
                                                                     cd *__restrict__ a, cd *__restrict__ log_mgf, double rtol,
                                                                     double atol)
{
    const size_t j = static_cast<size_t>(blockIdx.x) * HK_AB + threadIdx.x;
    if (j >= n_grid) return;
    const HawkesOdeSet &set = sets.s[blockIdx.y];
    const size_t off = static_cast<size_t>(blockIdx.y) * n_grid;       // this set's rows
    hawkes_grid_point(phi + off, psi + off, j, ttm, set.o, set.lambda_p, set.lambda_m, a + 3 * off, log_mgf + off, rtol, atol);
}

// ---- the risk-premia (Esscher-type) kernel: hawkesjd_forwards_under_risk_kernel (:487-515) and
//      slice_pricer_with_mgf_grid_with_gamma (utils/mgf_pricer.py:273-321) ----------------------------------------------------
constexpr int HK_RISK_MAX_TTMS = HK_AB / 2;    // expiries per forwards launch: one lane pair each, one wave per set

struct HawkesRiskTtms {
    double ttm[HK_RISK_MAX_TTMS], forward[HK_RISK_MAX_TTMS];
    double gamma[HK_MAX_SETS];
    int m;                                     // expiries in this launch
};

// One wave per set (blockIdx.y), one lane pair per expiry: lane 2e + k integrates the coefficient ODEs from zero over the WHOLE
// [0, ttm_e] (no chaining across expiries, :497-507) at the real point phi = -gamma - k, psi = 0.  The even lane of the pair
// forms normalizer = 1 / exp(Re log E(-gamma)) and gamma_forward = forward exp(Re log E(-gamma - 1)) normalizer (:508-511).
// Latency-bound and tiny: the pair's two integrations diverge and are left to.  Outputs are [expiry][set] (ld = n_sets).
__global__ __launch_bounds__(HK_AB) void hawkes_risk_forwards_kernel(HawkesOdeBatch sets, HawkesRiskTtms tt, int n_sets,
                                                                     double *__restrict__ normalizers,
                                                                     double *__restrict__ gamma_forwards, double rtol,
                                                                     double atol)
{
    const int lane = threadIdx.x;
    const int e = lane >> 1, k = lane & 1;
    const HawkesOdeSet &set = sets.s[blockIdx.y];
    const double gamma = tt.gamma[blockIdx.y];
    double re = 0.0;
    if (e < tt.m) {
        const cd ph = C(-gamma - static_cast<double>(k));                     // phi_grid = [-gamma], phi_grid - 1.0
        const cd h0 = set.o.sigma2 * (0.5 * ((ph + 1.0) * ph));              // :623 with psi = 0
        cd y[3] = {C(0.0), C(0.0), C(0.0)};
        hawkes_dop853(set.o, ph, h0, tt.ttm[e], y, rtol, atol);
        re = ((y[0] + set.lambda_p * y[1]) + set.lambda_m * y[2]).re;        // :545
    }
    const double re1 = __shfl_xor(re, 1, 64);
    if (e < tt.m && k == 0) {
        const double normalizer = 1.0 / exp(re);
        const size_t at = static_cast<size_t>(e) * n_sets + blockIdx.y;
        normalizers[at] = normalizer;
        gamma_forwards[at] = (tt.forward[e] * exp(re1)) * normalizer;
    }
}

struct GammaSliceArgs {
    double x[MGF_SLICE_STRIKES];               // log(forward / strike)
    double strike[MGF_SLICE_STRIKES];
    int type[MGF_SLICE_STRIKES];               // 0 'C', 1 'P'
    double gamma[HK_MAX_SETS];
    int shortcut[HK_MAX_SETS];                 // 1: every |Re phi - (0.5 + gamma)| < 1e-10 (:296), decided on the host
    int k;
};

// One block per (strike, set), as mgf_vanilla_slice_kernel: the legacy Simpson dp, then the payoff weight of :296-302 -- the real
// shortcut (dp / pi) / (p^2 + 1/4) or the complex -(dp / pi) / ((phi + gamma + 1)(phi + gamma)) -- and
// nansum Re[w exp(-x phi + log E)] (NaN terms dropped, inf kept).  Thread 0 finishes the price from this expiry's normalizer and
// gamma forward (hawkes_risk_forwards_kernel's output, [expiry][set]): 'C' gamma_forward - normalizer K^(1 + gamma) cap,
// 'P' K - normalizer K^(1 + gamma) cap (:313-317).
__global__ __launch_bounds__(MGF_SLICE_BLOCK) void mgf_gamma_slice_kernel(const cd *__restrict__ phi, const cd *__restrict__ log_mgf,
                                                                          int n_grid, GammaSliceArgs sa,
                                                                          const double *__restrict__ normalizers,
                                                                          const double *__restrict__ gamma_forwards, size_t nf_at,
                                                                          double *__restrict__ prices, int prices_ld)
{
    __shared__ double lds[4];
    const int s = blockIdx.y;
    phi += static_cast<size_t>(s) * n_grid;
    log_mgf += static_cast<size_t>(s) * n_grid;
    const double x = sa.x[blockIdx.x];
    const double gamma = sa.gamma[s];
    const bool shortcut = sa.shortcut[s] != 0;
    const double h = phi[1].im - phi[0].im;
    const double cap = mgf_slice_nansum(n_grid, lds, [&](int j) {
        const cd ph = phi[j];
        const double dp_pi = legacy_weight(phi, j, n_grid, h, 1) / PI;
        cd pw;
        if (shortcut) {
            pw = C(dp_pi / (ph.im * ph.im + 0.25));
        } else {
            const cd pg = ph + gamma;
            pw = C(-dp_pi) / ((pg + 1.0) * pg);
        }
        const cd e = cexp_(log_mgf[j] - x * ph);
        return pw.re * e.re - pw.im * e.im;
    });
    if (threadIdx.x == 0) {
        const double strike = sa.strike[blockIdx.x];
        const double nk = normalizers[nf_at + s] * pow(strike, 1.0 + gamma);
        prices[static_cast<size_t>(s) * prices_ld + blockIdx.x] =
            (sa.type[blockIdx.x] == 0 ? gamma_forwards[nf_at + s] : strike) - nk * cap;
    }
}

}  // namespace

// the chain's stepping (svmc_chain.hip's svmc_hawkesjd_chain_price): every expiry in one launch per 16, the state starting at
// (0, lambda_p, lambda_m); the per-wave spot partials of each expiry left in `workspace` unreduced (spot_sums null, at most 16
// expiries) or reduced into spot_sums
int hawkes_step_partials(const double *params_host, double *x, double *lam_p, double *lam_m, size_t n_path, int n_slices,
                         const int *nb_steps_host, const double *dts_host, const double *forwards_host, uint64_t seed,
                         uint32_t call_id, uint64_t path_offset, double *x_snapshots, double *spot_sums, void *workspace,
                         size_t workspace_bytes, hipStream_t stream)
{
    const char *fn = "svmc_hawkesjd_chain_price";
    if (int rc = check_params(fn, params_host)) return rc;
    const HawkesModel md = make_hawkes_model(params_host);
    const StateInit init = {1, 0.0, params_host[P_LAMBDA_P], params_host[P_LAMBDA_M]};             // :672-674
    const auto fill = [&](HawkesChainSlices &cs, int i, int j) {
        cs.c[i] = make_hawkes_step(dts_host[j], params_host);
        cs.forward[i] = forwards_host[j];
    };
    const auto launch = [&](const HawkesChainSlices &cs, double *xs, double *, const StateInit &init_i, uint32_t step0) {
        hipLaunchKernelGGL(hawkesjd_chain_rng_kernel, dim3(hawkes_grid(n_path)), dim3(HAWKES_BLOCK), 0, stream, x, lam_p, lam_m, n_path,
                           cs, md, seed, call_id << 8, path_offset, step0, xs, static_cast<double *>(workspace), init_i);
    };
    return step_chain<HawkesChainSlices>(fn, init, x, lam_p, lam_m, n_path, n_slices, nb_steps_host, dts_host, forwards_host, call_id,
                                         0, x_snapshots, nullptr, spot_sums, workspace, workspace_bytes, stream, fill, launch);
}

// ---- conditional Monte Carlo: the stepping of svmc_hawkesjd_chain_cond (init not uniform: the state arrays) and of the fused
// drivers of svmc_chain.hip (hawkes_cond_step_from: from (0, lambda_p, lambda_m)).  Every check comes before the first launch;
// launches of at most 16 slices carry the step offset and the variance from one to the next.
static int hawkes_cond_step_chain(const char *fn, const StateInit &init, const double *params_host, double *mu, double *lam_p,
                                  double *lam_m, size_t n_path, int n_slices, const int *nb_steps_host, const double *dts_host,
                                  double cv_start, uint64_t seed, uint32_t call_id, uint64_t path_offset, uint32_t step_offset,
                                  double *mu_snapshots, double *cv_snapshots, double *cvs_host, hipStream_t stream)
{
#pragma clang fp contract(off)             // cv_i is rounded product by product and sum by sum, on any host
    if (int rc = check_params(fn, params_host)) return rc;
    SVMC_REQUIRE(mu && lam_p && lam_m, std::string(fn) + ": null state array");
    SVMC_REQUIRE(n_path > 0, std::string(fn) + ": n_path must be positive");
    SVMC_REQUIRE(n_slices >= 1 && nb_steps_host && dts_host, std::string(fn) + ": null grids / no slices");
    for (int i = 0; i < n_slices; ++i)
        SVMC_REQUIRE(nb_steps_host[i] >= 0 && dts_host[i] > 0.0 && std::isfinite(dts_host[i]),
                     std::string(fn) + ": need nb_steps >= 0 and dt > 0");
    SVMC_REQUIRE(call_id < (1u << 24), std::string(fn) + ": call_id must fit 24 bits");
    SVMC_REQUIRE(cv_start >= 0.0 && std::isfinite(cv_start), std::string(fn) + ": cv_start must be non-negative and finite");
    const HawkesModel md = make_hawkes_model(params_host);
    const double sigma2 = params_host[P_SIGMA] * params_host[P_SIGMA];
    double cv = cv_start;
    for (int i0 = 0; i0 < n_slices; i0 += HAWKES_MAX_SLICES) {
        HawkesCondSlices cs;
        cs.m = (n_slices - i0 < HAWKES_MAX_SLICES) ? (n_slices - i0) : HAWKES_MAX_SLICES;
        uint32_t steps = 0;
        for (int i = 0; i < HAWKES_MAX_SLICES; ++i) {
            const int j = (i < cs.m) ? i0 + i : i0;            // unused entries repeat a valid one
            cs.c[i] = make_hawkes_step(dts_host[j], params_host);
            cs.nb_steps[i] = (i < cs.m) ? nb_steps_host[j] : 0;
            if (i < cs.m) {
                const double per_step = sigma2 * dts_host[j];
                const double added = static_cast<double>(nb_steps_host[j]) * per_step;
                cv = cv + added;
                if (cvs_host != nullptr) cvs_host[j] = cv;
            }
            cs.cv[i] = cv;
            steps += static_cast<uint32_t>(cs.nb_steps[i]);
        }
        const size_t row = static_cast<size_t>(i0) * n_path;
        hipLaunchKernelGGL(hawkes_chain_cond_kernel, dim3(static_cast<unsigned>((n_path + HAWKES_COND_BLOCK - 1) / HAWKES_COND_BLOCK)),
                           dim3(HAWKES_COND_BLOCK), 0, stream, mu, lam_p, lam_m, n_path, cs, md, seed, call_id << 8, path_offset,
                           step_offset, mu_snapshots ? mu_snapshots + row : nullptr, cv_snapshots ? cv_snapshots + row : nullptr,
                           (i0 == 0) ? init : StateInit());
        if (int rc = check_launch(fn)) return rc;
        step_offset += steps;
    }
    return SVMC_OK;
}

int hawkes_cond_step_from(const char *fn, const double *params_host, double *mu, double *lam_p, double *lam_m, size_t n_path,
                          int n_slices, const int *nb_steps_host, const double *dts_host, uint64_t seed, uint32_t call_id,
                          uint64_t path_offset, double *mu_snapshots, double *cv_snapshots, hipStream_t stream)
{
    if (int rc = check_params(fn, params_host)) return rc;
    const StateInit init = {1, 0.0, params_host[P_LAMBDA_P], params_host[P_LAMBDA_M]};
    return hawkes_cond_step_chain(fn, init, params_host, mu, lam_p, lam_m, n_path, n_slices, nb_steps_host, dts_host, 0.0, seed,
                                  call_id, path_offset, 0u, mu_snapshots, cv_snapshots, nullptr, stream);
}

int hawkes_check_params(const char *fn, const double *params_host) { return check_params(fn, params_host); }

// ---- many jobs of one chain (svmc_chain.hip's svmc_hawkesjd_chain_price_many / _tilted_many)

size_t hawkes_many_table_bytes(int n_jobs, int n_slices)
{
    const size_t J = static_cast<size_t>(n_jobs);
    return J * sizeof(HawkesJob) + J * static_cast<size_t>(n_slices) * sizeof(HawkesStep);
}

// every job's parameter block, before anything is launched
int hawkes_check_many(const char *fn, int n_jobs, const double *params_host)
{
    for (int j = 0; j < n_jobs; ++j)
        if (int rc = check_params((std::string(fn) + " job " + std::to_string(j)).c_str(),
                                  params_host + static_cast<size_t>(SVMC_HAWKESJD_PARAMS) * j))
            return rc;
    return SVMC_OK;
}

int hawkes_chain_rng_many(size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
                          const double *forwards_host, const double *params_host, const uint64_t *seeds, const uint32_t *call_ids,
                          uint64_t path_offset, void *table_host, void *table_dev, double *x_snapshots, double *spot_partials,
                          hipStream_t stream)
{
    const char *fn = "hawkes_chain_rng_many";
    SVMC_REQUIRE(n_path > 0 && n_jobs >= 1 && n_jobs <= SVMC_MANY_MAX_JOBS && n_slices >= 1 && n_slices <= HAWKES_MAX_SLICES,
                 std::string(fn) + ": bad sizes");
    SVMC_REQUIRE(nb_steps_host && dts_host && forwards_host && params_host && seeds && call_ids && table_host && table_dev &&
                     x_snapshots && spot_partials,
                 std::string(fn) + ": null pointer");
    for (int i = 0; i < n_slices; ++i)
        SVMC_REQUIRE(nb_steps_host[i] > 0 && dts_host[i] > 0.0, std::string(fn) + ": nb_steps and dt must be positive");
    for (int j = 0; j < n_jobs; ++j) SVMC_REQUIRE(call_ids[j] < (1u << 24), std::string(fn) + ": call_id must fit 24 bits");
    if (int rc = hawkes_check_many(fn, n_jobs, params_host)) return rc;
    // the pinned table in the device table's byte layout: [J] jobs, then [J][m] step constants
    HawkesJob *jobs = static_cast<HawkesJob *>(table_host);
    HawkesStep *steps = reinterpret_cast<HawkesStep *>(jobs + n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        const double *p = params_host + static_cast<size_t>(SVMC_HAWKESJD_PARAMS) * j;
        jobs[j] = HawkesJob{make_hawkes_model(p), p[P_LAMBDA_P], p[P_LAMBDA_M], seeds[j], call_ids[j] << 8, 0u};      // :672-674
        for (int i = 0; i < n_slices; ++i) steps[static_cast<size_t>(j) * n_slices + i] = make_hawkes_step(dts_host[i], p);
    }
    SVMC_HIP_TRY(hipMemcpyAsync(table_dev, table_host, hawkes_many_table_bytes(n_jobs, n_slices), hipMemcpyHostToDevice, stream));
    HawkesManySlices cs;
    cs.m = n_slices;
    for (int i = 0; i < HAWKES_MAX_SLICES; ++i) {
        cs.forward[i] = forwards_host[i < n_slices ? i : 0];
        cs.nb_steps[i] = i < n_slices ? nb_steps_host[i] : 0;
    }
    const HawkesJob *jobs_dev = static_cast<const HawkesJob *>(table_dev);
    hipLaunchKernelGGL(hawkesjd_chain_rng_many_kernel, dim3(hawkes_grid(n_path), static_cast<unsigned>(n_jobs)), dim3(HAWKES_BLOCK), 0,
                       stream, n_path, cs, jobs_dev, reinterpret_cast<const HawkesStep *>(jobs_dev + n_jobs), path_offset, x_snapshots,
                       spot_partials);
    return check_launch(fn);
}

}  // namespace svmc

using namespace svmc;

extern "C" {

int svmc_hawkesjd_terminal_rng(double *x, double *lambda_p, double *lambda_m, size_t n_path, int nb_steps, double dt,
                               const double *params_host, uint64_t seed, uint32_t call_id, uint64_t path_offset,
                               uint32_t step_offset, svmc_stream_t stream)
{
    const char *fn = "svmc_hawkesjd_terminal_rng";
    if (int rc = check_params(fn, params_host)) return rc;
    SVMC_REQUIRE(x && lambda_p && lambda_m, std::string(fn) + ": null state array");
    SVMC_REQUIRE(n_path > 0, std::string(fn) + ": n_path must be positive");
    SVMC_REQUIRE(nb_steps >= 0 && dt > 0.0 && std::isfinite(dt), std::string(fn) + ": need nb_steps >= 0 and dt > 0");
    SVMC_REQUIRE(call_id < (1u << 24), std::string(fn) + ": call_id must fit 24 bits");
    if (nb_steps == 0) return SVMC_OK;
    HawkesChainSlices cs;
    cs.m = 1;
    for (int i = 0; i < HAWKES_MAX_SLICES; ++i) {
        cs.c[i] = make_hawkes_step(dt, params_host);
        cs.forward[i] = 1.0;
        cs.nb_steps[i] = (i == 0) ? nb_steps : 0;
    }
    hipLaunchKernelGGL(hawkesjd_rng_kernel, dim3(hawkes_grid(n_path)), dim3(HAWKES_BLOCK), 0, as_stream(stream), x, lambda_p, lambda_m,
                       n_path, cs, make_hawkes_model(params_host), seed, call_id << 8, path_offset, step_offset);
    return check_launch(fn);
}

int svmc_hawkesjd_chain_cond(double *mu, double *lambda_p, double *lambda_m, size_t n_path, int n_slices, const int *nb_steps_host,
                             const double *dts_host, const double *params_host, double cv_start, uint64_t seed, uint32_t call_id,
                             uint64_t path_offset, uint32_t step_offset, double *mu_snapshots, double *cv_snapshots, double *cvs_host,
                             svmc_stream_t stream)
{
    return hawkes_cond_step_chain("svmc_hawkesjd_chain_cond", StateInit(), params_host, mu, lambda_p, lambda_m, n_path, n_slices,
                                  nb_steps_host, dts_host, cv_start, seed, call_id, path_offset, step_offset, mu_snapshots,
                                  cv_snapshots, cvs_host, as_stream(stream));
}

int svmc_hawkesjd_mgf_grid(const double *phi, const double *psi, size_t n_grid, double ttm, const double *params_host, double *a,
                           double *log_mgf, double rtol, double atol, svmc_stream_t stream)
{
    const char *fn = "svmc_hawkesjd_mgf_grid";
    if (int rc = check_params(fn, params_host)) return rc;
    SVMC_REQUIRE(phi && psi && a && log_mgf, std::string(fn) + ": null pointer");
    SVMC_REQUIRE(ttm > 0.0 && rtol > 0.0 && atol > 0.0, std::string(fn) + ": ttm, rtol, atol must be positive");
    return svmc_hawkesjd_mgf_grid_batch(phi, psi, n_grid, 1, ttm, params_host, a, log_mgf, rtol, atol, stream);
}

int svmc_hawkesjd_mgf_grid_batch(const double *phi, const double *psi, size_t n_grid, int n_sets, double ttm,
                                 const double *params_host, double *a, double *log_mgf, double rtol, double atol,
                                 svmc_stream_t stream)
{
    const char *fn = "svmc_hawkesjd_mgf_grid_batch";
    SVMC_REQUIRE(phi && psi && a && log_mgf && params_host, std::string(fn) + ": null pointer");
    SVMC_REQUIRE(n_sets >= 1, std::string(fn) + ": n_sets < 1");
    SVMC_REQUIRE(ttm > 0.0 && rtol > 0.0 && atol > 0.0, std::string(fn) + ": ttm, rtol, atol must be positive");
    for (int s = 0; s < n_sets; ++s)                           // every set before anything is launched
        if (int rc = check_params((std::string(fn) + " set " + std::to_string(s)).c_str(),
                                  params_host + static_cast<size_t>(SVMC_HAWKESJD_PARAMS) * s))
            return rc;
    if (n_grid == 0) return SVMC_OK;
    for (int s0 = 0; s0 < n_sets; s0 += HK_MAX_SETS) {
        const int m = (n_sets - s0 < HK_MAX_SETS) ? (n_sets - s0) : HK_MAX_SETS;
        HawkesOdeBatch sets;
        for (int i = 0; i < HK_MAX_SETS; ++i) {                // unused slots repeat the first set: never read
            const double *p = params_host + static_cast<size_t>(SVMC_HAWKESJD_PARAMS) * (s0 + (i < m ? i : 0));
            sets.s[i] = HawkesOdeSet{make_hawkes_ode(p), p[P_LAMBDA_P], p[P_LAMBDA_M]};
        }
        const size_t off = static_cast<size_t>(s0) * n_grid;
        hipLaunchKernelGGL(hawkes_mgf_grid_batch_kernel, dim3(static_cast<unsigned>((n_grid + HK_AB - 1) / HK_AB), static_cast<unsigned>(m)),
                           dim3(HK_AB), 0, as_stream(stream), reinterpret_cast<const cd *>(phi) + off,
                           reinterpret_cast<const cd *>(psi) + off, n_grid, ttm, sets, reinterpret_cast<cd *>(a) + 3 * off,
                           reinterpret_cast<cd *>(log_mgf) + off, rtol, atol);
    }
    return check_launch(fn);
}

int svmc_hawkesjd_risk_forwards_batch(const double *params_host, const double *gammas_host, int n_sets, const double *ttms_host,
                                      const double *forwards_host, size_t n_ttms, double *normalizers, double *gamma_forwards,
                                      double rtol, double atol, svmc_stream_t stream)
{
    const char *fn = "svmc_hawkesjd_risk_forwards_batch";
    SVMC_REQUIRE(params_host && gammas_host && normalizers && gamma_forwards, std::string(fn) + ": null pointer");
    SVMC_REQUIRE(n_ttms == 0 || (ttms_host && forwards_host), std::string(fn) + ": null ttms or forwards");
    SVMC_REQUIRE(n_sets >= 1, std::string(fn) + ": n_sets < 1");
    SVMC_REQUIRE(rtol > 0.0 && atol > 0.0, std::string(fn) + ": rtol, atol must be positive");
    for (int s = 0; s < n_sets; ++s) {                         // every set and expiry before anything is launched
        if (int rc = check_params((std::string(fn) + " set " + std::to_string(s)).c_str(),
                                  params_host + static_cast<size_t>(SVMC_HAWKESJD_PARAMS) * s))
            return rc;
        SVMC_REQUIRE(std::isfinite(gammas_host[s]), std::string(fn) + ": non-finite gamma");
    }
    for (size_t e = 0; e < n_ttms; ++e) {
        SVMC_REQUIRE(ttms_host[e] > 0.0 && std::isfinite(ttms_host[e]), std::string(fn) + ": ttm must be positive and finite");
        SVMC_REQUIRE(std::isfinite(forwards_host[e]), std::string(fn) + ": non-finite forward");
    }
    for (int s0 = 0; s0 < n_sets; s0 += HK_MAX_SETS) {
        const int m = (n_sets - s0 < HK_MAX_SETS) ? (n_sets - s0) : HK_MAX_SETS;
        HawkesOdeBatch sets;
        HawkesRiskTtms tt;
        for (int i = 0; i < HK_MAX_SETS; ++i) {                // unused slots repeat the first set: never read
            const int si = s0 + (i < m ? i : 0);
            const double *p = params_host + static_cast<size_t>(SVMC_HAWKESJD_PARAMS) * si;
            sets.s[i] = HawkesOdeSet{make_hawkes_ode(p), p[P_LAMBDA_P], p[P_LAMBDA_M]};
            tt.gamma[i] = gammas_host[si];
        }
        for (size_t e0 = 0; e0 < n_ttms; e0 += HK_RISK_MAX_TTMS) {
            tt.m = static_cast<int>((n_ttms - e0 < HK_RISK_MAX_TTMS) ? (n_ttms - e0) : HK_RISK_MAX_TTMS);
            for (int e = 0; e < HK_RISK_MAX_TTMS; ++e) {
                tt.ttm[e] = (e < tt.m) ? ttms_host[e0 + e] : 1.0;
                tt.forward[e] = (e < tt.m) ? forwards_host[e0 + e] : 1.0;
            }
            const size_t at = e0 * static_cast<size_t>(n_sets) + static_cast<size_t>(s0);
            hipLaunchKernelGGL(hawkes_risk_forwards_kernel, dim3(1, static_cast<unsigned>(m)), dim3(HK_AB), 0, as_stream(stream),
                               sets, tt, n_sets, normalizers + at, gamma_forwards + at, rtol, atol);
        }
    }
    return check_launch(fn);
}

int svmc_mgf_gamma_slice_batch(const double *phi, const double *log_mgf, size_t n_grid, int n_sets, const double *gammas_host,
                               const int *shortcut_host, const double *normalizers, const double *gamma_forwards, int expiry,
                               double forward, const double *strikes_host, const int *type_codes_host, size_t n_strikes,
                               double *prices, svmc_stream_t stream)
{
    const char *fn = "svmc_mgf_gamma_slice_batch";
    SVMC_REQUIRE(phi && log_mgf && gammas_host && shortcut_host && normalizers && gamma_forwards && prices,
                 std::string(fn) + ": null pointer");
    SVMC_REQUIRE(n_strikes == 0 || (strikes_host && type_codes_host), std::string(fn) + ": null strikes or types");
    SVMC_REQUIRE(n_grid >= 3 && n_grid < (1u << 30), std::string(fn) + ": grid too short or too long");
    SVMC_REQUIRE(n_sets >= 1 && n_sets <= 65535, std::string(fn) + ": n_sets out of range");
    SVMC_REQUIRE(expiry >= 0, std::string(fn) + ": negative expiry");
    SVMC_REQUIRE(forward > 0.0 && std::isfinite(forward), std::string(fn) + ": forward must be positive and finite");
    for (int s = 0; s < n_sets; ++s)
        SVMC_REQUIRE(std::isfinite(gammas_host[s]), std::string(fn) + ": non-finite gamma");
    for (size_t k = 0; k < n_strikes; ++k) {
        SVMC_REQUIRE(strikes_host[k] > 0.0 && std::isfinite(strikes_host[k]), std::string(fn) + ": strikes must be positive");
        if (type_codes_host[k] != 0 && type_codes_host[k] != 1)   // :313-319: 'C' and 'P' only
            return fail(SVMC_ERR_UNKNOWN_PAYOFF, std::string(fn) + ": option type must be 'C' (0) or 'P' (1)");
    }
    const size_t nf_at = static_cast<size_t>(expiry) * static_cast<size_t>(n_sets);
    for (int s0 = 0; s0 < n_sets; s0 += HK_MAX_SETS) {
        const int m = (n_sets - s0 < HK_MAX_SETS) ? (n_sets - s0) : HK_MAX_SETS;
        for (size_t k0 = 0; k0 < n_strikes; k0 += MGF_SLICE_STRIKES) {
            GammaSliceArgs sa;
            sa.k = fill_strike_chunk(sa.x, strikes_host, k0, n_strikes,
                                     [&](double strike) { return log(forward / strike); });               // :304
            for (int k = 0; k < MGF_SLICE_STRIKES; ++k) {
                sa.strike[k] = (k < sa.k) ? strikes_host[k0 + k] : 1.0;
                sa.type[k] = (k < sa.k) ? type_codes_host[k0 + k] : 0;
            }
            for (int i = 0; i < HK_MAX_SETS; ++i) {
                sa.gamma[i] = gammas_host[s0 + (i < m ? i : 0)];
                sa.shortcut[i] = shortcut_host[s0 + (i < m ? i : 0)] != 0;
            }
            const size_t off = static_cast<size_t>(s0) * n_grid;
            hipLaunchKernelGGL(mgf_gamma_slice_kernel, dim3(sa.k, static_cast<unsigned>(m)), dim3(MGF_SLICE_BLOCK), 0,
                               as_stream(stream), reinterpret_cast<const cd *>(phi) + off, reinterpret_cast<const cd *>(log_mgf) + off,
                               static_cast<int>(n_grid), sa, normalizers + s0, gamma_forwards + s0, nf_at,
                               prices + static_cast<size_t>(s0) * n_strikes + k0, static_cast<int>(n_strikes));
        }
    }
    return check_launch(fn);
}

}  // extern "C"
