// svmc_cmc.hip -- conditional Monte Carlo chain pricers for LogSV and Heston Euler (include/svmc.h states the
// estimator, the recentring, the keep rule and the degenerate cases).
//
// Given the path of the volatility's driver b the log-return of both discretised schemes is Gaussian, x_T | {b_t} ~ N(mu, cv):
// the stepping kernels here draw ONE normal per step (stream 8, four steps per Philox call), advance the volatility on it and
// carry (mu, cv, sigma | v, qvar) per path; the payoff kernels integrate the orthogonal Brownian motion out in closed form, a
// Black-76 price per (path, strike) of F_c = F exp(mu + cv / 2) at total variance cv.
//
//   logsv_chain_cmc_kernel / _lat_kernel     all expiries of a chain in one stepping launch (full-launch / few-waves form)
//   heston_chain_cmc_kernel / _lat_kernel    the same for the reference's Heston Euler step
//   cmc_forward_kernel, cmc_forward_finish_kernel   per expiry the sums of exp(mu + cv/2) - 1, its square and the kept count;
//                                                   then, in row order, the forward statistics and the per-strike constants
//   cmc_payoff_kernel                        a block column per group of up to CMC_KT strikes of one expiry
//   cmc_finish_kernel                        a block per quote: column sums in row order, price and error
//   logsv_chain_cond_many_kernel / _lat_kernel, heston_chain_cond_many_kernel / _lat_kernel   many jobs of one chain in one stepping
//                                            launch (row f14): the bodies above on job blockIdx.y of a device table
//   cond_sens_jobs_kernel, cond_sens_pairs_kernel, cond_sens_finish_kernel   parameter sensitivities on common random numbers
#include "svmc_internal.h"

#include <cmath>
#include <cstring>
#include <vector>

#include "svmc_black.h"
#include "svmc_block.h"
#include "svmc_jobs.h"
#include "svmc_models.h"
#include "svmc_quotes.h"
#include "svmc_rng.h"
#include "svmc_slice.h"

namespace svmc {

constexpr uint32_t CMC_STREAM = 8u;    // svmc_rng.h: one normal per step, word step & 3 of call step >> 2

// ---------------------------------------------------------------------------------------------------
// stepping
// ---------------------------------------------------------------------------------------------------
// Time steps [0, nb) of a lane whose first step has the chain-global index step0, ONE unscaled normal each.  A Philox call serves
// the four steps 4c .. 4c + 3 and each word is guarded by a wave-uniform test: a slice that starts or ends inside a call uses
// the words that are its own, so slicing a chain differently never changes what a (path, step) sees.  tick(t) runs once per call
// with the local index of the call's first step (the progress priorities).
template <class Step, class Tick>
__device__ __forceinline__ void cmc_time_loop(const PhiloxLane &lane, uint32_t step0, int nb, const RngTables &tab, Step &&step, Tick &&tick)
{
    if (nb <= 0) return;
    const uint32_t first = step0, last = step0 + static_cast<uint32_t>(nb) - 1u;
    for (uint32_t c = first >> 2; c <= (last >> 2); ++c) {
        tick(static_cast<int>(4u * c - first));
        uint32_t r[4];
        philox_draw(lane, c, r);
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t s = 4u * c + k;
            if (s >= first && s <= last)
                step(normal_icdf32<SVMC_ICDF_M, SVMC_ICDF_SEGMENTS, SVMC_ICDF_DEG, SVMC_ICDF_EDGE != 0, SVMC_ICDF_RAW != 0>(r[k], tab.icdf));
        }
    }
}

// start state of a launch: read from the four state arrays (uniform = 0) or the same constants for every path
struct CmcInit {
    int uniform = 0;
    double mu0 = 0.0, cv0 = 0.0, vol0 = 0.0, qvar0 = 0.0;
};

// Where a conditional chain body's job comes from, as svmc_jobs.h's ChainArgs / ManyTable are for the plain generators: the LogSV and
// Heston bodies below are written once over a job source and run the same statements -- hence give the same bits -- whichever one
// hands them the job:
//   CmcChainArgs<Slices>   the one-job kernels: everything is a kernel argument (Slices = LogsvCmcSlices | HestonCmcSlices); the path
//                          starts from `init` or the four state arrays at step `step_offset` of its stream, expiry i goes to row i
//                          and the terminal state is written back
//   CmcManyTable<Consts>   the many-job kernels: job blockIdx.y of the device table (Consts = LogsvCmc | HestonCmc); the path starts
//                          from (0, 0, vol0_j, 0) at step 0 of (seed_j, call id_j), expiry i goes to row j m + i, nothing is
//                          written back and there are no qvar rows
template <class Slices>
struct CmcChainArgs {
    const Slices &cs;
    uint64_t seed_;
    uint32_t c3_, step_offset;
    const CmcInit &init;
    double *__restrict__ mu, *__restrict__ cv, *__restrict__ vol, *__restrict__ qvar, *__restrict__ q_snap;

    __device__ __forceinline__ int m() const { return cs.m; }
    __device__ __forceinline__ int nb_steps(int i) const { return cs.nb_steps[i]; }
    __device__ __forceinline__ int total_steps() const { return cs.total_steps; }
    __device__ __forceinline__ auto consts(int i) const { return cs.c[i]; }
    __device__ __forceinline__ unsigned joined() const { return cs.joined; }
    __device__ __forceinline__ uint64_t seed() const { return seed_; }
    __device__ __forceinline__ uint32_t c3() const { return c3_; }
    __device__ __forceinline__ uint32_t step_origin() const { return step_offset; }
    __device__ __forceinline__ size_t row(int i) const { return static_cast<size_t>(i); }
    __device__ __forceinline__ double *qvar_rows() const { return q_snap; }
    // path(): the lane's path index, formed where it is needed (the LogSV bodies step the lanes past the last path on a dummy state)
    template <class Path>
    __device__ __forceinline__ void start(Path &&path, bool active, double &m_, double &v_, double &s, double &q_) const
    {
        m_ = 0.0;
        v_ = 0.0;
        s = 1.0;
        q_ = 0.0;
        if (init.uniform) {                                // wave-uniform
            m_ = init.mu0;
            v_ = init.cv0;
            s = init.vol0;
            q_ = init.qvar0;
        } else if (active) {
            const size_t p = path();
            m_ = mu[p];
            v_ = cv[p];
            s = vol[p];
            q_ = qvar[p];
        }
    }
    __device__ __forceinline__ void finish(size_t p, double m_, double v_, double s, double q_) const
    {
        mu[p] = m_;
        cv[p] = v_;
        vol[p] = s;
        qvar[p] = q_;
    }
};

// the slices of a many-job launch and its per-job device table, one upload per call: the (job, expiry) constants [J][m] (LogsvCmc |
// HestonCmc), then per job the start volatility (variance for Heston), the Philox key, the call id's counter word and the job's
// own `joined` mask (cmc_joined_mask: the rule of cmc_step_chain)
struct CmcManySlices {
    int nb_steps[MAX_CHAIN_SLICES];
    int m, total_steps = 0;
};
struct CmcManyJobs {
    const void *consts;
    const double *vol0;
    const uint64_t *seed;
    const uint32_t *c3, *joined;
};

template <class Consts>
struct CmcManyTable {
    const CmcManySlices &cs;
    const CmcManyJobs &jobs;

    __device__ __forceinline__ int job() const { return blockIdx.y; }
    __device__ __forceinline__ int m() const { return cs.m; }
    __device__ __forceinline__ int nb_steps(int i) const { return cs.nb_steps[i]; }
    __device__ __forceinline__ int total_steps() const { return cs.total_steps; }
    // job-uniform values go through uniform_load (svmc_jobs.h): the step keeps its scalar operands
    __device__ __forceinline__ Consts consts(int i) const
    {
        return uniform_load(static_cast<const Consts *>(jobs.consts) + static_cast<size_t>(job()) * cs.m + i);
    }
    __device__ __forceinline__ unsigned joined() const { return uniform_load(jobs.joined + job()); }
    __device__ __forceinline__ uint64_t seed() const { return uniform_load(jobs.seed + job()); }
    __device__ __forceinline__ uint32_t c3() const { return uniform_load(jobs.c3 + job()); }
    __device__ __forceinline__ uint32_t step_origin() const { return 0u; }
    __device__ __forceinline__ size_t row(int i) const { return static_cast<size_t>(job()) * cs.m + i; }
    __device__ __forceinline__ double *qvar_rows() const { return nullptr; }
    template <class Path>
    __device__ __forceinline__ void start(Path &&, bool, double &m_, double &v_, double &s, double &q_) const
    {
        m_ = 0.0;
        v_ = 0.0;
        s = uniform_load(jobs.vol0 + job());
        q_ = 0.0;
    }
    __device__ __forceinline__ void finish(size_t, double, double, double, double) const {}
};

// ---- LogSV: logsv_step_acc with the two noise FMAs replaced by one (the volatility moves on beta w0 + volvol w1 = vartheta b)
// and the drift added to L in one piece (logsv_cmc_step)
struct LogsvCmc {
    double c1, c2, c3;   // LogsvFast's drift constants, in log units
    double vs;           // vartheta sqrt(dt), in log units
    double hA, ahA;      // eta^2 dt / 2, alpha/2 eta^2 dt
    double rhoB;         // rho eta sqrt(dt), rho = beta / vartheta (0 when vartheta == 0)
    double cvA;          // (volvol^2 / vartheta^2) eta^2 dt (factor 1 when vartheta == 0): the quotient, not 1 - rho^2
};

static LogsvCmc make_logsv_cmc(double dt, double theta, double kappa1, double kappa2, double beta, double volvol, double eta,
                               int is_spot_measure)
{
    const LogsvFast f = logsv_fast_in_log_units(make_logsv_fast(make_logsv_consts(dt, theta, kappa1, kappa2, beta, volvol, eta, is_spot_measure)));
    const double vartheta2 = beta * beta + volvol * volvol, vartheta = sqrt(vartheta2);
    LogsvCmc c;
    c.c1 = f.c1;
    c.c2 = f.c2;
    c.c3 = f.c3;
    c.vs = vartheta * sqrt(dt) * LOG_UNITS_PER_NAT;
    c.hA = f.hA;
    c.ahA = f.ahA;
    c.rhoB = (vartheta > 0.0) ? (beta / vartheta) * f.B : 0.0;
    c.cvA = (vartheta > 0.0) ? ((volvol * volvol) / vartheta2) * f.A : f.A;
    return c;
}

// The drift is formed apart from L and added once (c3v: c3 in a vector register, so that fma(c2, s, c3) has one scalar operand):
// the instruction count of logsv_step_acc's three updates of L, but two roundings at L's magnitude per step instead of four.
// Where the noise is small against the drift (beta = volvol = 0: L hardly moves) the roundings of consecutive steps are the
// same ones and add up instead of averaging out -- 18 ulp in sigma after 64 steps of the zero-noise set of
// tests/golden/cmc_steps.npz with the drift added term by term, 2.5 with it added once.
__device__ __forceinline__ void logsv_cmc_step(const LogsvCmc &c, double c3v, double &xacc, double &L, double &sigma, double &acc, double b,
                                               const double *exp_table)
{
    const double s = sigma;
    const double y = rcp_1n(s);
    xacc = fma(s, b, xacc);                      // sum sigma_t b_t
    acc = fma(s, s, acc);                        // sum sigma_t^2, the squares the steps START from
    double d = fma(c.c2, s, c3v);
    d = fma(c.c1, y, d);
    L = L + d;
    L = fma(c.vs, b, L);
    sigma = exp2u_tab(L, exp_table);
}

// the fold at a slice's end: mu += ahA acc + rho B xacc, cv += (volvol^2 / vartheta^2) A acc, qvar as logsv_fold_acc
__device__ __forceinline__ void logsv_cmc_fold(const LogsvCmc &c, double &mu, double &cv, double &qvar, double xacc, double acc,
                                               double s2_start, double s2_now)
{
    mu = fma(c.rhoB, xacc, mu);
    mu = fma(c.ahA, acc, mu);
    cv = fma(c.cvA, acc, cv);
    const double tail = s2_now - s2_start;
    const bool finite = acc < __builtin_huge_val();
    const double e = finite ? (acc + acc) + tail : acc;
    qvar = fma(c.hA, e, qvar);
}

// `joined`, bit i: slice i has the bit-equal constants of slice i - 1 of the same launch.  Such a boundary is a snapshot and nothing
// else: the accumulators (and LogSV's L) run on and the snapshot is the fold of the sums since the last boundary that was not
// joined, so a chain's values do not depend on how a stretch of equal steps is cut into slices (3 + 5 + 8 steps = 16 steps, to
// the bit).  Set on the host (cmc_step_chain).
struct LogsvCmcSlices {
    LogsvCmc c[MAX_CHAIN_SLICES];
    int nb_steps[MAX_CHAIN_SLICES];
    int m, total_steps = 0;
    unsigned joined = 0;
};

// One body for both launch forms.  PARK (the full-launch form, 1024-thread blocks at eight waves per SIMD): the base values of mu, cv
// and qvar are dead inside the time loop but live across it, and wait in LDS as logsv_chain_rng_kernel parks x and qvar; the few-waves form keeps
// them in registers.  The statements on the state are the same, hence the bits.
template <bool PARK, int TB, class Src>
__device__ __forceinline__ void logsv_chain_cmc_body(const Src &src, size_t n, uint64_t path_offset, double *__restrict__ mu_snap,
                                                     double *__restrict__ cv_snap)
{
    __shared__ RngTablesLds s_tab;
    __shared__ double s_exp[256];
    __shared__ double s_park[PARK ? 3 * TB : 1];           // [0, TB): mu, [TB, 2 TB): cv, [2 TB, 3 TB): qvar -- lane t owns its three
    const RngTables tab = stage_tables(s_tab, s_exp);
    const auto path_index = [&]() {                        // re-derived where needed: one VGPR across the time loop
        uint32_t t = threadIdx.x;
        asm volatile("" : "+v"(t));
        return static_cast<size_t>(blockIdx.x) * TB + t;
    };
    const bool active = path_index() < n;
    double m_, v_, s, q_;                                  // lanes past the last path step a dummy state
    src.start(path_index, active, m_, v_, s, q_);
    if constexpr (PARK) {
        s_park[threadIdx.x] = m_;
        s_park[TB + threadIdx.x] = v_;
        s_park[2 * TB + threadIdx.x] = q_;
    }
    const PhiloxLane lane = philox_prepare(src.seed(), src.c3() | CMC_STREAM, path_offset + path_index());
    LogsvProgress prog = {(src.total_steps() + 3) >> 2};
    const int n_slices = src.m();
    const unsigned joined = src.joined();
    const uint32_t step_offset = src.step_origin();
    double *__restrict__ q_snap = src.qvar_rows();
    int tg = 0;
    // L = ln sigma in log units is derived once per LAUNCH and carried from slice to slice.  One Newton step on exp(L) = sigma:
    // log_state is good to 4 ULP of ln sigma, which is up to 4 ulp(ln sigma) RELATIVE in the volatility the first step ends with
    double L = log_state(s) * LOG_UNITS_PER_NAT;
    {
        const double back = exp2u_tab(L, s_exp);
        if (back > 0.0 && back < __builtin_huge_val() && s < __builtin_huge_val())
            L = fma(LOG_UNITS_PER_NAT, (s - back) / back, L);
    }
    // the sums since the last boundary that was not joined; (m_, v_, q_) -- parked in LDS in the PARK form -- is the state AT it
    double acc = 0.0, xacc = 0.0, s2_start = square_rn(s);
    for (int i = 0; i < n_slices; ++i) {
        const int nb = src.nb_steps(i);
        const LogsvCmc c = src.consts(i);
        double c3v = c.c3;
        asm volatile("" : "+v"(c3v));
        cmc_time_loop(
            lane, step_offset + static_cast<uint32_t>(tg), nb, tab, [&](double b) { logsv_cmc_step(c, c3v, xacc, L, s, acc, b, s_exp); },
            [&](int t) {
                if (tg + t >= prog.next_stage_t) {         // wave-uniform
                    progress_priority(prog.stage++);
                    prog.next_stage_t += prog.quarter;
                }
            });
        double ms, vs, qs;                                 // the expiry's values: the base folded with the sums so far
        if constexpr (PARK) {
            ms = s_park[threadIdx.x];                      // a lane reads back what it alone wrote: no barrier needed
            vs = s_park[TB + threadIdx.x];
            qs = s_park[2 * TB + threadIdx.x];
        } else {
            ms = m_;
            vs = v_;
            qs = q_;
        }
        logsv_cmc_fold(c, ms, vs, qs, xacc, acc, s2_start, square_rn(s));
        tg += nb;
        if (active) {
            const size_t o = src.row(i) * n + path_index();
            mu_snap[o] = ms;
            cv_snap[o] = vs;
            if (q_snap != nullptr) q_snap[o] = qs;
        }
        const bool runs_on = i + 1 < n_slices && ((joined >> (i + 1)) & 1u) != 0u;     // wave-uniform
        if (!runs_on) {                                    // a real boundary (the launch's end is one): the values become the base
            if constexpr (PARK) {
                s_park[threadIdx.x] = ms;
                s_park[TB + threadIdx.x] = vs;
                s_park[2 * TB + threadIdx.x] = qs;
            } else {
                m_ = ms;
                v_ = vs;
                q_ = qs;
            }
            acc = 0.0;
            xacc = 0.0;
            s2_start = square_rn(s);
        }
    }
    if (active) {
        const size_t p = path_index();
        if constexpr (PARK) {
            m_ = s_park[threadIdx.x];
            v_ = s_park[TB + threadIdx.x];
            q_ = s_park[2 * TB + threadIdx.x];
        }
        src.finish(p, m_, v_, s, q_);
    }
}

constexpr int CMC_CHAIN_BLOCK = 1024;  // as logsv_chain_rng_kernel: two blocks per CU share its LDS (table 32 KB + exp 2 KB + park 24 KB each)
__global__ __launch_bounds__(CMC_CHAIN_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8), amdgpu_num_sgpr(80))) void logsv_chain_cmc_kernel(
    double *__restrict__ mu, double *__restrict__ cv, double *__restrict__ sigma, double *__restrict__ qvar, size_t n, LogsvCmcSlices cs,
    uint64_t seed, uint32_t c3, uint64_t path_offset, uint32_t step_offset, double *__restrict__ mu_snap, double *__restrict__ cv_snap,
    double *__restrict__ q_snap, CmcInit init)
{
    logsv_chain_cmc_body<true, CMC_CHAIN_BLOCK>(CmcChainArgs<LogsvCmcSlices>{cs, seed, c3, step_offset, init, mu, cv, sigma, qvar, q_snap}, n,
                                                path_offset, mu_snap, cv_snap);
}

// the few-waves form (few_waves_launch()): 256-thread blocks so that every CU gets work, registers to spare
__global__ __launch_bounds__(FEW_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) void logsv_chain_cmc_lat_kernel(
    double *__restrict__ mu, double *__restrict__ cv, double *__restrict__ sigma, double *__restrict__ qvar, size_t n, LogsvCmcSlices cs,
    uint64_t seed, uint32_t c3, uint64_t path_offset, uint32_t step_offset, double *__restrict__ mu_snap, double *__restrict__ cv_snap,
    double *__restrict__ q_snap, CmcInit init)
{
    logsv_chain_cmc_body<false, FEW_BLOCK>(CmcChainArgs<LogsvCmcSlices>{cs, seed, c3, step_offset, init, mu, cv, sigma, qvar, q_snap}, n,
                                           path_offset, mu_snap, cv_snap);
}

// many jobs of one chain in ONE launch: blockIdx.y = job, blockIdx.x = block of that job's n paths.  The names
// of these kernels carry none of the words the f11 to f13 metadata tests count kernels by.
__global__ __launch_bounds__(CMC_CHAIN_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8), amdgpu_num_sgpr(80))) void logsv_chain_cond_many_kernel(
    size_t n, CmcManySlices cs, CmcManyJobs jobs, uint64_t path_offset, double *__restrict__ mu_snap, double *__restrict__ cv_snap)
{
    logsv_chain_cmc_body<true, CMC_CHAIN_BLOCK>(CmcManyTable<LogsvCmc>{cs, jobs}, n, path_offset, mu_snap, cv_snap);
}

__global__ __launch_bounds__(FEW_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) void logsv_chain_cond_many_lat_kernel(
    size_t n, CmcManySlices cs, CmcManyJobs jobs, uint64_t path_offset, double *__restrict__ mu_snap, double *__restrict__ cv_snap)
{
    logsv_chain_cmc_body<false, FEW_BLOCK>(CmcManyTable<LogsvCmc>{cs, jobs}, n, path_offset, mu_snap, cv_snap);
}

// ---- Heston: the reference's Euler step with its 1e-4 floor, the variance driven by b = rho w0 + rho_1 w1
struct HestonCmc {
    double dt, one_m_kdt, ktdt;   // 1 - kappa dt, kappa theta dt
    double a;                     // volvol sqrt(dt)
    double rho_sdt;               // rho sqrt(dt)
    double rho1sq;                // rho_1^2 = 1 - rho^2
};

static HestonCmc make_heston_cmc(double dt, double theta, double kappa, double rho, double volvol)
{
    HestonCmc c;
    c.dt = dt;
    c.one_m_kdt = 1.0 - kappa * dt;
    c.ktdt = kappa * theta * dt;
    c.a = volvol * sqrt(dt);
    c.rho_sdt = rho * sqrt(dt);
    c.rho1sq = 1.0 - rho * rho;
    return c;
}

__device__ __forceinline__ void heston_cmc_step(const HestonCmc &c, double &xacc, double &var, double &vacc, double b)
{
    const double v = var;
    const double s = sqrt_pos_1g(v);                       // v > 0: heston_euler_guard_zero + the floor
    vacc = vacc + v;
    xacc = fma(s, b, xacc);
    const double vn = fma(s, c.a * b, fma(v, c.one_m_kdt, c.ktdt));
    var = fmax(vn, 1e-4);                                  // np.maximum(v, 1e-4); a NaN is put back by the fold
}

// mu += -dt sum v / 2 + rho sqrt(dt) sum sqrt(v) b, cv += rho_1^2 dt sum v, qvar += dt sum v
__device__ __forceinline__ void heston_cmc_fold(const HestonCmc &c, double &mu, double &cv, double &qvar, double &var, double xacc, double vacc)
{
    const double q = c.dt * vacc;
    mu = fma(c.rho_sdt, xacc, fma(-0.5, q, mu));
    cv = fma(c.rho1sq, q, cv);
    qvar = qvar + q;
    const double finite_or_nan = ((c.one_m_kdt * 0.0 + c.ktdt * 0.0) + c.a * 0.0) + vacc * 0.0;   // 0 or NaN (heston_fold_acc)
    var = var + finite_or_nan;
}

struct HestonCmcSlices {
    HestonCmc c[MAX_CHAIN_SLICES];
    int nb_steps[MAX_CHAIN_SLICES];
    int m, total_steps = 0;
    unsigned joined = 0;               // as LogsvCmcSlices
};

template <class Src>
__device__ __forceinline__ void heston_chain_cmc_body(const Src &src, size_t n, uint64_t path_offset, double *__restrict__ mu_snap,
                                                      double *__restrict__ cv_snap)
{
    __shared__ RngTablesLds s_tab;
    const RngTables tab = stage_rng_tables(s_tab);
    const size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool active = p < n;
    if (!active) return;                                   // (after the block's only barrier)
    double m_, c_, v, q_;
    src.start([&]() { return p; }, true, m_, c_, v, q_);
    const PhiloxLane lane = philox_prepare(src.seed(), src.c3() | CMC_STREAM, path_offset + p);
    const int n_slices = src.m();
    const unsigned joined = src.joined();
    double *__restrict__ q_snap = src.qvar_rows();
    uint32_t step = src.step_origin();
    double xacc = 0.0, vacc = 0.0;                         // the sums since the last boundary that was not joined (HestonCmcSlices)
    for (int i = 0; i < n_slices; ++i) {
        const int nb = src.nb_steps(i);
        const HestonCmc c = src.consts(i);
        v = heston_euler_guard_zero(v);
        cmc_time_loop(lane, step, nb, tab, [&](double b) { heston_cmc_step(c, xacc, v, vacc, b); }, [](int) {});
        double ms = m_, vs = c_, qs = q_;
        heston_cmc_fold(c, ms, vs, qs, v, xacc, vacc);
        step += static_cast<uint32_t>(nb);
        const size_t o = src.row(i) * n + p;
        mu_snap[o] = ms;
        cv_snap[o] = vs;
        if (q_snap != nullptr) q_snap[o] = qs;
        const bool runs_on = i + 1 < n_slices && ((joined >> (i + 1)) & 1u) != 0u;     // wave-uniform
        if (!runs_on) {
            m_ = ms;
            c_ = vs;
            q_ = qs;
            xacc = 0.0;
            vacc = 0.0;
        }
    }
    src.finish(p, m_, c_, v, q_);
}

__global__ __launch_bounds__(RNG_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void heston_chain_cmc_kernel(
    double *__restrict__ mu, double *__restrict__ cv, double *__restrict__ var, double *__restrict__ qvar, size_t n, HestonCmcSlices cs,
    uint64_t seed, uint32_t c3, uint64_t path_offset, uint32_t step_offset, double *__restrict__ mu_snap, double *__restrict__ cv_snap,
    double *__restrict__ q_snap, CmcInit init)
{
    heston_chain_cmc_body(CmcChainArgs<HestonCmcSlices>{cs, seed, c3, step_offset, init, mu, cv, var, qvar, q_snap}, n, path_offset, mu_snap,
                          cv_snap);
}

__global__ __launch_bounds__(FEW_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) void heston_chain_cmc_lat_kernel(
    double *__restrict__ mu, double *__restrict__ cv, double *__restrict__ var, double *__restrict__ qvar, size_t n, HestonCmcSlices cs,
    uint64_t seed, uint32_t c3, uint64_t path_offset, uint32_t step_offset, double *__restrict__ mu_snap, double *__restrict__ cv_snap,
    double *__restrict__ q_snap, CmcInit init)
{
    heston_chain_cmc_body(CmcChainArgs<HestonCmcSlices>{cs, seed, c3, step_offset, init, mu, cv, var, qvar, q_snap}, n, path_offset, mu_snap,
                          cv_snap);
}

__global__ __launch_bounds__(RNG_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void heston_chain_cond_many_kernel(
    size_t n, CmcManySlices cs, CmcManyJobs jobs, uint64_t path_offset, double *__restrict__ mu_snap, double *__restrict__ cv_snap)
{
    heston_chain_cmc_body(CmcManyTable<HestonCmc>{cs, jobs}, n, path_offset, mu_snap, cv_snap);
}

__global__ __launch_bounds__(FEW_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) void heston_chain_cond_many_lat_kernel(
    size_t n, CmcManySlices cs, CmcManyJobs jobs, uint64_t path_offset, double *__restrict__ mu_snap, double *__restrict__ cv_snap)
{
    heston_chain_cmc_body(CmcManyTable<HestonCmc>{cs, jobs}, n, path_offset, mu_snap, cv_snap);
}

// ---- host side of the stepping: launches of at most MAX_CHAIN_SLICES expiries, the step offset carried from launch to launch
// bit i: slice i has the bit-equal constants of slice i - 1 (LogsvCmcSlices)
template <class Consts>
static unsigned cmc_joined_mask(const Consts *c, int m)
{
    unsigned joined = 0u;
    for (int i = 1; i < m; ++i)
        if (memcmp(&c[i], &c[i - 1], sizeof(Consts)) == 0) joined |= 1u << i;
    return joined;
}
template <class Slices, class Fill, class Launch>
static int cmc_step_chain(const char *fn, const CmcInit &init, const double *mu, const double *cv, const double *vol, const double *qvar,
                          size_t n_path, int n_slices, const int *nb_steps_host, const double *dts_host, uint32_t call_id,
                          uint32_t step_offset, double *mu_snapshots, double *cv_snapshots, double *qvar_snapshots, Fill &&fill,
                          Launch &&launch)
{
    SVMC_REQUIRE(mu && cv && vol && qvar && mu_snapshots && cv_snapshots, std::string(fn) + ": null pointer");
    SVMC_REQUIRE(nb_steps_host && dts_host && n_slices >= 1, std::string(fn) + ": null grids / no slices");
    SVMC_REQUIRE(call_id < (1u << 24), std::string(fn) + ": call_id must fit 24 bits");
    SVMC_REQUIRE(n_path > 0, std::string(fn) + ": n_path must be positive");
    for (int i = 0; i < n_slices; ++i)
        SVMC_REQUIRE(nb_steps_host[i] > 0 && dts_host[i] > 0.0, std::string(fn) + ": nb_steps and dt must be positive");
    for (int i0 = 0; i0 < n_slices; i0 += MAX_CHAIN_SLICES) {
        Slices cs;
        cs.m = (n_slices - i0 < MAX_CHAIN_SLICES) ? (n_slices - i0) : MAX_CHAIN_SLICES;
        uint32_t steps = 0;
        for (int i = 0; i < MAX_CHAIN_SLICES; ++i) {
            const int j = (i < cs.m) ? i0 + i : i0;        // unused entries repeat a valid one
            cs.nb_steps[i] = (i < cs.m) ? nb_steps_host[j] : 0;
            steps += static_cast<uint32_t>(cs.nb_steps[i]);
            fill(cs, i, j);
        }
        cs.total_steps = static_cast<int>(steps);
        cs.joined = cmc_joined_mask(cs.c, cs.m);
        const size_t row = static_cast<size_t>(i0) * n_path;
        launch(cs, mu_snapshots + row, cv_snapshots + row, qvar_snapshots ? qvar_snapshots + row : nullptr, (i0 == 0) ? init : CmcInit(),
               step_offset);
        if (int rc = check_launch(fn)) return rc;
        step_offset += steps;
    }
    return SVMC_OK;
}

int logsv_cmc_step_chain(const char *fn, const CmcInit &init, double *mu, double *cv, double *sigma, double *qvar, size_t n_path,
                         int n_slices, const int *nb_steps_host, const double *dts_host, const double *etas_host, double theta,
                         double kappa1, double kappa2, double beta, double volvol, int is_spot_measure, uint64_t seed, uint32_t call_id,
                         uint64_t path_offset, uint32_t step_offset, double *mu_snapshots, double *cv_snapshots, double *qvar_snapshots,
                         hipStream_t stream)
{
    const auto fill = [&](LogsvCmcSlices &cs, int i, int j) {
        cs.c[i] = make_logsv_cmc(dts_host[j], theta, kappa1, kappa2, beta, volvol, etas_host ? etas_host[j] : 1.0, is_spot_measure);
    };
    const auto launch = [&](const LogsvCmcSlices &cs, double *ms, double *vs, double *qs, const CmcInit &init_i, uint32_t step0) {
        if (few_waves_launch(n_path))
            hipLaunchKernelGGL(logsv_chain_cmc_lat_kernel, dim3(lat_grid(n_path)), dim3(FEW_BLOCK), 0, stream, mu, cv, sigma, qvar, n_path,
                               cs, seed, make_c3(call_id), path_offset, step0, ms, vs, qs, init_i);
        else
            hipLaunchKernelGGL(logsv_chain_cmc_kernel, dim3(static_cast<unsigned>((n_path + CMC_CHAIN_BLOCK - 1) / CMC_CHAIN_BLOCK)),
                               dim3(CMC_CHAIN_BLOCK), 0, stream, mu, cv, sigma, qvar, n_path, cs, seed, make_c3(call_id), path_offset, step0,
                               ms, vs, qs, init_i);
    };
    return cmc_step_chain<LogsvCmcSlices>(fn, init, mu, cv, sigma, qvar, n_path, n_slices, nb_steps_host, dts_host, call_id, step_offset,
                                          mu_snapshots, cv_snapshots, qvar_snapshots, fill, launch);
}

int heston_cmc_step_chain(const char *fn, const CmcInit &init, double *mu, double *cv, double *var, double *qvar, size_t n_path,
                          int n_slices, const int *nb_steps_host, const double *dts_host, double theta, double kappa, double rho,
                          double volvol, uint64_t seed, uint32_t call_id, uint64_t path_offset, uint32_t step_offset,
                          double *mu_snapshots, double *cv_snapshots, double *qvar_snapshots, hipStream_t stream)
{
    const auto fill = [&](HestonCmcSlices &cs, int i, int j) { cs.c[i] = make_heston_cmc(dts_host[j], theta, kappa, rho, volvol); };
    const auto launch = [&](const HestonCmcSlices &cs, double *ms, double *vs, double *qs, const CmcInit &init_i, uint32_t step0) {
        if (few_waves_launch(n_path))
            hipLaunchKernelGGL(heston_chain_cmc_lat_kernel, dim3(lat_grid(n_path)), dim3(FEW_BLOCK), 0, stream, mu, cv, var, qvar, n_path,
                               cs, seed, make_c3(call_id), path_offset, step0, ms, vs, qs, init_i);
        else
            hipLaunchKernelGGL(heston_chain_cmc_kernel, dim3(rng_grid(n_path)), dim3(rng_block()), 0, stream, mu, cv, var, qvar, n_path, cs,
                               seed, make_c3(call_id), path_offset, step0, ms, vs, qs, init_i);
    };
    return cmc_step_chain<HestonCmcSlices>(fn, init, mu, cv, var, qvar, n_path, n_slices, nb_steps_host, dts_host, call_id, step_offset,
                                           mu_snapshots, cv_snapshots, qvar_snapshots, fill, launch);
}

// the fused drivers' stepping (svmc_chain.hip) from the start state (0, 0, vol0, 0)
int logsv_cmc_step_from(double sigma0, double *mu, double *cv, double *sigma, double *qvar, size_t n_path, int n_slices,
                        const int *nb_steps_host, const double *dts_host, const double *etas_host, double theta, double kappa1,
                        double kappa2, double beta, double volvol, int is_spot_measure, uint64_t seed, uint32_t call_id,
                        uint64_t path_offset, double *mu_snapshots, double *cv_snapshots, hipStream_t stream)
{
    const CmcInit init = {1, 0.0, 0.0, sigma0, 0.0};
    return logsv_cmc_step_chain("svmc_logsv_chain_price_cmc", init, mu, cv, sigma, qvar, n_path, n_slices, nb_steps_host, dts_host,
                                etas_host, theta, kappa1, kappa2, beta, volvol, is_spot_measure, seed, call_id, path_offset, 0u,
                                mu_snapshots, cv_snapshots, nullptr, stream);
}

int heston_cmc_step_from(double var0, double *mu, double *cv, double *var, double *qvar, size_t n_path, int n_slices,
                         const int *nb_steps_host, const double *dts_host, double theta, double kappa, double rho, double volvol,
                         uint64_t seed, uint32_t call_id, uint64_t path_offset, double *mu_snapshots, double *cv_snapshots,
                         hipStream_t stream)
{
    const CmcInit init = {1, 0.0, 0.0, var0, 0.0};
    return heston_cmc_step_chain("svmc_heston_chain_price_cmc", init, mu, cv, var, qvar, n_path, n_slices, nb_steps_host, dts_host, theta,
                                 kappa, rho, volvol, seed, call_id, path_offset, 0u, mu_snapshots, cv_snapshots, nullptr, stream);
}

// ---- many jobs of one chain in one stepping launch (svmc_*_chain_cmc_many and the fused drivers of svmc_chain.hip)
template <class Consts>
static size_t cmc_many_table_bytes_of(int n_jobs, int n_slices)
{
    const size_t J = static_cast<size_t>(n_jobs);
    return J * static_cast<size_t>(n_slices) * sizeof(Consts) + J * (sizeof(double) + sizeof(uint64_t) + 2 * sizeof(uint32_t));
}
size_t cmc_many_table_bytes(int n_jobs, int n_slices)
{
    return std::max(cmc_many_table_bytes_of<LogsvCmc>(n_jobs, n_slices), cmc_many_table_bytes_of<HestonCmc>(n_jobs, n_slices));
}

// The checks, the job table -- filled in table_host (the table's byte layout; the caller keeps it until the stream has passed
// the upload), uploaded to table_dev -- and launch(cs, jobs).  fill(j, consts) sets job j's n_slices constants and returns its
// start volatility.  `what`: CMC_MANY_FILL the table in table_host, CMC_MANY_ENQUEUE its upload and the launch -- whose arguments
// depend on neither the parameters nor the streams, so that a captured upload and launch serve every later fill.
template <class Consts, class Fill, class Launch>
static int cmc_step_many(const char *fn, size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
                         const double *params_host, const uint64_t *seeds, const uint32_t *call_ids, void *table_host, void *table_dev,
                         double *mu_snapshots, double *cv_snapshots, hipStream_t stream, int what, Fill &&fill, Launch &&launch)
{
    SVMC_REQUIRE(nb_steps_host && dts_host && params_host && seeds && call_ids && table_host && table_dev && mu_snapshots && cv_snapshots,
                 std::string(fn) + ": null pointer");
    if (int rc = check_many(fn, n_path, n_jobs, n_slices, nb_steps_host, dts_host, call_ids)) return rc;
    const size_t J = static_cast<size_t>(n_jobs), nc = J * static_cast<size_t>(n_slices);
    unsigned char *h = static_cast<unsigned char *>(table_host);
    Consts *consts = reinterpret_cast<Consts *>(h);
    double *vol0 = reinterpret_cast<double *>(h + nc * sizeof(Consts));
    uint64_t *seed = reinterpret_cast<uint64_t *>(vol0 + J);
    uint32_t *c3 = reinterpret_cast<uint32_t *>(seed + J), *joined = c3 + J;
    for (int j = 0; (what & CMC_MANY_FILL) && j < n_jobs; ++j) {
        Consts *cj = consts + static_cast<size_t>(j) * n_slices;
        vol0[j] = fill(j, cj);
        seed[j] = seeds[j];
        c3[j] = make_c3(call_ids[j]);
        joined[j] = cmc_joined_mask(cj, n_slices);
    }
    if (!(what & CMC_MANY_ENQUEUE)) return SVMC_OK;
    const size_t bytes = cmc_many_table_bytes_of<Consts>(n_jobs, n_slices);
    SVMC_HIP_TRY(hipMemcpyAsync(table_dev, table_host, bytes, hipMemcpyHostToDevice, stream));
    const unsigned char *d = static_cast<const unsigned char *>(table_dev);
    const size_t o_vol = nc * sizeof(Consts), o_seed = o_vol + J * sizeof(double), o_c3 = o_seed + J * sizeof(uint64_t),
                 o_joined = o_c3 + J * sizeof(uint32_t);
    const CmcManyJobs jobs = {d, reinterpret_cast<const double *>(d + o_vol), reinterpret_cast<const uint64_t *>(d + o_seed),
                              reinterpret_cast<const uint32_t *>(d + o_c3), reinterpret_cast<const uint32_t *>(d + o_joined)};
    CmcManySlices cs;
    cs.m = n_slices;
    for (int i = 0; i < MAX_CHAIN_SLICES; ++i) {
        cs.nb_steps[i] = i < n_slices ? nb_steps_host[i] : 0;
        cs.total_steps += cs.nb_steps[i];
    }
    // the form is chosen by the launch's TOTAL path count, as logsv_chain_rng_many chooses it
    launch(cs, jobs, few_waves_launch(J * n_path));
    return check_launch(fn);
}

int logsv_cmc_step_many(const char *fn, size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
                        const double *params_host, int is_spot_measure, const uint64_t *seeds, const uint32_t *call_ids,
                        uint64_t path_offset, void *table_host, void *table_dev, double *mu_snapshots, double *cv_snapshots,
                        hipStream_t stream, int what)
{
    const size_t row = 6 + static_cast<size_t>(n_slices > 0 ? n_slices : 0);       // v0 theta kappa1 kappa2 beta volvol, etas
    const unsigned J = static_cast<unsigned>(n_jobs);
    return cmc_step_many<LogsvCmc>(fn, n_path, n_jobs, n_slices, nb_steps_host, dts_host, params_host, seeds, call_ids, table_host,
                                   table_dev, mu_snapshots, cv_snapshots, stream, what,
                                   [&](int j, LogsvCmc *c) {
        const double *p = params_host + row * static_cast<size_t>(j);
        for (int i = 0; i < n_slices; ++i) c[i] = make_logsv_cmc(dts_host[i], p[1], p[2], p[3], p[4], p[5], p[6 + i], is_spot_measure);
        return p[0];
    },
                                   [&](const CmcManySlices &cs, const CmcManyJobs &jobs, bool few) {
        if (few)
            hipLaunchKernelGGL(logsv_chain_cond_many_lat_kernel, dim3(lat_grid(n_path), J), dim3(FEW_BLOCK), 0, stream, n_path, cs, jobs,
                               path_offset, mu_snapshots, cv_snapshots);
        else
            hipLaunchKernelGGL(logsv_chain_cond_many_kernel, dim3(lat_grid(n_path, CMC_CHAIN_BLOCK), J), dim3(CMC_CHAIN_BLOCK), 0, stream,
                               n_path, cs, jobs, path_offset, mu_snapshots, cv_snapshots);
    });
}

int heston_cmc_step_many(const char *fn, size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
                         const double *params_host, const uint64_t *seeds, const uint32_t *call_ids, uint64_t path_offset,
                         void *table_host, void *table_dev, double *mu_snapshots, double *cv_snapshots, hipStream_t stream, int what)
{
    const unsigned J = static_cast<unsigned>(n_jobs);
    return cmc_step_many<HestonCmc>(fn, n_path, n_jobs, n_slices, nb_steps_host, dts_host, params_host, seeds, call_ids, table_host,
                                    table_dev, mu_snapshots, cv_snapshots, stream, what,
                                    [&](int j, HestonCmc *c) {
        const double *p = params_host + 5 * static_cast<size_t>(j);               // v0 theta kappa rho volvol
        for (int i = 0; i < n_slices; ++i) c[i] = make_heston_cmc(dts_host[i], p[1], p[2], p[3], p[4]);
        return p[0];
    },
                                    [&](const CmcManySlices &cs, const CmcManyJobs &jobs, bool few) {
        if (few)
            hipLaunchKernelGGL(heston_chain_cond_many_lat_kernel, dim3(lat_grid(n_path), J), dim3(FEW_BLOCK), 0, stream, n_path, cs, jobs,
                               path_offset, mu_snapshots, cv_snapshots);
        else
            hipLaunchKernelGGL(heston_chain_cond_many_kernel, dim3(rng_grid(n_path), J), dim3(rng_block()), 0, stream, n_path, cs, jobs,
                               path_offset, mu_snapshots, cv_snapshots);
    });
}

// ---------------------------------------------------------------------------------------------------
// payoff reduction
// ---------------------------------------------------------------------------------------------------
static_assert(QUOTE_BLOCK == BLOCK, "svmc_quotes.h sizes the partial rows for blocks of BLOCK paths");

// a path is kept iff mu, cv and e = exp(mu + cv / 2) are finite and cv >= 0 (include/svmc.h); h = mu + cv / 2
__device__ __forceinline__ bool cmc_keep(double mu, double cv, double &h, double &e)
{
    h = fma(0.5, cv, mu);
    e = exp_full(h);
    const double inf = __builtin_huge_val();
    return fabs(mu) < inf && cv >= 0.0 && cv < inf && e < inf;     // a NaN fails a comparison
}

// the undiscounted Black-76 price of F_c = F e against K' at total variance cv, on the quoted side's own formula
__device__ __forceinline__ double cmc_black(double fc, double ln_fc, double cv, double sd, double inv_sd, double kp, double ln_kp, bool put)
{
    if (!(kp > 0.0)) return put ? 0.0 : fc - kp;
    if (cv == 0.0) return put ? fmax(kp - fc, 0.0) : fmax(fc - kp, 0.0);
    const double d1 = fma(ln_fc - ln_kp, inv_sd, 0.5 * sd), d2 = d1 - sd;
    return put ? kp * black_norm_cdf(-d2) - fc * black_norm_cdf(-d1) : fc * black_norm_cdf(d1) - kp * black_norm_cdf(d2);
}

__global__ __launch_bounds__(BLOCK) void cmc_forward_kernel(CmcTable t, size_t n)
{
    __shared__ double lds[4 * 3];
    const CmcExpiry ex = t.expiries[blockIdx.y];
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    double v[3] = {0.0, 0.0, 0.0};
    for (size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x; i < n; i += stride) {
        double h, e;
        if (cmc_keep(ex.mu[i], ex.cv[i], h, e)) {
            const double d = e - 1.0;
            v[0] += d;
            v[1] = fma(d, d, v[1]);
            v[2] += 1.0;
        }
    }
    block_sum_store<3>(v, lds, t.fwd_partials + (static_cast<size_t>(blockIdx.x) * t.m + blockIdx.y) * 3, 3);
}

// its in-order finish, a block per expiry: the three column sums in row order, the forward statistics, and -- once per strike --
// K' = K + corr, ln K' and the shift of the strike's sums: the price of the expiry's path 0 (identical paths then leave sums
// that are exactly zero), or the intrinsic value at the forward where that path is dropped
__global__ __launch_bounds__(BLOCK) void cmc_forward_finish_kernel(CmcTable t, size_t n, int recenter)
{
    __shared__ double lds[4];
    __shared__ double s_corr;
    const int i = blockIdx.x;
    const CmcExpiry ex = t.expiries[i];
    const size_t ld = 3 * static_cast<size_t>(t.m);
    const double *base = t.fwd_partials + 3 * static_cast<size_t>(i);
    const double s0 = block_column_sum(base, t.rows, ld, lds);
    __syncthreads();
    const double s1 = block_column_sum(base + 1, t.rows, ld, lds);
    __syncthreads();
    const double cnt = block_column_sum(base + 2, t.rows, ld, lds);
    if (threadIdx.x == 0) {
        const double dmean = s0 / cnt;                     // 0 / 0 -> NaN like nanmean of an empty slice
        double var = s1 / cnt - dmean * dmean;
        if (var < 0.0) var = 0.0;
        const double fmean = fma(ex.forward, dmean, ex.forward);
        const double corr = recenter ? ex.forward * dmean : 0.0;       // mean_kept(F_c) - F
        double *f = t.fwd + 4 * i, *st = t.stats + SVMC_CMC_STATS_DOUBLES * i;
        f[0] = s0;
        f[1] = s1;
        f[2] = cnt;
        f[3] = corr;
        st[0] = fmean;
        st[1] = fabs(ex.forward) * sqrt(var) / sqrt(static_cast<double>(n));
        st[2] = corr;
        st[3] = cnt;
        st[4] = static_cast<double>(n) - cnt;
        s_corr = corr;
    }
    __syncthreads();
    const double corr = s_corr;
    double h, e;
    const double mu0 = ex.mu[0], cv0 = ex.cv[0];
    const bool keep0 = cmc_keep(mu0, cv0, h, e);
    const double fc = ex.forward * e, ln_fc = ex.ln_forward + h, sd = sqrt(cv0), inv_sd = 1.0 / sd;
    for (int k = ex.k0 + static_cast<int>(threadIdx.x); k < ex.k1; k += BLOCK) {
        const double kp = t.strikes[k] + corr;
        const double ln_kp = (kp > 0.0) ? log(kp) : 0.0;
        t.kp[k] = kp;
        t.ln_kp[k] = ln_kp;
        t.shift[k] = keep0 ? cmc_black(fc, ln_fc, cv0, sd, inv_sd, kp, ln_kp, t.is_put[k] != 0.0) : t.intrinsic[k];
    }
}

__global__ __launch_bounds__(BLOCK) void cmc_payoff_kernel(CmcTable t, size_t n)
{
    __shared__ double lds[4 * block_sum_padded(2 * CMC_KT)];
    const QuoteGroup g = t.groups[blockIdx.y];
    const CmcExpiry ex = t.expiries[g.expiry];
    double kp[CMC_KT], ln_kp[CMC_KT], shift[CMC_KT], acc[2 * CMC_KT];
    bool put[CMC_KT];
#pragma unroll
    for (int k = 0; k < CMC_KT; ++k) {
        const int kk = g.k0 + ((k < g.nk) ? k : 0);        // the unused strikes of a group repeat its first; their sums are dropped
        kp[k] = t.kp[kk];
        ln_kp[k] = t.ln_kp[kk];
        shift[k] = t.shift[kk];
        put[k] = t.is_put[kk] != 0.0;
        acc[k] = acc[CMC_KT + k] = 0.0;
    }
    const double forward = ex.forward, ln_forward = ex.ln_forward;
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    for (size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x; i < n; i += stride) {
        const double cv = ex.cv[i];
        double h, e;
        if (!cmc_keep(ex.mu[i], cv, h, e)) continue;
        const double fc = forward * e, ln_fc = ln_forward + h;
        const double sd = sqrt(cv), inv_sd = 1.0 / sd;
#pragma unroll
        for (int k = 0; k < CMC_KT; ++k) {
            const double d = cmc_black(fc, ln_fc, cv, sd, inv_sd, kp[k], ln_kp[k], put[k]) - shift[k];
            acc[k] += d;
            acc[CMC_KT + k] = fma(d, d, acc[CMC_KT + k]);
        }
    }
    double *out = t.pay_partials + (static_cast<size_t>(blockIdx.x) * t.K + g.k0) * 2;
    const int nk = g.nk;
    block_sum_apply<2 * CMC_KT>(acc, lds, 2 * CMC_KT, [&](int j, double s) {
        const int k = (j < CMC_KT) ? j : j - CMC_KT;
        if (k < nk) out[2 * k + ((j < CMC_KT) ? 0 : 1)] = s;
    });
}

// a block per quote: its two column sums in row order, then utils/mc_payoffs.py:85-88 on them (payoff_finalize_one): price =
// discfactor (shift + mean), error = discfactor x population deviation / sqrt(n_path)
__global__ __launch_bounds__(BLOCK) void cmc_finish_kernel(CmcTable t, size_t n)
{
    __shared__ double lds[4];
    const int k = blockIdx.x;
    int i = 0;
    while (i + 1 < t.m && k >= t.expiries[i].k1) ++i;      // (block-uniform; expiries without strikes are skipped over)
    const size_t ld = 2 * static_cast<size_t>(t.K);
    const double s = block_column_sum(t.pay_partials + 2 * static_cast<size_t>(k), t.rows, ld, lds);
    __syncthreads();
    const double s2 = block_column_sum(t.pay_partials + 2 * static_cast<size_t>(k) + 1, t.rows, ld, lds);
    if (threadIdx.x == 0) {
        double price, err;
        payoff_finalize_one(s, s2, t.fwd[4 * i + 2], t.shift[k], t.expiries[i].discfactor, static_cast<double>(n), &price, &err);
        t.out[k] = price;
        t.out[t.K + k] = err;
    }
}

// ---------------------------------------------------------------------------------------------------
// derivatives of the conditional estimator in F and K (include/svmc.h states the formulas)
// ---------------------------------------------------------------------------------------------------
// The kernels' names carry neither of the words the f11 and f12 metadata tests count kernels by.

// Per kept path and strike: delta_i = e B_f + c B_k, dual_delta_i = B_k, dual_gamma_i = phi(d2) / (K' sd), with d1 and d2 formed as
// cmc_black forms them.  Each side's B_f and B_k come from its own tail (put: B_f = -N(-d1), B_k = N(-d2)), as its price does.
// Every multiply-add is written out, so that the value does not depend on the call site's contraction: the shift is this
// function on path 0 and identical paths must give differences that are exactly zero.
__device__ __forceinline__ void cmc_derivs(double e, double c, double fc, double ln_fc, double cv, double sd, double inv_sd, double kp,
                                           double ln_kp, double inv_kp, bool put, double &delta, double &dual_delta, double &dual_gamma)
{
    double bf, bk, dg = 0.0;
    if (!(kp > 0.0)) {
        bf = put ? 0.0 : 1.0;
        bk = -bf;
    } else if (cv == 0.0) {
        const bool itm = put ? (fc < kp) : (fc > kp);      // strict: a tie has payoff 0 and indicator 0
        bf = itm ? (put ? -1.0 : 1.0) : 0.0;
        bk = -bf;
    } else {
        const double d1 = fma(ln_fc - ln_kp, inv_sd, 0.5 * sd), d2 = d1 - sd;
        bf = put ? -black_norm_cdf(-d1) : black_norm_cdf(d1);
        bk = put ? black_norm_cdf(-d2) : -black_norm_cdf(d2);
        dg = (exp_full((-0.5 * d2) * d2) * 0.39894228040143267794) * (inv_sd * inv_kp);
    }
    delta = fma(e, bf, c * bk);
    dual_delta = bk;
    dual_gamma = dg;
}

// the shift of a strike's sums: cmc_derivs on the expiry's path 0, or at (mu, cv) = (0, 0) where that path is dropped
struct CmcPath0 {
    double e, fc, ln_fc, cv, sd, inv_sd;
};
__device__ __forceinline__ CmcPath0 cmc_path0(const CmcExpiry &ex)
{
    double h, e;
    double cv = ex.cv[0];
    if (!cmc_keep(ex.mu[0], cv, h, e)) {
        h = 0.0;
        e = 1.0;
        cv = 0.0;
    }
    const double sd = sqrt(cv);
    return CmcPath0{e, ex.forward * e, ex.ln_forward + h, cv, sd, 1.0 / sd};
}

template <int KT>
__global__ __launch_bounds__(BLOCK) void cond_deriv_kernel(CmcTable t, CmcDerivTable dt, size_t n, int recenter)
{
    constexpr int NV = CMC_DQ * KT + 1;                    // the last value: the count of cv == 0 paths
    __shared__ double lds[4 * block_sum_padded(NV)];
    const QuoteGroup g = dt.groups[blockIdx.y];
    const CmcExpiry ex = t.expiries[g.expiry];
    const int nk = g.nk;                                   // (block-uniform; 0: the group only counts)
    const double *fw = t.fwd + 4 * g.expiry;
    const double c = recenter ? fw[0] / fw[2] : 0.0;       // mean_kept(e) - 1, the quotient cmc_forward_finish_kernel forms
    double kp[KT], ln_kp[KT], inv_kp[KT], sh[3][KT], acc[NV];
    bool put[KT];
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = 0.0;
    if (nk > 0) {
        const CmcPath0 p0 = cmc_path0(ex);
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            const int kk = g.k0 + ((k < nk) ? k : 0);      // the unused strikes of a group repeat its first; their sums are dropped
            kp[k] = t.kp[kk];
            ln_kp[k] = t.ln_kp[kk];
            inv_kp[k] = 1.0 / kp[k];
            put[k] = t.is_put[kk] != 0.0;
            cmc_derivs(p0.e, c, p0.fc, p0.ln_fc, p0.cv, p0.sd, p0.inv_sd, kp[k], ln_kp[k], inv_kp[k], put[k], sh[0][k], sh[1][k], sh[2][k]);
            if (blockIdx.x == 0 && threadIdx.x == 0 && k < nk) {
                dt.shift[3 * kk] = sh[0][k];
                dt.shift[3 * kk + 1] = sh[1][k];
                dt.shift[3 * kk + 2] = sh[2][k];
            }
        }
    }
    const double forward = ex.forward, ln_forward = ex.ln_forward;
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    for (size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x; i < n; i += stride) {
        const double cv = ex.cv[i];
        double h, e;
        if (!cmc_keep(ex.mu[i], cv, h, e)) continue;
        if (cv == 0.0) acc[NV - 1] += 1.0;
        if (nk > 0) {
            const double fc = forward * e, ln_fc = ln_forward + h;
            const double sd = sqrt(cv), inv_sd = 1.0 / sd;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                double v[3];
                cmc_derivs(e, c, fc, ln_fc, cv, sd, inv_sd, kp[k], ln_kp[k], inv_kp[k], put[k], v[0], v[1], v[2]);
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const double d = v[q] - sh[q][k];
                    acc[(2 * q) * KT + k] += d;
                    acc[(2 * q + 1) * KT + k] = fma(d, d, acc[(2 * q + 1) * KT + k]);
                }
            }
        }
    }
    double *out = dt.partials + (static_cast<size_t>(blockIdx.x) * t.K + g.k0) * CMC_DQ;
    double *zero = (g.pad != 0) ? dt.zero_partials + static_cast<size_t>(blockIdx.x) * t.m + g.expiry : nullptr;
    block_sum_apply<NV>(acc, lds, NV, [&](int j, double s) {
        if (j == NV - 1) {
            if (zero != nullptr) *zero = s;
        } else {
            const int q = j / KT, k = j - q * KT;
            if (k < nk) out[CMC_DQ * k + q] = s;
        }
    });
}

// a block per quote, then a block per expiry.  Quote k: its six column sums in row order, payoff_finalize_one on each pair (value =
// discfactor (shift + mean over the kept paths), error = discfactor x population deviation / sqrt(n_path)), gamma and its error
// from dual gamma by (K / F)^2.  Expiry i (block K + i): the column sum of its cv == 0 counts.
__global__ __launch_bounds__(BLOCK) void cond_deriv_finish_kernel(CmcTable t, CmcDerivTable dt, size_t n)
{
    __shared__ double lds[4];
    const int k = blockIdx.x;
    if (k >= t.K) {                                        // (block-uniform)
        const int i = k - t.K;
        const double z = block_column_sum(dt.zero_partials + i, t.rows, static_cast<size_t>(t.m), lds);
        if (threadIdx.x == 0) dt.zero[i] = z;
        return;
    }
    int i = 0;
    while (i + 1 < t.m && k >= t.expiries[i].k1) ++i;
    const size_t ld = CMC_DQ * static_cast<size_t>(t.K);
    const double *base = dt.partials + CMC_DQ * static_cast<size_t>(k);
    double s[CMC_DQ];
#pragma unroll
    for (int q = 0; q < CMC_DQ; ++q) {
        if (q > 0) __syncthreads();
        s[q] = block_column_sum(base + q, t.rows, ld, lds);
    }
    if (threadIdx.x == 0) {
        const double cnt = t.fwd[4 * i + 2], df = t.expiries[i].discfactor, nn = static_cast<double>(n);
        double v[3], err[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) payoff_finalize_one(s[2 * q], s[2 * q + 1], cnt, dt.shift[3 * k + q], df, nn, &v[q], &err[q]);
        const double r = t.strikes[k] / t.expiries[i].forward, r2 = r * r;
        const size_t K = static_cast<size_t>(t.K);
        dt.out[k] = v[0];
        dt.out[K + k] = err[0];
        dt.out[2 * K + k] = v[1];
        dt.out[3 * K + k] = err[1];
        dt.out[4 * K + k] = r2 * v[2];
        dt.out[5 * K + k] = r2 * err[2];
        dt.out[6 * K + k] = v[2];
        dt.out[7 * K + k] = err[2];
    }
}

// prices_host, stderrs_host [K], stats_host [m][SVMC_CMC_STATS_DOUBLES] (nullable); returns after the stream is synchronised.
// pinned (nullable): page-locked host memory of cmc_pinned_bytes_of(m, K, deriv) for the table's image and the results
// greeks_host (nullable) [SVMC_CMC_GREEKS_ROWS][K]: the derivative launches run after the payoff tail's, prices_host and stderrs_host
// are not read and stats_host is [m][SVMC_CMC_GREEKS_STATS_DOUBLES]
int cmc_tail(const char *fn, const double *const *mu_snapshots_host, const double *const *cv_snapshots_host, size_t n_path,
                    const double *forwards_host, const double *discfactors_host, int n_expiries, const double *strikes_host,
                    const int8_t *types_host, const size_t *strike_offsets_host, int recenter, double *prices_host, double *stderrs_host,
                    double *greeks_host, double *stats_host, void *workspace, size_t workspace_bytes, hipStream_t stream, void *pinned,
                    size_t pinned_bytes)
{
    const bool deriv = greeks_host != nullptr;
    SVMC_REQUIRE(mu_snapshots_host && cv_snapshots_host && discfactors_host && (deriv || (prices_host && stderrs_host)) && workspace,
                 std::string(fn) + ": null pointer");
    if (int rc = check_quotes(fn, n_path, forwards_host, nullptr, n_expiries, strikes_host, types_host, strike_offsets_host, 1u << 30, 1))
        return rc;                                         // (any discount factor is taken: a non-finite one gives non-finite prices)
    const int m = n_expiries;
    const size_t K = strike_offsets_host[m];
    for (int i = 0; i < m; ++i) SVMC_REQUIRE(mu_snapshots_host[i] && cv_snapshots_host[i], std::string(fn) + ": null snapshot");
    const int G = quote_groups(m, strike_offsets_host, CMC_KT, false), GD = deriv ? quote_groups(m, strike_offsets_host, CMC_DKT, true) : 0;
    CmcTable t;
    CmcDerivTable dt;
    Layout w{static_cast<unsigned char *>(workspace)};
    const size_t up_bytes = cmc_workspace(w, n_path, m, K, G, GD, t, dt);
    if (workspace_bytes < w.bytes())
        return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": workspace too small (svmc_cmc_payoff_workspace_bytes / svmc_cmc_greeks_workspace_bytes)");

    // the table's host image and the results' landing: in the caller's page-locked staging block where it gave one that holds both
    // (the fused drivers: an upload from and downloads into pageable memory go through the runtime's staging path, 16 us apiece)
    CmcImage im;
    Layout need{nullptr};
    cmc_pinned(need, m, K, G, GD, im);
    const bool staged = pinned != nullptr && pinned_bytes >= need.bytes();
    std::vector<unsigned char> pageable(staged ? 0 : need.bytes());
    Layout h{staged ? static_cast<unsigned char *>(pinned) : pageable.data()};
    const CmcResults res = cmc_pinned(h, m, K, G, GD, im);
    cmc_fill_image(im, mu_snapshots_host, cv_snapshots_host, forwards_host, discfactors_host, m, strikes_host, types_host, strike_offsets_host,
                   deriv);
    SVMC_HIP_TRY(hipMemcpyAsync(workspace, h.base, up_bytes, hipMemcpyHostToDevice, stream));

    hipLaunchKernelGGL(cmc_forward_kernel, dim3(t.rows, m), dim3(BLOCK), 0, stream, t, n_path);
    if (int rc = check_launch(fn)) return rc;
    hipLaunchKernelGGL(cmc_forward_finish_kernel, dim3(m), dim3(BLOCK), 0, stream, t, n_path, recenter ? 1 : 0);
    if (int rc = check_launch(fn)) return rc;
    if (K > 0) {
        hipLaunchKernelGGL(cmc_payoff_kernel, dim3(t.rows, G), dim3(BLOCK), 0, stream, t, n_path);
        if (int rc = check_launch(fn)) return rc;
        hipLaunchKernelGGL(cmc_finish_kernel, dim3(static_cast<unsigned>(K)), dim3(BLOCK), 0, stream, t, n_path);
        if (int rc = check_launch(fn)) return rc;
    }
    if (deriv) {
        // price and error are the payoff tail's own launches above (bit-equal to svmc_cmc_payoff_chain by construction); the
        // derivative kernels evaluate the two normal CDFs again
        hipLaunchKernelGGL(cond_deriv_kernel<CMC_DKT>, dim3(t.rows, GD), dim3(BLOCK), 0, stream, t, dt, n_path, recenter ? 1 : 0);
        if (int rc = check_launch(fn)) return rc;
        hipLaunchKernelGGL(cond_deriv_finish_kernel, dim3(static_cast<unsigned>(K) + m), dim3(BLOCK), 0, stream, t, dt, n_path);
        if (int rc = check_launch(fn)) return rc;
    }
    SVMC_HIP_TRY(hipMemcpyAsync(res.out, t.out, need.bytes() - up_bytes, hipMemcpyDeviceToHost, stream));     // (the results are one block)
    SVMC_HIP_TRY(hipStreamSynchronize(stream));            // the table's host image and the results' landing
    if (!deriv) {
        memcpy(prices_host, res.out, K * sizeof(double));
        memcpy(stderrs_host, res.out + K, K * sizeof(double));
        if (stats_host != nullptr) memcpy(stats_host, res.stats, static_cast<size_t>(SVMC_CMC_STATS_DOUBLES) * m * sizeof(double));
        return SVMC_OK;
    }
    memcpy(greeks_host, res.out, static_cast<size_t>(SVMC_CMC_GREEKS_ROWS) * K * sizeof(double));     // prices, errors, then deriv_out
    if (stats_host != nullptr) {
        for (int i = 0; i < m; ++i) {
            memcpy(stats_host + static_cast<size_t>(SVMC_CMC_GREEKS_STATS_DOUBLES) * i, res.stats + SVMC_CMC_STATS_DOUBLES * i,
                   SVMC_CMC_STATS_DOUBLES * sizeof(double));
            stats_host[static_cast<size_t>(SVMC_CMC_GREEKS_STATS_DOUBLES) * i + SVMC_CMC_STATS_DOUBLES] = res.zero[i];
        }
    }
    return SVMC_OK;
}

// ---------------------------------------------------------------------------------------------------
// parameter sensitivities of the conditional estimator on common random numbers (include/svmc.h states the
// estimator, the delta-method term of its error and the shift convention)
// ---------------------------------------------------------------------------------------------------
// The 2P bumped jobs (up_0, dn_0, up_1, ...) of a chain of m expiries and K quotes are laid out as ONE CmcTable of 2P m expiries and
// 2P K strikes, job-major: cmc_forward_kernel and cmc_forward_finish_kernel then form every job's forward statistics, K' and ln K'
// as they form a single job's -- the same statements, hence the same bits.  The kernels below put the job and pair axes on
// blockIdx.z (blockIdx.y in the finish), so the launch count does not grow with P.

// the job pass: per kept path of job blockIdx.z the dual delta B_k of cmc_derivs against the job's own K'
__global__ __launch_bounds__(BLOCK) void cond_sens_jobs_kernel(CmcTable t, CmcSensTable st, size_t n)
{
    __shared__ double lds[4 * block_sum_padded(SENS_KT)];
    const QuoteGroup g = st.groups[blockIdx.y];
    const int job = blockIdx.z, nk = g.nk;
    const CmcExpiry ex = t.expiries[job * st.m + g.expiry];
    const size_t kbase = static_cast<size_t>(job) * st.K + g.k0;
    double kp[SENS_KT], ln_kp[SENS_KT], acc[SENS_KT];
    bool put[SENS_KT];
#pragma unroll
    for (int k = 0; k < SENS_KT; ++k) {
        const size_t kk = kbase + ((k < nk) ? k : 0);      // the unused strikes of a group repeat its first; their sums are dropped
        kp[k] = t.kp[kk];
        ln_kp[k] = t.ln_kp[kk];
        put[k] = t.is_put[kk] != 0.0;
        acc[k] = 0.0;
    }
    const double forward = ex.forward, ln_forward = ex.ln_forward;
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    for (size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x; i < n; i += stride) {
        const double cv = ex.cv[i];
        double h, e;
        if (!cmc_keep(ex.mu[i], cv, h, e)) continue;
        const double fc = forward * e, ln_fc = ln_forward + h;
        const double sd = sqrt(cv), inv_sd = 1.0 / sd;
#pragma unroll
        for (int k = 0; k < SENS_KT; ++k) {
            double delta, bk, dg;
            cmc_derivs(e, 0.0, fc, ln_fc, cv, sd, inv_sd, kp[k], ln_kp[k], 0.0, put[k], delta, bk, dg);
            acc[k] += bk;
        }
    }
    double *out = st.q_partials + static_cast<size_t>(blockIdx.x) * (2 * static_cast<size_t>(st.P) * st.K) + kbase;
    block_sum_apply<SENS_KT>(acc, lds, SENS_KT, [&](int j, double s) {
        if (j < nk) out[j] = s;
    });
}

// what a group of the pair pass holds per strike: each job's K', ln K' and q (0 without recentring)
struct CmcSensStrikes {
    double kpu[SENS_KT], lku[SENS_KT], kpd[SENS_KT], lkd[SENS_KT], qu[SENS_KT], qd[SENS_KT];
    bool put[SENS_KT];
};

// d = B_up - B_dn and dt = d + F (q_up (e_up - 1) - q_dn (e_dn - 1)) of path i for the strikes of a group; false: not a kept pair.
// The shift is this function on path 0: the multiply-adds are written out so that identical paths give differences of exactly 0.
__device__ __forceinline__ bool cond_sens_path(const CmcExpiry &xu, const CmcExpiry &xd, size_t i, const CmcSensStrikes &s,
                                               double (&d)[SENS_KT], double (&dt)[SENS_KT])
{
    const double cvu = xu.cv[i], cvd = xd.cv[i];
    double hu, eu, hd, ed;
    const bool keep_u = cmc_keep(xu.mu[i], cvu, hu, eu), keep_d = cmc_keep(xd.mu[i], cvd, hd, ed);
    if (!(keep_u && keep_d)) return false;
    const double fcu = xu.forward * eu, lfu = xu.ln_forward + hu, sdu = sqrt(cvu), isu = 1.0 / sdu;
    const double fcd = xd.forward * ed, lfd = xd.ln_forward + hd, sdd = sqrt(cvd), isd = 1.0 / sdd;
    const double du = eu - 1.0, dd = ed - 1.0;
#pragma unroll
    for (int k = 0; k < SENS_KT; ++k) {
        const double bu = cmc_black(fcu, lfu, cvu, sdu, isu, s.kpu[k], s.lku[k], s.put[k]);
        const double bd = cmc_black(fcd, lfd, cvd, sdd, isd, s.kpd[k], s.lkd[k], s.put[k]);
        d[k] = bu - bd;
        dt[k] = fma(xu.forward, fma(s.qu[k], du, -(s.qd[k] * dd)), d[k]);
    }
    return true;
}

// the pair pass: path blocks x groups x pairs
__global__ __launch_bounds__(BLOCK) void cond_sens_pairs_kernel(CmcTable t, CmcSensTable st, size_t n, int recenter)
{
    constexpr int NV = 3 * SENS_KT + 1;                    // the last value: the kept pairs
    __shared__ double lds[4 * block_sum_padded(NV)];
    const QuoteGroup g = st.groups[blockIdx.y];
    const int p = blockIdx.z, nk = g.nk;
    const CmcExpiry xu = t.expiries[(2 * p) * st.m + g.expiry], xd = t.expiries[(2 * p + 1) * st.m + g.expiry];
    const size_t ku = static_cast<size_t>(2 * p) * st.K + g.k0, kd = ku + st.K;
    CmcSensStrikes s;
    double acc[NV], sh_d[SENS_KT], sh_t[SENS_KT];
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = 0.0;
#pragma unroll
    for (int k = 0; k < SENS_KT; ++k) {
        const int o = (k < nk) ? k : 0;
        s.kpu[k] = t.kp[ku + o];
        s.lku[k] = t.ln_kp[ku + o];
        s.kpd[k] = t.kp[kd + o];
        s.lkd[k] = t.ln_kp[kd + o];
        s.qu[k] = recenter ? st.q[ku + o] : 0.0;
        s.qd[k] = recenter ? st.q[kd + o] : 0.0;
        s.put[k] = t.is_put[ku + o] != 0.0;
    }
    if (!cond_sens_path(xu, xd, 0, s, sh_d, sh_t)) {
#pragma unroll
        for (int k = 0; k < SENS_KT; ++k) sh_d[k] = sh_t[k] = 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double *sh = st.pair_shift + 2 * (static_cast<size_t>(p) * st.K + g.k0);
#pragma unroll
        for (int k = 0; k < SENS_KT; ++k)
            if (k < nk) {
                sh[2 * k] = sh_d[k];
                sh[2 * k + 1] = sh_t[k];
            }
    }
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    for (size_t i = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x; i < n; i += stride) {
        double d[SENS_KT], dt[SENS_KT];
        if (!cond_sens_path(xu, xd, i, s, d, dt)) continue;
        acc[NV - 1] += 1.0;
#pragma unroll
        for (int k = 0; k < SENS_KT; ++k) {
            const double a = d[k] - sh_d[k], b = dt[k] - sh_t[k];
            acc[k] += a;
            acc[SENS_KT + k] += b;
            acc[2 * SENS_KT + k] = fma(b, b, acc[2 * SENS_KT + k]);
        }
    }
    double *out = st.pair_partials + ((static_cast<size_t>(blockIdx.x) * st.P + p) * st.K + g.k0) * SENS_PQ;
    block_sum_apply<NV>(acc, lds, NV, [&](int j, double v) {
        if (j == NV - 1) {
            for (int k = 0; k < nk; ++k) out[SENS_PQ * k + 3] = v;
        } else {
            const int q = j / SENS_KT, k = j - q * SENS_KT;
            if (k < nk) out[SENS_PQ * k + q] = v;
        }
    });
}

// a block per (quote, job) -- phase 0: q = the column sum of the job's dual deltas in row order over its kept count -- or per (quote,
// pair) -- phase 1: the four column sums in row order, then sens = DF (d0 + mean_pairs(d - d0)) / (2 h), its error DF x population
// deviation of dt over the pairs / sqrt(n_path) / (2 h) and the kept pairs; no kept pair: 0 / 0 = NaN and a count of 0
__global__ __launch_bounds__(BLOCK) void cond_sens_finish_kernel(CmcTable t, CmcSensTable st, size_t n, int phase)
{
    __shared__ double lds[4];
    const int k = blockIdx.x, z = blockIdx.y;
    int i = 0;
    while (i + 1 < st.m && k >= t.expiries[i].k1) ++i;     // (block-uniform; the first m expiries of the table are job 0's)
    const size_t col = static_cast<size_t>(z) * st.K + k;
    if (phase == 0) {                                      // (block-uniform)
        const double s = block_column_sum(st.q_partials + col, t.rows, 2 * static_cast<size_t>(st.P) * st.K, lds);
        if (threadIdx.x == 0) st.q[col] = s / t.fwd[4 * (z * st.m + i) + 2];
        return;
    }
    const size_t ld = SENS_PQ * static_cast<size_t>(st.P) * st.K;
    const double *base = st.pair_partials + SENS_PQ * col;
    double s[SENS_PQ];
#pragma unroll
    for (int q = 0; q < SENS_PQ; ++q) {
        if (q > 0) __syncthreads();
        s[q] = block_column_sum(base + q, t.rows, ld, lds);
    }
    if (threadIdx.x == 0) {
        const double cnt = s[3], df = t.expiries[i].discfactor, h2 = 2.0 * st.steps[z];
        const double mean_d = st.pair_shift[2 * col] + s[0] / cnt;
        const double mean_t = s[1] / cnt;
        double var = s[2] / cnt - mean_t * mean_t;
        if (var < 0.0) var = 0.0;
        double *out = st.out + static_cast<size_t>(z) * SVMC_CMC_SENS_ROWS * st.K + k;
        out[0] = df * mean_d / h2;
        out[st.K] = df * sqrt(var) / sqrt(static_cast<double>(n)) / h2;
        out[2 * static_cast<size_t>(st.K)] = cnt;
    }
}

// The sensitivity tail queued on `stream` (no synchronisation): the table's image is built in `image` (the head of cmc_sens_pinned's
// block; the caller keeps it until the stream has passed the upload), *results_dev gets the device address of the [P][3][K] results.
// The arguments are check_quotes'ed and check_steps'ed by the caller.
int cmc_sens_enqueue(const char *fn, const double *const *up_mu, const double *const *up_cv, const double *const *dn_mu,
                     const double *const *dn_cv, size_t n_path, const double *forwards_host, const double *discfactors_host, int n_expiries,
                     const double *strikes_host, const int8_t *types_host, const size_t *strike_offsets_host, int n_params,
                     const double *steps_host, int recenter, void *image, void *workspace, size_t workspace_bytes, hipStream_t stream,
                     double **results_dev)
{
    SVMC_REQUIRE(up_mu && up_cv && dn_mu && dn_cv && image && workspace && results_dev, std::string(fn) + ": null pointer");
    const int m = n_expiries, P = n_params, J = 2 * P;
    const size_t K = strike_offsets_host[m];
    for (int r = 0; r < P * m; ++r)
        SVMC_REQUIRE(up_mu[r] && up_cv[r] && dn_mu[r] && dn_cv[r], std::string(fn) + ": null snapshot");
    const int G = quote_groups(m, strike_offsets_host, SENS_KT, false);
    CmcTable t;
    CmcSensTable st;
    Layout w{static_cast<unsigned char *>(workspace)}, h{static_cast<unsigned char *>(image)};
    const size_t image_bytes = cmc_sens_workspace(w, n_path, m, K, G, P, t, st);
    if (workspace_bytes < w.bytes())
        return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": workspace too small (svmc_cmc_sens_workspace_bytes)");
    cmc_sens_fill_image(cmc_sens_image(h, m, K, G, P), up_mu, up_cv, dn_mu, dn_cv, forwards_host, discfactors_host, m, strikes_host,
                        types_host, strike_offsets_host, P, steps_host);
    SVMC_HIP_TRY(hipMemcpyAsync(workspace, image, image_bytes, hipMemcpyHostToDevice, stream));
    *results_dev = st.out;

    hipLaunchKernelGGL(cmc_forward_kernel, dim3(t.rows, static_cast<unsigned>(t.m)), dim3(BLOCK), 0, stream, t, n_path);
    if (int rc = check_launch(fn)) return rc;
    hipLaunchKernelGGL(cmc_forward_finish_kernel, dim3(static_cast<unsigned>(t.m)), dim3(BLOCK), 0, stream, t, n_path, recenter ? 1 : 0);
    if (int rc = check_launch(fn)) return rc;
    if (K == 0) return SVMC_OK;
    const unsigned uG = static_cast<unsigned>(G), uK = static_cast<unsigned>(K);
    if (recenter) {                                        // (without recentring q is not read)
        hipLaunchKernelGGL(cond_sens_jobs_kernel, dim3(t.rows, uG, static_cast<unsigned>(J)), dim3(BLOCK), 0, stream, t, st, n_path);
        if (int rc = check_launch(fn)) return rc;
        hipLaunchKernelGGL(cond_sens_finish_kernel, dim3(uK, static_cast<unsigned>(J)), dim3(BLOCK), 0, stream, t, st, n_path, 0);
        if (int rc = check_launch(fn)) return rc;
    }
    hipLaunchKernelGGL(cond_sens_pairs_kernel, dim3(t.rows, uG, static_cast<unsigned>(P)), dim3(BLOCK), 0, stream, t, st, n_path, recenter ? 1 : 0);
    if (int rc = check_launch(fn)) return rc;
    hipLaunchKernelGGL(cond_sens_finish_kernel, dim3(uK, static_cast<unsigned>(P)), dim3(BLOCK), 0, stream, t, st, n_path, 1);
    return check_launch(fn);
}

// ---------------------------------------------------------------------------------------------------
// the conditional calibration objective: P parameter sets of one chain in one tail (include/svmc.h)
// ---------------------------------------------------------------------------------------------------
// The P sets are laid out as ONE CmcTable of P m expiries and P K strikes, set-major, as the sensitivity tail lays out its bumped
// jobs: cmc_forward_kernel, cmc_forward_finish_kernel and cmc_payoff_kernel serve every set with a single call's statements.  The two
// kernels below end the tail; their names carry none of the words the earlier rows' metadata tests count kernels by.

// cmc_finish_kernel with the results' landing in page-locked host memory (no copy node): block (k, q) with k < K is quote k of set q
// -- its two column sums in row order, payoff_finalize_one on them, price and error stored at st.prices / st.stderrs and the price
// kept on the device for the inversion; block (K + i, q) stores the statistics of expiry i of set q.
__global__ __launch_bounds__(BLOCK) void cond_vols_finish_kernel(CmcTable t, CmcSetsTable st, size_t n)
{
    __shared__ double lds[4];
    const int q = blockIdx.y;
    if (static_cast<int>(blockIdx.x) >= st.K) {            // (block-uniform)
        const size_t e = static_cast<size_t>(q) * st.m + (blockIdx.x - st.K);
        if (threadIdx.x < SVMC_CMC_STATS_DOUBLES)
            st.stats[SVMC_CMC_STATS_DOUBLES * e + threadIdx.x] = t.stats[SVMC_CMC_STATS_DOUBLES * e + threadIdx.x];
        return;
    }
    const int k = q * st.K + static_cast<int>(blockIdx.x);
    int i = q * st.m;
    while (i + 1 < (q + 1) * st.m && k >= t.expiries[i].k1) ++i;      // (block-uniform; expiries without strikes are skipped over)
    const size_t ld = 2 * static_cast<size_t>(t.K);
    const double s = block_column_sum(t.pay_partials + 2 * static_cast<size_t>(k), t.rows, ld, lds);
    __syncthreads();
    const double s2 = block_column_sum(t.pay_partials + 2 * static_cast<size_t>(k) + 1, t.rows, ld, lds);
    if (threadIdx.x == 0) {
        double price, err;
        payoff_finalize_one(s, s2, t.fwd[4 * i + 2], t.shift[k], t.expiries[i].discfactor, static_cast<double>(n), &price, &err);
        t.out[k] = price;
        st.prices[k] = price;
        st.stderrs[k] = err;
    }
}

// the Black-76 implied vols of the table's quotes, a lane per quote and 64 quotes side by side in a wave (chain_implied_vols_kernel's
// shape: one lane of a wave per quote behind the finish's blocks measured slower there), stored at st.ivols
__global__ __launch_bounds__(64) void cond_vols_invert_kernel(CmcTable t, CmcSetsTable st, double vol_lo, double vol_hi)
{
    const int k = static_cast<int>(blockIdx.x) * 64 + static_cast<int>(threadIdx.x);
    if (k >= t.K) return;
    const double *qc = st.quote_consts + static_cast<size_t>(SETS_QC) * k;
    st.ivols[k] = black_implied_vol(t.out[k], t.strikes[k], t.is_put[k] == 0.0, qc[0], qc[1], qc[2], vol_lo, vol_hi);
}

size_t cmc_sets_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, int n_sets)
{
    return cmc_sets_workspace_bytes_of(n_path, n_expiries, total_strikes, n_sets);
}
size_t cmc_sets_pinned_bytes(int n_expiries, size_t total_strikes, int n_sets)
{
    CmcSetsTable st;
    return cmc_sets_pinned(nullptr, n_expiries, total_strikes, n_sets, true, st);
}

// the table and its landing from the walks of svmc_quotes.h; G: the table's group count
static int cmc_sets_tables(const char *fn, size_t n_path, int m, const size_t *offsets, int P, void *workspace, size_t workspace_bytes,
                           void *pinned, bool want_ivols, CmcTable &t, CmcSetsTable &st, int &G, size_t &image_bytes)
{
    SVMC_REQUIRE(offsets && workspace && pinned, std::string(fn) + ": null pointer");
    const size_t K = offsets[m];
    std::vector<size_t> table_offsets(static_cast<size_t>(P) * m + 1);
    cmc_sets_offsets(m, offsets, P, table_offsets.data());
    G = quote_groups(P * m, table_offsets.data(), CMC_KT, false);
    Layout w{static_cast<unsigned char *>(workspace)};
    image_bytes = cmc_sets_workspace(w, n_path, m, K, G, P, t, st);
    if (workspace_bytes < w.bytes()) return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": workspace too small");
    cmc_sets_pinned(pinned, m, K, P, want_ivols, st);
    return SVMC_OK;
}

// The table's image -- set q's expiry i reads rows q m + i of mu_snapshots / cv_snapshots ([n_sets][m][n_path]) -- uploaded to the
// head of `workspace`; returns after the stream is synchronised.  It depends on the chain and the buffers alone: once per capture.
int cmc_sets_upload(const char *fn, const double *mu_snapshots, const double *cv_snapshots, size_t n_path, const double *ttms_host,
                    const double *forwards_host, const double *discfactors_host, int n_expiries, const double *strikes_host,
                    const int8_t *types_host, const size_t *strike_offsets_host, int n_sets, void *workspace, size_t workspace_bytes,
                    void *pinned, hipStream_t stream)
{
    SVMC_REQUIRE(mu_snapshots && cv_snapshots && ttms_host && discfactors_host, std::string(fn) + ": null pointer");
    const int m = n_expiries, P = n_sets;
    CmcTable t;
    CmcSetsTable st;
    int G;
    size_t image_bytes;
    if (int rc = cmc_sets_tables(fn, n_path, m, strike_offsets_host, P, workspace, workspace_bytes, pinned, true, t, st, G, image_bytes)) return rc;
    std::vector<const double *> mus(static_cast<size_t>(P) * m), cvs(mus.size());
    for (size_t r = 0; r < mus.size(); ++r) {
        mus[r] = mu_snapshots + r * n_path;
        cvs[r] = cv_snapshots + r * n_path;
    }
    std::vector<size_t> table_offsets(mus.size() + 1);
    cmc_sets_offsets(m, strike_offsets_host, P, table_offsets.data());
    std::vector<unsigned char> image(image_bytes);
    Layout h{image.data()};
    cmc_sets_fill_image(cmc_sets_image(h, m, strike_offsets_host[m], G, P), mus.data(), cvs.data(), ttms_host, forwards_host, discfactors_host, m,
                        strikes_host, types_host, strike_offsets_host, P, table_offsets.data());
    SVMC_HIP_TRY(hipMemcpyAsync(workspace, image.data(), image_bytes, hipMemcpyHostToDevice, stream));
    SVMC_HIP_TRY(hipStreamSynchronize(stream));
    return SVMC_OK;
}

// The tail of every set queued on `stream` (no upload, no copy, no synchronisation: what a graph captures): the three kernels of a
// single call on the table cmc_sets_upload left, then the finish and, with want_ivols, the inversion on [vol_lo, vol_hi].  The
// results land in `pinned` as cmc_sets_results finds them.
int cmc_sets_enqueue(const char *fn, size_t n_path, int n_expiries, const size_t *strike_offsets_host, int n_sets, int recenter,
                     bool want_ivols, double vol_lo, double vol_hi, void *workspace, size_t workspace_bytes, void *pinned, hipStream_t stream)
{
    const int m = n_expiries, P = n_sets;
    CmcTable t;
    CmcSetsTable st;
    int G;
    size_t image_bytes;
    if (int rc = cmc_sets_tables(fn, n_path, m, strike_offsets_host, P, workspace, workspace_bytes, pinned, want_ivols, t, st, G, image_bytes))
        return rc;
    hipLaunchKernelGGL(cmc_forward_kernel, dim3(t.rows, static_cast<unsigned>(t.m)), dim3(BLOCK), 0, stream, t, n_path);
    if (int rc = check_launch(fn)) return rc;
    hipLaunchKernelGGL(cmc_forward_finish_kernel, dim3(static_cast<unsigned>(t.m)), dim3(BLOCK), 0, stream, t, n_path, recenter ? 1 : 0);
    if (int rc = check_launch(fn)) return rc;
    if (t.K > 0) {
        hipLaunchKernelGGL(cmc_payoff_kernel, dim3(t.rows, static_cast<unsigned>(G)), dim3(BLOCK), 0, stream, t, n_path);
        if (int rc = check_launch(fn)) return rc;
    }
    hipLaunchKernelGGL(cond_vols_finish_kernel, dim3(static_cast<unsigned>(st.K + st.m), static_cast<unsigned>(P)), dim3(BLOCK), 0, stream, t,
                       st, n_path);
    if (int rc = check_launch(fn)) return rc;
    if (want_ivols && t.K > 0) {
        hipLaunchKernelGGL(cond_vols_invert_kernel, dim3(static_cast<unsigned>((t.K + 63) / 64)), dim3(64), 0, stream, t, st, vol_lo, vol_hi);
        if (int rc = check_launch(fn)) return rc;
    }
    return SVMC_OK;
}

void cmc_sets_results(void *pinned, int n_expiries, size_t total_strikes, int n_sets, const double **prices, const double **stderrs,
                      const double **stats, const double **ivols)
{
    CmcSetsTable st;
    cmc_sets_pinned(pinned, n_expiries, total_strikes, n_sets, true, st);
    *prices = st.prices;
    *stderrs = st.stderrs;
    *stats = st.stats;
    *ivols = st.ivols;
}

}  // namespace svmc

using namespace svmc;

extern "C" {

int svmc_logsv_chain_cmc(double *mu, double *cv, double *sigma, double *qvar, size_t n_path, int n_slices, const int *nb_steps_host,
                         const double *dts_host, const double *etas_host, double theta, double kappa1, double kappa2, double beta,
                         double volvol, int is_spot_measure, uint64_t seed, uint32_t call_id, uint64_t path_offset, uint32_t step_offset,
                         double *mu_snapshots, double *cv_snapshots, double *qvar_snapshots, svmc_stream_t stream)
{
    return logsv_cmc_step_chain("svmc_logsv_chain_cmc", CmcInit(), mu, cv, sigma, qvar, n_path, n_slices, nb_steps_host, dts_host, etas_host,
                                theta, kappa1, kappa2, beta, volvol, is_spot_measure, seed, call_id, path_offset, step_offset, mu_snapshots,
                                cv_snapshots, qvar_snapshots, as_stream(stream));
}

int svmc_heston_chain_cmc(double *mu, double *cv, double *var, double *qvar, size_t n_path, int n_slices, const int *nb_steps_host,
                          const double *dts_host, double theta, double kappa, double rho, double volvol, uint64_t seed, uint32_t call_id,
                          uint64_t path_offset, uint32_t step_offset, double *mu_snapshots, double *cv_snapshots, double *qvar_snapshots,
                          svmc_stream_t stream)
{
    return heston_cmc_step_chain("svmc_heston_chain_cmc", CmcInit(), mu, cv, var, qvar, n_path, n_slices, nb_steps_host, dts_host, theta,
                                 kappa, rho, volvol, seed, call_id, path_offset, step_offset, mu_snapshots, cv_snapshots, qvar_snapshots,
                                 as_stream(stream));
}

int svmc_cmc_payoff_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, size_t *bytes)
{
    SVMC_REQUIRE(bytes != nullptr && n_expiries >= 1, "svmc_cmc_payoff_workspace_bytes: null output or no expiries");
    *bytes = cmc_workspace_bytes_of(n_path, n_expiries, total_strikes, false);
    return SVMC_OK;
}

int svmc_cmc_payoff_chain(const double *const *mu_snapshots_host, const double *const *cv_snapshots_host, size_t n_path,
                          const double *forwards_host, const double *discfactors_host, int n_expiries, const double *strikes_host,
                          const int8_t *types_host, const size_t *strike_offsets_host, int recenter, double *prices_host,
                          double *stderrs_host, double *stats_host, void *workspace, size_t workspace_bytes, svmc_stream_t stream)
{
    return cmc_tail("svmc_cmc_payoff_chain", mu_snapshots_host, cv_snapshots_host, n_path, forwards_host, discfactors_host, n_expiries,
                    strikes_host, types_host, strike_offsets_host, recenter, prices_host, stderrs_host, nullptr, stats_host, workspace,
                    workspace_bytes, as_stream(stream), nullptr, 0);
}

int svmc_cmc_greeks_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, size_t *bytes)
{
    SVMC_REQUIRE(bytes != nullptr && n_expiries >= 1, "svmc_cmc_greeks_workspace_bytes: null output or no expiries");
    *bytes = cmc_workspace_bytes_of(n_path, n_expiries, total_strikes, true);
    return SVMC_OK;
}

int svmc_cmc_greeks_chain(const double *const *mu_snapshots_host, const double *const *cv_snapshots_host, size_t n_path,
                          const double *forwards_host, const double *discfactors_host, int n_expiries, const double *strikes_host,
                          const int8_t *types_host, const size_t *strike_offsets_host, int recenter, double *greeks_host,
                          double *stats_host, void *workspace, size_t workspace_bytes, svmc_stream_t stream)
{
    SVMC_REQUIRE(greeks_host != nullptr, "svmc_cmc_greeks_chain: null pointer");
    return cmc_tail("svmc_cmc_greeks_chain", mu_snapshots_host, cv_snapshots_host, n_path, forwards_host, discfactors_host, n_expiries,
                    strikes_host, types_host, strike_offsets_host, recenter, nullptr, nullptr, greeks_host, stats_host, workspace,
                    workspace_bytes, as_stream(stream), nullptr, 0);
}

int svmc_cmc_many_workspace_bytes(int n_jobs, int n_slices, size_t *bytes)
{
    SVMC_REQUIRE(bytes != nullptr && n_jobs >= 1 && n_jobs <= SVMC_MANY_MAX_JOBS && n_slices >= 1 && n_slices <= MAX_CHAIN_SLICES,
                 "svmc_cmc_many_workspace_bytes: null output, n_jobs outside [1, SVMC_MANY_MAX_JOBS] or n_slices outside [1, 16]");
    *bytes = cmc_many_table_bytes(n_jobs, n_slices);
    return SVMC_OK;
}

// (the job table is built in pageable memory here: the call returns after the stream is synchronised)
int svmc_logsv_chain_cmc_many(size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
                              const double *params_host, int is_spot_measure, const uint64_t *seeds_host, const uint32_t *call_ids_host,
                              uint64_t path_offset, double *mu_snapshots, double *cv_snapshots, void *workspace, size_t workspace_bytes,
                              svmc_stream_t stream)
{
    const char *fn = "svmc_logsv_chain_cmc_many";
    SVMC_REQUIRE(n_jobs >= 1 && n_jobs <= SVMC_MANY_MAX_JOBS && n_slices >= 1 && n_slices <= MAX_CHAIN_SLICES,
                 std::string(fn) + ": n_jobs outside [1, SVMC_MANY_MAX_JOBS] or n_slices outside [1, 16]");
    if (workspace == nullptr || workspace_bytes < cmc_many_table_bytes(n_jobs, n_slices))
        return fail(workspace ? SVMC_ERR_WORKSPACE : SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": workspace null or too small (svmc_cmc_many_workspace_bytes)");
    std::vector<unsigned char> table(cmc_many_table_bytes(n_jobs, n_slices));
    if (int rc = logsv_cmc_step_many(fn, n_path, n_jobs, n_slices, nb_steps_host, dts_host, params_host, is_spot_measure, seeds_host,
                                     call_ids_host, path_offset, table.data(), workspace, mu_snapshots, cv_snapshots, as_stream(stream)))
        return rc;
    SVMC_HIP_TRY(hipStreamSynchronize(as_stream(stream)));
    return SVMC_OK;
}

int svmc_heston_chain_cmc_many(size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
                               const double *params_host, const uint64_t *seeds_host, const uint32_t *call_ids_host, uint64_t path_offset,
                               double *mu_snapshots, double *cv_snapshots, void *workspace, size_t workspace_bytes, svmc_stream_t stream)
{
    const char *fn = "svmc_heston_chain_cmc_many";
    SVMC_REQUIRE(n_jobs >= 1 && n_jobs <= SVMC_MANY_MAX_JOBS && n_slices >= 1 && n_slices <= MAX_CHAIN_SLICES,
                 std::string(fn) + ": n_jobs outside [1, SVMC_MANY_MAX_JOBS] or n_slices outside [1, 16]");
    if (workspace == nullptr || workspace_bytes < cmc_many_table_bytes(n_jobs, n_slices))
        return fail(workspace ? SVMC_ERR_WORKSPACE : SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": workspace null or too small (svmc_cmc_many_workspace_bytes)");
    std::vector<unsigned char> table(cmc_many_table_bytes(n_jobs, n_slices));
    if (int rc = heston_cmc_step_many(fn, n_path, n_jobs, n_slices, nb_steps_host, dts_host, params_host, seeds_host, call_ids_host,
                                      path_offset, table.data(), workspace, mu_snapshots, cv_snapshots, as_stream(stream)))
        return rc;
    SVMC_HIP_TRY(hipStreamSynchronize(as_stream(stream)));
    return SVMC_OK;
}

int svmc_cmc_sens_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, int n_params, size_t *bytes)
{
    SVMC_REQUIRE(bytes != nullptr && n_expiries >= 1 && n_params >= 1 && n_params <= SVMC_GREEKS_MAX_PARAMS,
                 "svmc_cmc_sens_workspace_bytes: null output, no expiries or n_params outside [1, SVMC_GREEKS_MAX_PARAMS]");
    *bytes = cmc_sens_workspace_bytes_of(n_path, n_expiries, total_strikes, n_params);
    return SVMC_OK;
}

int svmc_cmc_sens_chain(const double *const *up_mu_host, const double *const *up_cv_host, const double *const *dn_mu_host,
                        const double *const *dn_cv_host, size_t n_path, const double *forwards_host, const double *discfactors_host,
                        int n_expiries, const double *strikes_host, const int8_t *types_host, const size_t *strike_offsets_host,
                        int n_params, const double *steps_host, int recenter, double *sens_host, void *workspace, size_t workspace_bytes,
                        svmc_stream_t stream)
{
    const char *fn = "svmc_cmc_sens_chain";
    SVMC_REQUIRE(sens_host && discfactors_host && steps_host, std::string(fn) + ": null pointer");
    if (int rc = check_steps(fn, n_params, steps_host, 1)) return rc;
    if (int rc = check_quotes(fn, n_path, forwards_host, discfactors_host, n_expiries, strikes_host, types_host, strike_offsets_host, 1u << 30,
                              2 * static_cast<size_t>(n_params)))
        return rc;
    const size_t K = strike_offsets_host[n_expiries];
    std::vector<unsigned char> image(cmc_sens_pinned(nullptr, n_expiries, K, n_params, nullptr));
    double *res = nullptr;
    if (int rc = cmc_sens_enqueue(fn, up_mu_host, up_cv_host, dn_mu_host, dn_cv_host, n_path, forwards_host, discfactors_host, n_expiries,
                                  strikes_host, types_host, strike_offsets_host, n_params, steps_host, recenter, image.data(), workspace,
                                  workspace_bytes, as_stream(stream), &res))
        return rc;
    if (K > 0)
        SVMC_HIP_TRY(hipMemcpyAsync(sens_host, res, static_cast<size_t>(SVMC_CMC_SENS_ROWS) * n_params * K * sizeof(double),
                                    hipMemcpyDeviceToHost, as_stream(stream)));
    SVMC_HIP_TRY(hipStreamSynchronize(as_stream(stream)));     // the table's host image and the results' landing
    return SVMC_OK;
}

}  // extern "C"
