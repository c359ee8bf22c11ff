// svmc_greeks.hip -- Monte Carlo chain Greeks on common random numbers (include/svmc.h states the estimators,
// the keep rule and the errors).
//
// The payoff tail of svmc_logsv_chain_price_greeks / svmc_heston_chain_price_greeks and, on any device arrays, of
// svmc_greeks_payoff_chain: the base job's rows give the pathwise forward delta and the dual delta; the P pairs of bumped jobs,
// stepped on the base job's random stream, give per path the difference of the two bumped payoffs, whose mean is the central
// difference of the prices and whose deviation is the error of that difference -- orders below the two prices' own errors.
//
//   greeks_payoff_kernel<KT>   a block = a path block x a group of up to KT strikes of one expiry x a slot (blockIdx.z).
//                              JOB PASS: a slot is one of the 1 + 2P jobs; per strike the sums of g - shift, its square and the
//                              in-the-money count (the base job's give the two deltas, every job's count its in-the-money
//                              fraction q).  PAIR PASS: a slot is a bump pair, reading the up and the dn row of the expiry; per
//                              strike the sums of d, dt and dt^2, per path the pair count; dt = d - s (q_up (spot_up - F) -
//                              q_dn (spot_dn - F)) carries the delta-method term of the two recentring means.
//                              payoff_group_kernel's trips: the ones every lane of the block makes go through the batched double
//                              buffer, the ragged last one on its own.  One partial row per block, no atomics.
//   greeks_finish_kernel       a block per (slot, quote): the column sums in row order, then the values and errors, stored
//                              where the host reads them (job pass: also q of every job and quote, on the device).
// Four launches: the job pass and its finish, then the pair pass and its finish.
#include "svmc_internal.h"

#include <cmath>
#include <cstring>
#include <vector>

#include "svmc_block.h"
#include "svmc_math.h"
#include "svmc_quotes.h"

namespace svmc {

static_assert(QUOTE_BLOCK == BLOCK, "svmc_quotes.h sizes the partial rows for blocks of BLOCK paths");
constexpr int GREEKS_PREFETCH = 2;             // trips between a path's load and its use

// the kept-path mean of exp(x) of a job's expiry, from its reduced spot sums [sum F exp(x), count]
__device__ __forceinline__ double greeks_mean_exp(const double *__restrict__ spot_sums, double forward)
{
    return (spot_sums[0] / spot_sums[1]) / forward;
}

constexpr int greeks_min_waves(int kt) { return kt <= 8 ? 3 : 2; }

template <int KT>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(greeks_min_waves(KT), greeks_min_waves(KT)))) void greeks_payoff_kernel(
    GreeksTable t, size_t n, int pair_pass)
{
    constexpr int NSUM = block_sum_padded(3 * KT + 1);
    __shared__ double lds[4 * NSUM];
    const QuoteGroup g = t.groups[blockIdx.y];
    const GreeksExpiry ex = t.expiries[g.expiry];
    const int z = blockIdx.z, m = t.m;                      // job pass: the job; pair pass: the parameter (block-uniform)
    const double forward = ex.forward;
    double sg[KT], c[KT], shift[KT], shift_dn[KT], acc[NSUM];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        const int kk = g.k0 + ((k < g.nk) ? k : 0);         // the unused strikes of a group repeat its first; their sums are dropped
        sg[k] = t.sg[kk];
        c[k] = t.c[kk];
        shift[k] = t.gshift[kk];
    }
#pragma unroll
    for (int j = 0; j < NSUM; ++j) acc[j] = 0.0;
    const size_t stride = static_cast<size_t>(gridDim.x) * BLOCK;
    const size_t i0 = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x;
    const size_t block_last = static_cast<size_t>(blockIdx.x) * BLOCK + (BLOCK - 1);
    const int full_trips = (n > block_last) ? static_cast<int>((n - 1 - block_last) / stride + 1) : 0;     // block-uniform
    if (!pair_pass) {
        const double *__restrict__ x = t.rows[z * m + g.expiry];
        const double mean = greeks_mean_exp(t.spot_sums + 2 * (z * m + g.expiry), forward);
        // g = sg e 1{sg (spot - K) > 0}, e = exp(x) - M + 1, spot = F e: a NaN spot is out of the money and adds g = 0
        const auto add_path = [&](double xi) {
            const double e = (exp_full(xi) - mean) + 1.0;
            const double spot = forward * e;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const bool itm = fma(sg[k], spot, c[k]) > 0.0;               // the sign of sg (spot - K), exact: strict
                const double gg = (itm ? sg[k] * e : 0.0) - shift[k];
                acc[k] += gg;
                acc[KT + k] = fma(gg, gg, acc[KT + k]);
                acc[2 * KT + k] += itm ? 1.0 : 0.0;
            }
        };
        const double *const w[1] = {x + i0};
        streamed_time_loop<1, GREEKS_PREFETCH>(w, stride, full_trips, [&](const double(&v)[1]) { add_path(v[0]); });
        for (size_t i = i0 + static_cast<size_t>(full_trips) * stride; i < n; i += stride) add_path(x[i]);
    } else {
        const int up = 2 * z + 1, dn = 2 * z + 2;
        const double *__restrict__ xu = t.rows[up * m + g.expiry];
        const double *__restrict__ xd = t.rows[dn * m + g.expiry];
        const double mean_u = greeks_mean_exp(t.spot_sums + 2 * (up * m + g.expiry), forward);
        const double mean_d = greeks_mean_exp(t.spot_sums + 2 * (dn * m + g.expiry), forward);
        // the delta-method coefficients of the two recentring means: s q of the up and of the dn job's quote
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            const int kk = g.k0 + ((k < g.nk) ? k : 0);
            shift[k] = sg[k] * t.itm_fraction[static_cast<size_t>(up) * t.K + kk];
            shift_dn[k] = sg[k] * t.itm_fraction[static_cast<size_t>(dn) * t.K + kk];
        }
        // d = pay(x_up) - pay(x_dn), each job recentred by its own mean; a pair is kept iff neither payoff is NaN, that is iff
        // neither spot is; dt = d - s (q_up (spot_up - F) - q_dn (spot_dn - F))
        const auto add_pair = [&](double xui, double xdi) {
            const double su = forward * ((exp_full(xui) - mean_u) + 1.0);
            const double sd = forward * ((exp_full(xdi) - mean_d) + 1.0);
            const bool keep = su == su && sd == sd;
            const double au = su - forward, ad = sd - forward;
            acc[3 * KT] += keep ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const double pu = fmax(fma(sg[k], su, c[k]), 0.0), pd = fmax(fma(sg[k], sd, c[k]), 0.0);
                const double d = keep ? pu - pd : 0.0;
                const double dt = keep ? (pu - pd) - (shift[k] * au - shift_dn[k] * ad) : 0.0;
                acc[k] += d;
                acc[KT + k] += dt;
                acc[2 * KT + k] = fma(dt, dt, acc[2 * KT + k]);
            }
        };
        const double *const w[2] = {xu + i0, xd + i0};
        streamed_time_loop<2, GREEKS_PREFETCH>(w, stride, full_trips, [&](const double(&v)[2]) { add_pair(v[0], v[1]); });
        for (size_t i = i0 + static_cast<size_t>(full_trips) * stride; i < n; i += stride) add_pair(xu[i], xd[i]);
    }
    // partial row layout: GREEKS_COLS columns per strike, interleaved, at partials[path block][slot][strike]; the pair count
    // of a block, one per path, is stored with every strike of the group
    double *row = t.partials + ((static_cast<size_t>(blockIdx.x) * gridDim.z + z) * t.K + g.k0) * GREEKS_COLS;
    const int nk = g.nk;
    block_sum_apply<NSUM>(acc, lds, 3 * KT + 1, [&](int j, double s) {
        if (j == 3 * KT) {
            for (int k = 0; k < nk; ++k) row[GREEKS_COLS * k + 3] = s;
            return;
        }
        const int which = j / KT, k = j - which * KT;
        if (k < nk) row[GREEKS_COLS * k + which] = s;
    });
}

// a block per (slot, quote): its column sums in row order, then include/svmc.h's values and errors
__global__ __launch_bounds__(BLOCK) void greeks_finish_kernel(GreeksTable t, size_t n, int pair_pass, int slots)
{
    __shared__ double lds[4];
    const int z = static_cast<int>(blockIdx.x) / t.K, k = static_cast<int>(blockIdx.x) % t.K;
    int i = 0;
    while (i + 1 < t.m && k >= t.expiries[i].k1) ++i;      // (block-uniform; expiries without strikes are skipped over)
    const size_t ld = GREEKS_COLS * static_cast<size_t>(t.K) * static_cast<size_t>(slots);
    const double *base = t.partials + GREEKS_COLS * (static_cast<size_t>(z) * t.K + k);
    const double df = t.expiries[i].discfactor, nn = static_cast<double>(n);
    const size_t K = static_cast<size_t>(t.K);
    if (!pair_pass) {
        const double itm = block_column_sum(base + 2, t.n_rows, ld, lds);
        double s = 0.0, s2 = 0.0;
        if (z == 0) {                                      // (block-uniform) the base job: the two deltas
            __syncthreads();
            s = block_column_sum(base, t.n_rows, ld, lds);
            __syncthreads();
            s2 = block_column_sum(base + 1, t.n_rows, ld, lds);
        }
        if (threadIdx.x != 0) return;
        const double q = itm / nn;                         // every path counts: a NaN path is out of the money
        t.itm_fraction[static_cast<size_t>(z) * K + k] = q;
        if (z != 0) return;
        const double dmean = s / nn;
        double var = s2 / nn - dmean * dmean;
        if (var < 0.0) var = 0.0;
        double pq = q * (1.0 - q);
        if (pq < 0.0) pq = 0.0;
        double *o = t.base_out + k;
        o[0] = df * (t.gshift[k] + dmean);
        o[K] = df * sqrt(var) / sqrt(nn);
        o[2 * K] = -t.sg[k] * df * q;
        o[3 * K] = df * sqrt(pq) / sqrt(nn);
        o[4 * K] = itm;
    } else {
        double col[GREEKS_COLS];
#pragma unroll
        for (int j = 0; j < GREEKS_COLS; ++j) {
            if (j > 0) __syncthreads();
            col[j] = block_column_sum(base + j, t.n_rows, ld, lds);
        }
        if (threadIdx.x != 0) return;
        const double cnt = col[3];
        const double dmean = col[0] / cnt;                 // 0 / 0 -> NaN: no pair kept
        const double tmean = col[1] / cnt;
        double var = col[2] / cnt - tmean * tmean;
        if (var < 0.0) var = 0.0;
        const double two_h = 2.0 * t.steps[z];
        double *o = t.sens_out + static_cast<size_t>(z) * SVMC_GREEKS_SENS_ROWS * K + k;
        o[0] = df * dmean / two_h;
        o[K] = df * sqrt(var) / sqrt(nn) / two_h;
        o[2 * K] = cnt;
    }
}

// The launches of the tail (the job pass and its finish, then the pair pass and its finish), queued on `stream` (arguments checked by
// the caller: check_steps, check_quotes).  rows_host: [1 + 2P][m] device pointers, job-major.  image: host memory, the head of
// greeks_pinned's block, that must stay untouched until the stream has passed the upload -- page-locked in the fused drivers, which
// synchronise once for everything they queued.  base_out [SVMC_GREEKS_BASE_ROWS][K], sens_out [P][SVMC_GREEKS_SENS_ROWS][K]: device
// memory or device-visible pinned host memory; null: the block inside the workspace that *results_dev reports.
int greeks_payoff_enqueue(const char *fn, const double *const *rows_host, size_t n_path, const double *forwards_host,
                          const double *discfactors_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                          const size_t *strike_offsets_host, int n_params, const double *steps_host, const double *spot_sums,
                          double *base_out, double *sens_out, void *image, void *workspace, size_t workspace_bytes, hipStream_t stream,
                          double **results_dev)
{
    const int m = n_expiries, P = n_params;
    const size_t K = strike_offsets_host[m];
    const int G = quote_groups(m, strike_offsets_host, GREEKS_KT, false);
    GreeksTable t;
    Layout w{static_cast<unsigned char *>(workspace)}, h{static_cast<unsigned char *>(image)};
    const size_t image_bytes = greeks_workspace(w, n_path, m, K, G, P, t);
    if (workspace_bytes < w.bytes())
        return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": workspace too small (svmc_greeks_payoff_workspace_bytes)");
    for (int j = 0; j < (1 + 2 * P) * m; ++j) SVMC_REQUIRE(rows_host[j] != nullptr, std::string(fn) + ": null snapshot");
    greeks_fill_image(greeks_image(h, m, K, G, P), rows_host, forwards_host, discfactors_host, m, strikes_host, types_host,
                      strike_offsets_host, P, steps_host);
    SVMC_HIP_TRY(hipMemcpyAsync(workspace, image, image_bytes, hipMemcpyHostToDevice, stream));
    t.spot_sums = spot_sums;
    if (results_dev != nullptr) *results_dev = t.base_out;
    if (base_out != nullptr) t.base_out = base_out;
    if (sens_out != nullptr) t.sens_out = sens_out;
    if (K == 0) return SVMC_OK;
    // the job pass first: its finish leaves every job's in-the-money fractions where the pair pass reads them
    for (int pair_pass = 0; pair_pass <= (P > 0 ? 1 : 0); ++pair_pass) {
        const unsigned slots = pair_pass ? static_cast<unsigned>(P) : static_cast<unsigned>(1 + 2 * P);
        hipLaunchKernelGGL(greeks_payoff_kernel<GREEKS_KT>, dim3(t.n_rows, G, slots), dim3(BLOCK), 0, stream, t, n_path, pair_pass);
        if (int rc = check_launch(fn)) return rc;
        hipLaunchKernelGGL(greeks_finish_kernel, dim3(static_cast<unsigned>(K) * slots), dim3(BLOCK), 0, stream, t, n_path, pair_pass,
                           static_cast<int>(slots));
        if (int rc = check_launch(fn)) return rc;
    }
    return SVMC_OK;
}

}  // namespace svmc

using namespace svmc;

extern "C" {

int svmc_greeks_payoff_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, int n_params, size_t *bytes)
{
    SVMC_REQUIRE(bytes != nullptr && n_expiries >= 1, "svmc_greeks_payoff_workspace_bytes: null output or no expiries");
    SVMC_REQUIRE(n_params >= 0 && n_params <= SVMC_GREEKS_MAX_PARAMS, "svmc_greeks_payoff_workspace_bytes: n_params must be in [0, SVMC_GREEKS_MAX_PARAMS]");
    *bytes = greeks_payoff_workspace_bytes_of(n_path, n_expiries, total_strikes, n_params);
    return SVMC_OK;
}

int svmc_greeks_payoff_chain(const double *const *base_rows_host, const double *const *up_rows_host, const double *const *dn_rows_host,
                             size_t n_path, const double *forwards_host, const double *discfactors_host, int n_expiries,
                             const double *strikes_host, const int8_t *types_host, const size_t *strike_offsets_host, int n_params,
                             const double *steps_host, const double *spot_sums, double *greeks_host, double *sens_host, void *workspace,
                             size_t workspace_bytes, svmc_stream_t stream)
{
    const char *fn = "svmc_greeks_payoff_chain";
    SVMC_REQUIRE(base_rows_host && spot_sums && greeks_host && workspace && discfactors_host, std::string(fn) + ": null pointer");
    if (int rc = check_steps(fn, n_params, steps_host, 0)) return rc;
    if (int rc = check_quotes(fn, n_path, forwards_host, discfactors_host, n_expiries, strikes_host, types_host, strike_offsets_host, 1u << 24, 1))
        return rc;
    SVMC_REQUIRE(n_params == 0 || (up_rows_host && dn_rows_host && sens_host), std::string(fn) + ": null pointer");
    const int m = n_expiries, P = n_params;
    const size_t K = strike_offsets_host[m];
    std::vector<const double *> rows(static_cast<size_t>(1 + 2 * P) * m);
    for (int i = 0; i < m; ++i) {
        rows[i] = base_rows_host[i];
        for (int p = 0; p < P; ++p) {
            rows[static_cast<size_t>(1 + 2 * p) * m + i] = up_rows_host[static_cast<size_t>(p) * m + i];
            rows[static_cast<size_t>(2 + 2 * p) * m + i] = dn_rows_host[static_cast<size_t>(p) * m + i];
        }
    }
    std::vector<unsigned char> image(greeks_pinned(nullptr, m, K, P, nullptr));
    double *res = nullptr;
    if (int rc = greeks_payoff_enqueue(fn, rows.data(), n_path, forwards_host, discfactors_host, m, strikes_host, types_host,
                                       strike_offsets_host, P, steps_host, spot_sums, nullptr, nullptr, image.data(), workspace,
                                       workspace_bytes, as_stream(stream), &res))
        return rc;
    if (K > 0) {
        SVMC_HIP_TRY(hipMemcpyAsync(greeks_host, res, SVMC_GREEKS_BASE_ROWS * K * sizeof(double), hipMemcpyDeviceToHost, as_stream(stream)));
        if (P > 0)
            SVMC_HIP_TRY(hipMemcpyAsync(sens_host, res + SVMC_GREEKS_BASE_ROWS * K, static_cast<size_t>(SVMC_GREEKS_SENS_ROWS) * P * K * sizeof(double),
                                        hipMemcpyDeviceToHost, as_stream(stream)));
    }
    SVMC_HIP_TRY(hipStreamSynchronize(as_stream(stream)));  // the table's host image and the results' landing
    return SVMC_OK;
}

}  // extern "C"
