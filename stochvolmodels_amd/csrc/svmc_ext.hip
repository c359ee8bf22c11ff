// svmc_ext.hip -- libsvmc_ext.so, the model-agnostic estimators beside the closed core (include/svmc_ext.h).
// One translation unit on the header-only parts of csrc/; nothing of libsvmc.so is linked and no session is needed.
//
// Conditional Monte Carlo under the exponential risk-premia kernel (svmc_tilted_cond_payoff_chain; the header states the
// estimator, the keep rule, the recentring and the degenerate cases).  Four launches on one uploaded table:
//   tilted_cond_forward_kernel, tilted_cond_forward_finish_kernel   the statements of row f11's forward pass (svmc_cmc.hip): per
//                                expiry the sums of exp(mu + cv/2) - 1 and the kept count in the same blocks and the same order, so
//                                that corr is svmc_cmc_payoff_chain's to the bit; then K' = K + corr and ln K' once per strike
//   tilted_cond_payoff_kernel    block (path block, group of up to TC_KT strikes of one expiry, gamma): a thread forms per path
//                                sd and 1 / sd, the weight W and ln F_t once, then per strike the Black-76 price B and the sums of
//                                W d, (W d)^2, W (W d), d = B - shift; the expiry's seven statistics sums ride in the same block
//                                sum and are stored by the expiry's first group
//   tilted_cond_finish_kernel    a block per (quote | expiry, gamma): the column sums in row order, price, error, statistics
// The path blocks are quote_rows(n_path), a function of the path count alone; a strike's accumulators do not look at its
// neighbours' and the block sum's tree is the same for every accumulator index: a gamma's, an expiry's and a strike's results
// are the same bits whichever others share the call.  No atomics, no scratch, LDS for the block sums' exchange only.
// The four bodies, the table's walk and the host's check and driver are svmc_tilted_cond.h's, shared with libsvmc_est.so's tails (rows
// f18 to f20): this unit names the kernels, picks the path policy (TcTiltedPath) and the group width, and fills the image.
#include <hip/hip_runtime.h>

#include "svmc_ext.h"

#include "svmc_tilted_cond.h"

namespace svmc {

constexpr int TC_KT = 8;               // strikes per group: three accumulators and three constants per strike in vector registers

// the device table of a call (svmc_tilted_cond.h): zs the gammas [NG], q_partials [rows][NG][K][TC_PAY_COLS], stat_partials
// [rows][NG][m][TC_STAT_COLS], out: prices [NG][K], errors [NG][K], statistics [NG][m][SVMC_TILTED_STATS_DOUBLES]
struct TcTable : TcTableOf<double> {};
inline size_t tc_out_doubles(int m, size_t K, int NG)
{
    return static_cast<size_t>(NG) * (2 * K + static_cast<size_t>(SVMC_TILTED_STATS_DOUBLES) * m);
}
inline size_t tc_ext_workspace(Layout &w, size_t n_path, int m, size_t K, int G, int NG, TcTable &t)
{
    return tc_workspace(w, n_path, m, K, G, NG, NG, tc_out_doubles(m, K, NG), TC_PAY_COLS, TC_STAT_COLS, t);
}

// ---- the four kernels: the bodies of svmc_tilted_cond.h under this library's names -------------------------------------------------
__global__ __launch_bounds__(BLOCK) void tilted_cond_forward_kernel(TcTable t, size_t n)
{
    __shared__ double lds[4 * 3];
    tc_forward_body<false>(t, n, lds);
}

__global__ __launch_bounds__(BLOCK) void tilted_cond_forward_finish_kernel(TcTable t, int recenter)
{
    __shared__ double lds[4];
    tc_forward_finish_body(t, recenter, lds);
}

__global__ __launch_bounds__(BLOCK) void tilted_cond_payoff_kernel(TcTable t, size_t n)
{
    __shared__ double lds[4 * tc_payoff_sums(TC_KT)];
    tc_payoff_body<TC_KT, TcTiltedPath>(t, n, lds);
}

__global__ __launch_bounds__(BLOCK) void tilted_cond_finish_kernel(TcTable t, size_t n)
{
    __shared__ double lds[4];
    tc_finish_body<TcPlainWeights>(t, n, lds);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static bool tc_sizes_ok(size_t n_path, int n_expiries, int n_gammas)
{
    return n_path >= 1 && n_expiries >= 1 && n_gammas >= 1 && n_gammas <= SVMC_TILTED_MAX_GAMMAS;
}

}  // namespace svmc

using namespace svmc;

extern "C" {

int svmc_ext_version(void) { return SVMC_EXT_VERSION; }

int svmc_tilted_cond_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, int n_gammas, size_t *bytes)
{
    if (bytes == nullptr || !tc_sizes_ok(n_path, n_expiries, n_gammas)) return SVMC_ERR_INVALID_ARGUMENT;
    TcTable t;
    Layout w{nullptr};
    tc_ext_workspace(w, n_path, n_expiries, total_strikes, quote_groups_bound(n_expiries, total_strikes, TC_KT), n_gammas, t);
    *bytes = w.bytes();
    return SVMC_OK;
}

int svmc_tilted_cond_payoff_chain(const double *const *mu_snapshots_host, const double *const *cv_snapshots_host, size_t n_path,
                                  const double *forwards_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                  const double *shifts_host, const size_t *strike_offsets_host, const double *gammas_host, int n_gammas,
                                  int recenter, double *prices_host, double *stderrs_host, double *stats_host, void *workspace,
                                  size_t workspace_bytes, svmc_stream_t stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // everything is checked before anything is launched
    if (!mu_snapshots_host || !cv_snapshots_host || !forwards_host || !strikes_host || !types_host || !shifts_host ||
        !strike_offsets_host || !gammas_host || !prices_host || !stderrs_host || !stats_host || !workspace)
        return SVMC_ERR_INVALID_ARGUMENT;
    if (!tc_sizes_ok(n_path, n_expiries, n_gammas) || !tc_all_finite(gammas_host, n_gammas)) return SVMC_ERR_INVALID_ARGUMENT;
    const int m = n_expiries, NG = n_gammas;
    const int rc = tc_check_quotes(m, strike_offsets_host, mu_snapshots_host, cv_snapshots_host, forwards_host, strikes_host, shifts_host,
                                   types_host);
    if (rc != SVMC_OK) return rc;
    const size_t K = strike_offsets_host[m];
    const int G = quote_groups(m, strike_offsets_host, TC_KT, true);
    if (G > TC_MAX_GROUPS) return SVMC_ERR_INVALID_ARGUMENT;
    TcTable t;
    Layout w{static_cast<unsigned char *>(workspace)};
    std::vector<unsigned char> image(tc_ext_workspace(w, n_path, m, K, G, NG, t));
    if (workspace_bytes < w.bytes()) return SVMC_ERR_WORKSPACE;

    Layout h{image.data()};
    const TcImageOf<double> im = tc_image<double>(h, m, K, G, NG);
    tc_fill_image(im, m, strike_offsets_host, TC_KT, mu_snapshots_host, cv_snapshots_host, forwards_host, strikes_host, types_host,
                  [&](int, int k) { return shifts_host[k]; });
    for (int z = 0; z < NG; ++z) im.zs[z] = gammas_host[z];
    std::vector<double> out(tc_out_doubles(m, K, NG));
    const int run = tc_run(workspace, image, t.out, out, stream, [&]() {
        hipLaunchKernelGGL(tilted_cond_forward_kernel, dim3(t.rows, m), dim3(BLOCK), 0, stream, t, n_path);
        SVMC_TC_TRY(hipGetLastError());
        hipLaunchKernelGGL(tilted_cond_forward_finish_kernel, dim3(m), dim3(BLOCK), 0, stream, t, recenter ? 1 : 0);
        SVMC_TC_TRY(hipGetLastError());
        hipLaunchKernelGGL(tilted_cond_payoff_kernel, dim3(t.rows, G, NG), dim3(BLOCK), 0, stream, t, n_path);
        SVMC_TC_TRY(hipGetLastError());
        hipLaunchKernelGGL(tilted_cond_finish_kernel, dim3(static_cast<unsigned>(K) + m, NG), dim3(BLOCK), 0, stream, t, n_path);
        SVMC_TC_TRY(hipGetLastError());
        return SVMC_OK;
    });
    if (run != SVMC_OK) return run;
    const size_t GK = static_cast<size_t>(NG) * K;
    const double *block = tc_split(tc_split(out.data(), prices_host, GK), stderrs_host, GK);
    tc_split(block, stats_host, static_cast<size_t>(NG) * m * SVMC_TILTED_STATS_DOUBLES);
    return SVMC_OK;
}

}  // extern "C"
