// svmc_internal.h -- error plumbing shared by the translation units of libsvmc.so
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

#include "svmc.h"

namespace svmc {

std::string &last_error_ref();
int fail(int code, const std::string &msg);

#define SVMC_HIP_TRY(expr)                                                                         \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return ::svmc::fail(SVMC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

#define SVMC_REQUIRE(cond, msg)                                                                    \
    do {                                                                                           \
        if (!(cond)) return ::svmc::fail(SVMC_ERR_INVALID_ARGUMENT, std::string(msg));             \
    } while (0)

inline hipStream_t as_stream(svmc_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// rows of the generators' per-WAVE spot partials ([column][wave], svmc_slice.h SliceOut): one per 64 paths.  A fused launch
// writes 2 columns per (expiry, parameter set), so its workspace holds wave_rows(n) x 2 x columns doubles
inline unsigned wave_rows(size_t n) { return static_cast<unsigned>((n + 63) / 64); }

// ---- svmc_kernels.hip: host functions every Monte Carlo unit shares, each defined once
// the calling host thread's armed clock-probe buffer (svmc_clock_probe_arm), or null: a launcher that passes the probe (the LogSV
// on-device-RNG generators and the volatility paths; no other family) passes this -- one function, one thread_local, whichever unit
uint64_t *&armed_probe();
// true: a launch of n_path paths runs the few-waves form of its generator (per-device cache; SVMC_FEW_WAVES_MAX_PATHS read
// once): ONE function for every unit
size_t device_simds();
bool few_waves_launch(size_t n_path);
// the argument checks of the stepping entry points; allow_null_spot: the on-device-RNG slice launchers' internal callers
int check_state(const char *fn, const double *x, const double *v, const double *q, int nb_steps, double dt);
int check_slice_args(const char *fn, size_t n_path, const double *x_snapshot, const double *spot_sums, const void *workspace,
                     size_t workspace_bytes, bool allow_null_spot = false);
// reduce_columns_kernel is launched from svmc_kernels.hip only: out[j] = sum_r partials_base[r row_stride + j col_stride],
// j < n_cols (no launch check)
void reduce_columns(unsigned n_cols, hipStream_t stream, const double *partials_base, unsigned n_rows, size_t row_stride,
                    size_t col_stride, double *out);
// the host side of the many-job table (svmc_jobs.h): the launch's slices and the checks every family makes first
struct ManySlices;
ManySlices many_slices(int n_slices, const int *nb_steps_host, const double *forwards_host);
int check_many(const char *fn, size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
               const uint32_t *call_ids);
// the checks of a chain's quotes that the Greeks and the conditional tails and their fused drivers make (discfactors_host null: not
// checked; "too many strikes": quotes_per_strike x K reaches strike_limit), and of n_params in [min_params, max] and its steps
int check_quotes(const char *fn, size_t n_path, const double *forwards_host, const double *discfactors_host, int n_expiries,
                 const double *strikes_host, const int8_t *types_host, const size_t *strike_offsets_host, size_t strike_limit,
                 size_t quotes_per_strike);
int check_steps(const char *fn, int n_params, const double *steps_host, int min_params);

// svmc_kernels.hip: launches whose model constants live in device memory (graph replay, svmc_chain.hip)
constexpr int LOGSV_CONSTS_DOUBLES = 13;
int fill_state_indirect(double *x, double *vol, double *qvar, size_t n_path, const double *vol0_dev, hipStream_t stream);
int logsv_slice_w_indirect(double *x, double *sigma, double *qvar, size_t n_path, int nb_steps, const double *consts_dev,
                           const double *W0, const double *W1, size_t ldw, double forward, double *x_snapshot,
                           double *qvar_snapshot, double *spot_sums, void *workspace, size_t workspace_bytes,
                           hipStream_t stream);
constexpr int MAX_FUSED_SLICES = 16;    // = MAX_CHAIN_SLICES of svmc_jobs.h
int logsv_chain_w_indirect(double *x, double *sigma, double *qvar, size_t n_path, int n_slices, const int *nb_steps_host,
                           const double *consts_dev, const double *vol0_dev, const double *const *W0s, const double *const *W1s,
                           size_t ldw, const double *forwards_host, double *x_snapshots, double *qvar_snapshots,
                           double *spot_sums, void *workspace, size_t workspace_bytes, hipStream_t stream);
constexpr int MAX_FUSED_SETS = 8;       // = MAX_CHAIN_SETS of svmc_kernels.hip
int logsv_chain_w_sets(size_t n_path, int n_sets, int n_slices, const int *nb_steps_host, const double *consts_dev,
                       const double *vol0_dev, const double *const *W0s, const double *const *W1s, size_t ldw,
                       const double *forwards_host, double *x_snapshots, double *qvar_snapshots, double *spot_sums,
                       void *workspace, size_t workspace_bytes, hipStream_t stream);
// the same chain for n_sets parameter sets on randoms REGENERATED in registers from (seed, call_id): no resident randoms
constexpr int LOGSV_FAST_CONSTS_DOUBLES = 9;
int logsv_chain_rng_sets(size_t n_path, int n_sets, int n_slices, const int *nb_steps_host, const double *consts_dev,
                         const double *vol0_dev, const double *forwards_host, uint64_t seed, uint32_t call_id,
                         uint64_t path_offset, double *x_snapshots, double *qvar_snapshots, double *spot_sums, void *workspace,
                         size_t workspace_bytes, hipStream_t stream, bool allow_probe);
void logsv_fast_to_doubles(double dt, double theta, double kappa1, double kappa2, double beta, double volvol, double eta,
                           int is_spot_measure, double *out);
// payoff sums of n_sets parameter sets' snapshots in ONE launch and ONE column reduce (bit-equal to n_sets calls of
// svmc_payoff_sums_chain); payoff_sets_fit says whether the chain's strike groups fit one launch and the workspace
bool payoff_sets_fit(size_t n_path, int n_expiries, const size_t *offsets, const int8_t *types, int n_sets, size_t workspace_bytes);
int payoff_sums_chain_sets(const double *const *x_snapshots_host, const double *const *qvar_snapshots_host, size_t n_path,
                           const double *forwards_host, const double *ttms_host, const double *spot_sums, int n_expiries,
                           const double *strikes_host, const int8_t *types_host, const double *shifts_host,
                           const size_t *strike_offsets_host, int variable_type, double *sums, void *workspace,
                           size_t workspace_bytes, hipStream_t stream, int n_sets, size_t x_set_stride, size_t q_set_stride,
                           size_t spot_set_stride);
// ---- the one-device tail of an on-device-RNG chain (round 6): stepping that leaves its per-wave spot partials in `workspace`
// (spot_sums null, at most MAX_FUSED_SLICES expiries) or reduces them into spot_sums, then the payoff kernel (up to 2048 partial
// rows: every block sums its expiry's two columns itself) and chain_finish_kernel (a wave per quote: column sums in
// reduce_columns_kernel's order, stored where the host reads them)
int logsv_step_partials(double sigma0, double *x, double *sigma, double *qvar, size_t n_path, int n_slices, const int *nb_steps_host,
                        const double *dts_host, const double *etas_host, const double *forwards_host, double theta, double kappa1,
                        double kappa2, double beta, double volvol, int is_spot_measure, uint64_t seed, uint32_t call_id,
                        uint64_t path_offset, double *x_snapshots, double *qvar_snapshots, double *spot_sums, void *workspace,
                        size_t workspace_bytes, hipStream_t stream);
int heston_step_partials(double var0, double *x, double *var, double *qvar, size_t n_path, int n_slices, const int *nb_steps_host,
                         const double *dts_host, const double *forwards_host, double theta, double kappa, double rho, double volvol,
                         int scheme, uint64_t seed, uint32_t call_id, uint64_t path_offset, double *x_snapshots,
                         double *qvar_snapshots, double *spot_sums, void *workspace, size_t workspace_bytes, hipStream_t stream);
// svmc_hawkes.hip: the Hawkes jump-diffusion chain's stepping from (0, lambda_p, lambda_m) (params: SVMC_HAWKESJD_PARAMS doubles)
int hawkes_step_partials(const double *params_host, double *x, double *lam_p, double *lam_m, size_t n_path, int n_slices,
                         const int *nb_steps_host, const double *dts_host, const double *forwards_host, uint64_t seed,
                         uint32_t call_id, uint64_t path_offset, double *x_snapshots, double *spot_sums, void *workspace,
                         size_t workspace_bytes, hipStream_t stream);
// ---- many independent jobs of one chain in one stepping launch (svmc_*_chain_price_many): the launch uploads its job table
// (many_table_bytes, from the pinned table_host into table_dev) and writes job j's snapshot rows j m + i ([J m][n], qvar rows the
// same at qvar_snapshots) and per-wave spot partial column pairs 2 (j m + i) ([2 J m][wave_rows(n)]); params_host rows as in
// svmc.h.  payoff_sets_workspace_bytes bounds the workspace chain_payoff_and_finish_sets needs for the jobs' payoff partials.
// many_table_bytes is the largest of the families' *_many_table_bytes (svmc_kernels.hip, svmc_heston.hip, svmc_hawkes.hip).
size_t many_table_bytes(int n_jobs, int n_slices);
size_t logsv_many_table_bytes(int n_jobs, int n_slices);
size_t heston_many_table_bytes(int n_jobs, int n_slices);
int logsv_chain_rng_many(size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
                         const double *forwards_host, const double *params_host, int is_spot_measure, const uint64_t *seeds,
                         const uint32_t *call_ids, uint64_t path_offset, void *table_host, void *table_dev, double *x_snapshots,
                         double *qvar_snapshots, double *spot_partials, hipStream_t stream);
int heston_chain_rng_many(size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
                          const double *forwards_host, const double *params_host, int scheme, const uint64_t *seeds,
                          const uint32_t *call_ids, uint64_t path_offset, void *table_host, void *table_dev, double *x_snapshots,
                          double *qvar_snapshots, double *spot_partials, hipStream_t stream);
// svmc_hawkes.hip: the Hawkes jobs (params_host [n_jobs][SVMC_HAWKESJD_PARAMS], no qvar rows); hawkes_many_table_bytes is its share
// of many_table_bytes, hawkes_check_many the parameter checks of every job (made before anything is launched)
size_t hawkes_many_table_bytes(int n_jobs, int n_slices);
int hawkes_check_many(const char *fn, int n_jobs, const double *params_host);
int hawkes_chain_rng_many(size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
                          const double *forwards_host, const double *params_host, const uint64_t *seeds, const uint32_t *call_ids,
                          uint64_t path_offset, void *table_host, void *table_dev, double *x_snapshots, double *spot_partials,
                          hipStream_t stream);
// svmc_cmc.hip: the conditional Monte Carlo chain (svmc_*_chain_price_cmc) -- stepping from (mu, cv, vol, qvar) = (0, 0, vol0, 0)
// into the mu / cv snapshot rows, and the payoff tail: svmc_cmc_payoff_chain's body, or, with greeks_host [SVMC_CMC_GREEKS_ROWS][K]
// not null, svmc_cmc_greeks_chain's (prices_host and stderrs_host are then not read, stats_host is
// [m][SVMC_CMC_GREEKS_STATS_DOUBLES]); returns synchronised.  The sizes of its workspace and its page-locked block: svmc_quotes.h.
int logsv_cmc_step_from(double sigma0, double *mu, double *cv, double *sigma, double *qvar, size_t n_path, int n_slices,
                        const int *nb_steps_host, const double *dts_host, const double *etas_host, double theta, double kappa1,
                        double kappa2, double beta, double volvol, int is_spot_measure, uint64_t seed, uint32_t call_id,
                        uint64_t path_offset, double *mu_snapshots, double *cv_snapshots, hipStream_t stream);
int heston_cmc_step_from(double var0, double *mu, double *cv, double *var, double *qvar, size_t n_path, int n_slices,
                         const int *nb_steps_host, const double *dts_host, double theta, double kappa, double rho, double volvol,
                         uint64_t seed, uint32_t call_id, uint64_t path_offset, double *mu_snapshots, double *cv_snapshots,
                         hipStream_t stream);
// svmc_hawkes.hip: the Hawkes conditional stepping (row f16) from (0, lambda_p, lambda_m) into the mu / cv snapshot rows -- every
// cv row one double, formed on the host -- and the parameter block's checks (made by the fused drivers before anything else)
int hawkes_check_params(const char *fn, const double *params_host);
int hawkes_cond_step_from(const char *fn, const double *params_host, double *mu, double *lam_p, double *lam_m, size_t n_path,
                          int n_slices, const int *nb_steps_host, const double *dts_host, uint64_t seed, uint32_t call_id,
                          uint64_t path_offset, double *mu_snapshots, double *cv_snapshots, hipStream_t stream);
int cmc_tail(const char *fn, const double *const *mu_snapshots_host, const double *const *cv_snapshots_host, size_t n_path,
             const double *forwards_host, const double *discfactors_host, int n_expiries, const double *strikes_host,
             const int8_t *types_host, const size_t *strike_offsets_host, int recenter, double *prices_host, double *stderrs_host,
             double *greeks_host, double *stats_host, void *workspace, size_t workspace_bytes, hipStream_t stream, void *pinned,
             size_t pinned_bytes);
// ... many conditional jobs of one chain in ONE stepping launch (svmc_*_chain_cmc_many's body): the job table is filled in
// table_host (cmc_many_table_bytes; kept by the caller until the stream has passed the upload) and uploaded to table_dev, job j's
// rows are j m + i of mu_snapshots / cv_snapshots; params_host rows as svmc_*_chain_price_many.  `what`: fill the table in
// table_host, enqueue its upload and the launch, or both -- a captured upload and launch serve every later fill of the same sizes
constexpr int CMC_MANY_FILL = 1, CMC_MANY_ENQUEUE = 2;
size_t cmc_many_table_bytes(int n_jobs, int n_slices);
int logsv_cmc_step_many(const char *fn, size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
                        const double *params_host, int is_spot_measure, const uint64_t *seeds, const uint32_t *call_ids,
                        uint64_t path_offset, void *table_host, void *table_dev, double *mu_snapshots, double *cv_snapshots,
                        hipStream_t stream, int what = CMC_MANY_FILL | CMC_MANY_ENQUEUE);
int heston_cmc_step_many(const char *fn, size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
                         const double *params_host, const uint64_t *seeds, const uint32_t *call_ids, uint64_t path_offset,
                         void *table_host, void *table_dev, double *mu_snapshots, double *cv_snapshots, hipStream_t stream,
                         int what = CMC_MANY_FILL | CMC_MANY_ENQUEUE);
// ... and the tail of n_sets parameter sets of one chain (svmc_*_chain_price_cmc_sets): the sets as ONE table of n_sets x m expiries,
// set q's expiry i on rows q m + i of mu_snapshots / cv_snapshots.  cmc_sets_upload puts the table's image -- the chain and the
// buffers' addresses, nothing of the parameters -- at the head of `workspace` (cmc_sets_workspace_bytes) and returns synchronised;
// cmc_sets_enqueue queues the kernels alone, the last of which store prices, errors, statistics and (want_ivols) implied vols in
// the page-locked block `pinned` (cmc_sets_pinned_bytes), where cmc_sets_results finds them after the stream's synchronisation
size_t cmc_sets_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, int n_sets);
size_t cmc_sets_pinned_bytes(int n_expiries, size_t total_strikes, int n_sets);
int cmc_sets_upload(const char *fn, const double *mu_snapshots, const double *cv_snapshots, size_t n_path, const double *ttms_host,
                    const double *forwards_host, const double *discfactors_host, int n_expiries, const double *strikes_host,
                    const int8_t *types_host, const size_t *strike_offsets_host, int n_sets, void *workspace, size_t workspace_bytes,
                    void *pinned, hipStream_t stream);
int cmc_sets_enqueue(const char *fn, size_t n_path, int n_expiries, const size_t *strike_offsets_host, int n_sets, int recenter,
                     bool want_ivols, double vol_lo, double vol_hi, void *workspace, size_t workspace_bytes, void *pinned, hipStream_t stream);
void cmc_sets_results(void *pinned, int n_expiries, size_t total_strikes, int n_sets, const double **prices, const double **stderrs,
                      const double **stats, const double **ivols);
// ... and the sensitivity tail (svmc_cmc_sens_chain's body): the launches queued on `stream` from a host image the caller keeps
// until the stream has passed the upload (up / dn rows [P][m]; *results_dev: the [P][SVMC_CMC_SENS_ROWS][K] results on the
// device); the sizes of the workspace and of the host block [image | results' landing]: svmc_quotes.h
int cmc_sens_enqueue(const char *fn, const double *const *up_mu, const double *const *up_cv, const double *const *dn_mu,
                     const double *const *dn_cv, size_t n_path, const double *forwards_host, const double *discfactors_host, int n_expiries,
                     const double *strikes_host, const int8_t *types_host, const size_t *strike_offsets_host, int n_params,
                     const double *steps_host, int recenter, void *image, void *workspace, size_t workspace_bytes, hipStream_t stream,
                     double **results_dev);
// svmc_greeks.hip: the Greeks tail (svmc_greeks_payoff_chain's body) -- the launches queued on `stream` from a host image the
// caller keeps until the stream has passed the upload (rows_host [1 + 2P][m] job-major; base_out / sens_out device or pinned,
// null: inside the workspace at *results_dev); the sizes of the workspace and of the host block [image | results]: svmc_quotes.h
int greeks_payoff_enqueue(const char *fn, const double *const *rows_host, size_t n_path, const double *forwards_host,
                          const double *discfactors_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                          const size_t *strike_offsets_host, int n_params, const double *steps_host, const double *spot_sums,
                          double *base_out, double *sens_out, void *image, void *workspace, size_t workspace_bytes, hipStream_t stream,
                          double **results_dev);
size_t payoff_sets_workspace_bytes(size_t n_path, size_t total_strikes, int n_sets);
int chain_payoff_and_finish_sets(const double *const *x_snapshots_host, const double *const *qvar_snapshots_host, size_t n_path,
                                 const double *forwards_host, const double *ttms_host, const double *spot_sums, int n_expiries,
                                 const double *strikes_host, const int8_t *types_host, const double *shifts_host,
                                 const size_t *strike_offsets_host, int variable_type, void *workspace, size_t workspace_bytes,
                                 hipStream_t stream, int n_sets, size_t x_set_stride, size_t q_set_stride, size_t spot_set_stride,
                                 double *sums_dev, double *sums_out);
bool spot_sums_in_payoff_kernel(size_t n_path);
int reduce_spot_partials(const void *workspace, size_t n_path, int n_cols, double *spot_sums, hipStream_t stream);
int check_launch(const char *what);          // hipGetLastError -> SVMC_ERR_HIP "what: ..."

// The chain stepping of every on-device-RNG generator (LogSV: svmc_kernels.hip; Heston: svmc_heston.hip; Hawkes: svmc_hawkes.hip): the argument
// checks, launches of at most MAX_FUSED_SLICES expiries whose unused slice entries repeat a valid one, the step offset carried
// from launch to launch, and the reduce of each launch's per-wave spot partials into spot_sums -- with spot_sums null (one launch
// at most) they stay in `workspace`.  The model supplies fill(cs, i, j): entry i of its slices struct from expiry j (nb_steps and
// m are set here), and launch(cs, x_snap, q_snap, init, step_offset): one batch from its snapshot rows (q_snap nullable).
template <class Slices, class Init, class Fill, class Launch>
int step_chain(const char *fn, const Init &init, const double *x, const double *v, const double *q, size_t n_path, int n_slices,
               const int *nb_steps_host, const double *dts_host, const double *forwards_host, uint32_t call_id, uint32_t step_offset,
               double *x_snapshots, double *qvar_snapshots, double *spot_sums, void *workspace, size_t workspace_bytes,
               hipStream_t stream, Fill &&fill, Launch &&launch)
{
    SVMC_REQUIRE(x && v && q && x_snapshots && workspace, std::string(fn) + ": null pointer");
    SVMC_REQUIRE(nb_steps_host && dts_host && forwards_host && n_slices >= 1, std::string(fn) + ": null grids / no slices");
    SVMC_REQUIRE(spot_sums != nullptr || n_slices <= MAX_FUSED_SLICES, std::string(fn) + ": unreduced partials need one launch");
    SVMC_REQUIRE(call_id < (1u << 24), std::string(fn) + ": call_id must fit 24 bits");
    SVMC_REQUIRE(n_path > 0, std::string(fn) + ": n_path must be positive");
    for (int i = 0; i < n_slices; ++i)
        SVMC_REQUIRE(nb_steps_host[i] > 0 && dts_host[i] > 0.0, std::string(fn) + ": nb_steps and dt must be positive");
    for (int i0 = 0; i0 < n_slices; i0 += MAX_FUSED_SLICES) {
        Slices cs;
        cs.m = (n_slices - i0 < MAX_FUSED_SLICES) ? (n_slices - i0) : MAX_FUSED_SLICES;
        if (workspace_bytes < static_cast<size_t>(wave_rows(n_path)) * 2 * cs.m * sizeof(double))
            return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": workspace too small (svmc_slice_workspace_bytes)");
        uint32_t steps = 0;
        for (int i = 0; i < MAX_FUSED_SLICES; ++i) {
            const int j = (i < cs.m) ? i0 + i : i0;
            cs.nb_steps[i] = (i < cs.m) ? nb_steps_host[j] : 0;
            steps += static_cast<uint32_t>(cs.nb_steps[i]);
            fill(cs, i, j);
        }
        const size_t row = static_cast<size_t>(i0) * n_path;
        launch(cs, x_snapshots + row, qvar_snapshots ? qvar_snapshots + row : nullptr, (i0 == 0) ? init : Init(), step_offset);
        if (int rc = check_launch(fn)) return rc;
        if (spot_sums != nullptr)
            if (int rc = reduce_spot_partials(workspace, n_path, 2 * cs.m, spot_sums + 2 * i0, stream)) return rc;
        step_offset += steps;
    }
    return SVMC_OK;
}
int chain_payoff_and_finish(const double *const *x_snapshots_host, const double *const *qvar_snapshots_host, size_t n_path,
                            const double *forwards_host, const double *ttms_host, double *spot_sums, const double *spot_partials,
                            int n_expiries, const double *strikes_host, const int8_t *types_host, const double *shifts_host,
                            const size_t *strike_offsets_host, int variable_type, void *workspace, size_t workspace_bytes,
                            hipStream_t stream, double *sums_out);
constexpr int IV_QUOTE_DOUBLES_HOST = 6;   // = IV_QUOTE_DOUBLES of svmc_kernels.hip: {strike, code, shift, forward, ttm, df}
// ivols_out and sums_copy (nullable: the kernel also stores the 3 x n_quotes sums it read) may be device-visible pinned host
// memory: the results of a graph then reach the host without copy nodes
int chain_implied_vols(const double *sums_dev, const double *quotes_dev, size_t n_quotes, double n_path_total, double vol_lo,
                       double vol_hi, double *ivols_out, double *sums_copy, hipStream_t stream);
// svmc_comm.hip: ncclCommInitAll -- comms_out[n] communicators for the devices[n] of this process (svmc_multi.hip)
int rccl_comm_init_all(int n, const int *devices, void **comms_out);
void logsv_consts_to_doubles(double dt, double theta, double kappa1, double kappa2, double beta, double volvol, double eta,
                             int is_spot_measure, double *out);

}  // namespace svmc
