/*
 * svmc.h -- C ABI of libsvmc.so, the MI355X (gfx950) Monte Carlo engine behind the StochVolModels
 * hot path (LogSV / Heston terminal-state generators + forward-recentred payoff reduction).
 *
 * The reference (ArturSepp/StochVolModels, pure Python + Numba) has no FFI of its own; each entry point
 * below names the reference function it replaces (paths relative to src/stochvolmodels/).  The binding
 * a maintainer of the reference would add is a ctypes stub: see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns an svmc status code (0 = SVMC_OK); svmc_last_error() gives the message of
 *     the last failure on the calling thread.  No exceptions cross the boundary.
 *   - all `double *` state / random / output pointers are DEVICE pointers on the current HIP device
 *     (svmc_set_device) unless the parameter name ends in `_host`.  Buffers are caller-owned.
 *   - every compute call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the default
 *     stream).  Outputs are valid after svmc_stream_synchronize(stream).
 *   - all arithmetic is IEEE fp64.  Option payoff codes are int8: C=0, P=1, IC=2, IP=3
 *     (utils/config.py:8-15); variable types are 1=LOG_RETURN, 2=Q_VAR, 3=SIGMA (utils/config.py:18-24).
 *   - random layout is the reference's: W[t * ldw + p], step-major, UNSCALED N(0,1)
 *     (pricers/logsv_pricer.py:1028-1030).
 *   - the library is thread-compatible: concurrent calls must use distinct streams and buffers.
 */
#ifndef SVMC_H
#define SVMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVMC_VERSION 100 /* 0.1.0 */

#if defined(__GNUC__) || defined(__clang__)
#define SVMC_API __attribute__((visibility("default")))
#else
#define SVMC_API
#endif

/* status codes */
#define SVMC_OK 0
#define SVMC_ERR_INVALID_ARGUMENT 1
#define SVMC_ERR_HIP 2
#define SVMC_ERR_UNKNOWN_PAYOFF 3       /* reference: ValueError("unknown option payoff code"), utils/mc_payoffs.py:84 */
#define SVMC_ERR_UNSUPPORTED_VARIABLE 4 /* reference: NotImplementedError for VariableType.SIGMA, utils/mc_payoffs.py:69-70 */
#define SVMC_ERR_WORKSPACE 5
#define SVMC_ERR_RCCL 6                 /* RCCL missing at run time, or a collective / communicator call failed */

#define SVMC_CALL 0
#define SVMC_PUT 1
#define SVMC_INV_CALL 2
#define SVMC_INV_PUT 3

#define SVMC_LOG_RETURN 1
#define SVMC_Q_VAR 2
#define SVMC_SIGMA 3

#define SVMC_HESTON_EULER_FLOOR 0 /* the reference's scheme, pricers/heston_pricer.py:373-379 */
#define SVMC_HESTON_QE 1          /* Andersen QE-M; new capability */

typedef void *svmc_stream_t;  /* hipStream_t */
typedef void *svmc_session_t; /* opaque: one GPU's resident chain-pricing buffers */
typedef void *svmc_event_t;  /* hipEvent_t */
typedef void *svmc_comm_t;   /* ncclComm_t (RCCL) */

/* ---- library / device plumbing (no reference counterpart: the reference is single-process NumPy) -- */
SVMC_API int svmc_version(void);
/* The version of the counter-based random stream the generators draw from (SVMC_RNG_STREAM_VERSION): results for a
 * given seed are reproducible only within one stream version.  1 = Philox4x32-10 + 52-bit Box-Muller (round 1);
 * 2 = Philox4x32-7, one call per two steps, 32-bit radius / angle Box-Muller (round 2); 3 = Philox4x32-7, one call per two
 * steps, each 32-bit word turned into one normal by a piecewise-cubic inverse CDF on the lattice (int32) word + 1/2 (round 3);
 * 4 = the same on the lattice (int32) word itself -- one instruction less per normal, still exactly symmetric (round 6).
 * CHANGELOG.md. */
#define SVMC_RNG_STREAM_VERSION 4
SVMC_API int svmc_rng_stream_version(void);
SVMC_API const char *svmc_last_error(void);
SVMC_API int svmc_device_count(int *count);
SVMC_API int svmc_set_device(int device);
SVMC_API int svmc_get_device(int *device);
SVMC_API int svmc_device_info(int device, char *name, size_t name_len, int *compute_units, int *clock_khz,
                     size_t *hbm_bytes);
SVMC_API int svmc_malloc(void **dptr, size_t bytes);
SVMC_API int svmc_free(void *dptr);
SVMC_API int svmc_host_alloc(void **hptr, size_t bytes); /* pinned host memory for async H2D/D2H */
SVMC_API int svmc_host_free(void *hptr);
SVMC_API int svmc_memset(void *dptr, int value, size_t bytes, svmc_stream_t stream);
SVMC_API int svmc_memcpy_h2d(void *dst, const void *src_host, size_t bytes, svmc_stream_t stream);
SVMC_API int svmc_memcpy_d2h(void *dst_host, const void *src, size_t bytes, svmc_stream_t stream);
SVMC_API int svmc_memcpy_d2d(void *dst, const void *src, size_t bytes, svmc_stream_t stream);
/* strided upload of a [height][width] double sub-matrix (a rank's path range of a host W array) */
SVMC_API int svmc_memcpy2d_h2d(void *dst, size_t dst_pitch_bytes, const void *src_host, size_t src_pitch_bytes,
                      size_t width_bytes, size_t height, svmc_stream_t stream);
SVMC_API int svmc_stream_create(svmc_stream_t *stream);
SVMC_API int svmc_stream_destroy(svmc_stream_t stream);
SVMC_API int svmc_stream_synchronize(svmc_stream_t stream);
SVMC_API int svmc_event_create(svmc_event_t *event);
SVMC_API int svmc_event_destroy(svmc_event_t event);
SVMC_API int svmc_event_record(svmc_event_t event, svmc_stream_t stream);
SVMC_API int svmc_event_synchronize(svmc_event_t event);
SVMC_API int svmc_event_elapsed_ms(svmc_event_t start, svmc_event_t stop, float *ms); /* synchronises on `stop` */
/* The shader clock an on-device-RNG LogSV stepping launch (svmc_logsv_*_rng*, svmc_logsv_vol_paths) ran at, measured inside
 * that kernel (no reference counterpart: measurement plumbing of bench.py's roofline).  OFF by default -- the
 * kernels take a null probe pointer and do nothing.  svmc_clock_probe_arm(1) arms the CALLING THREAD: it gets its own 8-word
 * device buffer (on the current device) and its later launches hand it to the kernel, where thread 0 of the launch's first
 * and last block stamp s_memtime (tick = shader cycle) and s_memrealtime (100 MHz) at kernel entry and after the time loop.
 * svmc_clock_probe_read synchronises `stream` and returns stamps[8] = [first block | last block][t_entry, r_entry, t_exit,
 * r_exit] of the thread's latest armed launch; clock = (t_exit - t_entry) / (r_exit - r_entry) x 100 MHz.
 * svmc_clock_probe_arm(0) disarms and frees.  Per thread, not global: engines on other threads neither see nor disturb it. */
SVMC_API int svmc_clock_probe_arm(int enable);
SVMC_API int svmc_clock_probe_read(uint64_t *stamps, svmc_stream_t stream);

/* ---- state ----------------------------------------------------------------------------------------
 * x0 = zeros, sigma0 = v0 * ones, qvar0 = zeros of pricers/logsv_pricer.py:832-834 and
 * pricers/heston_pricer.py:303-305, written directly in HBM. */
SVMC_API int svmc_fill_state(double *x, double *vol, double *qvar, size_t n_path, double x0, double vol0,
                    double qvar0, svmc_stream_t stream);

/* ---- counter-based randoms (replaces np.random.normal inside the generators,
 * pricers/logsv_pricer.py:1025-1026, pricers/heston_pricer.py:369-370) ------------------------------
 * Philox4x32-7, key = seed, counter = (path_lo, path_hi, call index, stream | call_id << 8).  Stream 0: one call
 * serves the two normals (w0, w1) of each of the two time steps 2c, 2c + 1: every 32-bit word becomes one N(0,1)
 * variate by a piecewise-cubic inverse normal CDF (stream version 4, |z| <= 6.23); stream 1: one 52-bit uniform in
 * (0,1) per call.  `path` is the GLOBAL path id path_offset + p, `step` the chain-global step id step_offset + t, so
 * results do not depend on how paths are sharded over GPUs or how a chain is sliced.  `call_id` distinguishes the
 * calls of one seed: it occupies 24 bits of the counter (every entry point rejects call_id >= 2^24), so a host that
 * numbers its calls must re-seed before its 16 777 216th call -- the Python host's set_seed() counter wraps there and
 * says so (utils/funcs.py).  Exact definition: DESIGN.md "RNG"; CPU twin: oracle/svmc_oracle.c. */
SVMC_API int svmc_fill_normals(double *W0, double *W1, size_t ldw, size_t n_path, int nb_steps, uint64_t seed,
                      uint32_t call_id, uint64_t path_offset, uint32_t step_offset, svmc_stream_t stream);
SVMC_API int svmc_fill_uniforms(double *U, size_t ldw, size_t n_path, int nb_steps, uint64_t seed,
                       uint32_t call_id, uint64_t path_offset, uint32_t step_offset, svmc_stream_t stream);

/* ---- LogSV generator: simulate_logsv_x_vol_terminal, pricers/logsv_pricer.py:950-1047 ------------
 * In-place update of (x, sigma, qvar) over nb_steps log-Euler steps of size dt (Eq. 3.59).
 * _rng draws its increments on device (reference branch W0 is None, :1022-1026);
 * _w consumes supplied unscaled normals (reference branch :1028-1030). */
SVMC_API int svmc_logsv_terminal_rng(double *x, double *sigma, double *qvar, size_t n_path, int nb_steps, double dt,
                            double theta, double kappa1, double kappa2, double beta, double volvol,
                            double vol_backbone_eta, int is_spot_measure, uint64_t seed, uint32_t call_id,
                            uint64_t path_offset, uint32_t step_offset, svmc_stream_t stream);
/* Fused slice op for chain pricing: advance the state like svmc_logsv_terminal_rng AND, in the same kernel, copy
 * the terminal x (and qvar when qvar_snapshot != NULL) to the per-expiry snapshots and reduce
 * spot_sums[0..1] = { sum over non-NaN of forward*exp(x), count } (utils/mc_payoffs.py:61-62; the first step of
 * compute_mc_vars_payoff, see the payoff section below).  workspace >= svmc_slice_workspace_bytes(n_path). */
SVMC_API int svmc_logsv_slice_rng(double *x, double *sigma, double *qvar, size_t n_path, int nb_steps, double dt,
                                  double theta, double kappa1, double kappa2, double beta, double volvol,
                                  double vol_backbone_eta, int is_spot_measure, uint64_t seed, uint32_t call_id,
                                  uint64_t path_offset, uint32_t step_offset, double forward, double *x_snapshot,
                                  double *qvar_snapshot, double *spot_sums, void *workspace,
                                  size_t workspace_bytes, svmc_stream_t stream);
/* ALL expiries of a chain in one stepping launch (per 16 slices): slice i advances nb_steps_host[i] steps of
 * dts_host[i] with vol backbone etas_host[i] (NULL = 1), then writes x_snapshots[i][n_path] (and qvar_snapshots[i]
 * when non-NULL) and spot_sums[2i..2i+1] for forwards_host[i] -- the expiry loop of logsv_mc_chain_pricer
 * (pricers/logsv_pricer.py:840-865) without a launch boundary, and its tail, per expiry.  Same bits as calling
 * svmc_logsv_slice_rng slice by slice with step_offset advanced by the steps done. */
SVMC_API int svmc_logsv_chain_rng(double *x, double *sigma, double *qvar, size_t n_path, int n_slices,
                                  const int *nb_steps_host, const double *dts_host, const double *etas_host,
                                  const double *forwards_host, double theta, double kappa1, double kappa2, double beta,
                                  double volvol, int is_spot_measure, uint64_t seed, uint32_t call_id,
                                  uint64_t path_offset, uint32_t step_offset, double *x_snapshots, double *qvar_snapshots,
                                  double *spot_sums, void *workspace, size_t workspace_bytes, svmc_stream_t stream);
SVMC_API int svmc_logsv_terminal_w(double *x, double *sigma, double *qvar, size_t n_path, int nb_steps, double dt,
                          double theta, double kappa1, double kappa2, double beta, double volvol,
                          double vol_backbone_eta, int is_spot_measure, const double *W0, const double *W1,
                          size_t ldw, svmc_stream_t stream);
/* svmc_logsv_terminal_w + the slice epilogue of svmc_logsv_slice_rng (snapshots, spot sums) in the same launch:
 * one expiry of logsv_mc_chain_pricer_fixed_randoms (pricers/logsv_pricer.py:1140-1160) */
SVMC_API int svmc_logsv_slice_w(double *x, double *sigma, double *qvar, size_t n_path, int nb_steps, double dt,
                                double theta, double kappa1, double kappa2, double beta, double volvol,
                                double vol_backbone_eta, int is_spot_measure, const double *W0, const double *W1,
                                size_t ldw, double forward, double *x_snapshot, double *qvar_snapshot,
                                double *spot_sums, void *workspace, size_t workspace_bytes, svmc_stream_t stream);

/* ---- LogSV volatility paths on the full time grid: simulate_vol_paths, pricers/logsv_pricer.py:870-947 ---
 * sigma_t[(t+1)*ld + p] for t = 0..nb_steps-1, row 0 = v0 (written too): an explicit Euler scheme on L = ln sigma
 * driven by ONE Brownian motion with volatility vartheta = sqrt(beta^2 + volvol^2) (:937-945).  `brownians` are
 * the reference's SCALED increments sqrt(dt)*N(0,1), [nb_steps][ldb]; NULL draws them on device (stream 2 of the
 * counter-based generator: step t uses component t&1 of the Box-Muller pair of counter step t>>1).
 * HBM-write-bound: 8 B per path-step (+8 B read when brownians are supplied). */
SVMC_API int svmc_logsv_vol_paths(double *sigma_t, size_t ld, size_t n_path, int nb_steps, double dt, double v0,
                                  double theta, double kappa1, double kappa2, double beta, double volvol,
                                  int is_spot_measure, const double *brownians, size_t ldb, uint64_t seed,
                                  uint32_t call_id, uint64_t path_offset, svmc_stream_t stream);

/* ---- reductions of a resident [n_rows][ld] path array over the PATH axis: what the reference's callers of simulate_vol_paths
 * do with the array on the host (papers/logsv_model_with_quadratic_drift/moments_vol_qvar.py:48 -- np.mean / np.std along axis 1
 * of (sigma_t - theta)^k, k = 1..4 -- and :98 -- of sigma_t and of the expanding time average of sigma_t^2), done in HBM so that
 * 8 numbers per time step cross PCIe instead of nb_path.
 *   svmc_row_power_sums          sums[j * n_rows + t] = sum over the n_cols paths of (a[t * ld + p] - center)^(j + 1),
 *                                j = 0 .. 2 n_moments - 1 (n_moments <= 4): mean_k = S_k / n, var_k = S_2k / n - mean_k^2 of the
 *                                k-th power; deterministic (fixed tree); workspace >= n_rows x 4 x 2 n_moments doubles
 *   svmc_expanding_mean_squares  out[t * ldo + p] = mean of a[u * ld + p]^2 over u = 0 .. t (pandas expanding().mean() of the
 *                                squares, moments_vol_qvar.py:102); out may not alias a */
SVMC_API int svmc_row_power_sums(const double *a, size_t ld, size_t n_rows, size_t n_cols, double center, int n_moments,
                                 double *sums, void *workspace, size_t workspace_bytes, svmc_stream_t stream);
SVMC_API int svmc_expanding_mean_squares(const double *a, size_t ld, size_t n_rows, size_t n_cols, double *out, size_t ldo,
                                         svmc_stream_t stream);

/* ---- Black-76 implied vols of one slice, HOST arrays in and out (no device work): the price -> vol step between a
 * pricer and the calibration objective, OptionChain.compute_model_ivols_from_chain_data data/option_chain.py:327-346
 * (which delegates to the third-party vanilla_option_pricers.infer_bsm_ivols_from_model_chain_prices; parity with it
 * is unpinned).  optiontypes: SVMC_CALL / SVMC_PUT, and SVMC_INV_CALL / SVMC_INV_PUT as the vanilla inversion of price x
 * forward (the Black-76 value of (S - K)^+ / S is the vanilla value over the forward); another code gives
 * SVMC_ERR_UNKNOWN_PAYOFF.  A quote whose price is not strictly inside (price(vol_lo), price(vol_hi)) -- or is NaN -- gets NaN. */
SVMC_API int svmc_black_implied_vols(const double *prices, const double *strikes, const int8_t *optiontypes,
                                     size_t n_strikes, double forward, double ttm, double discfactor, double vol_lo,
                                     double vol_hi, double *ivols);

/* ---- rough LogSV (Markovian lift, n_factors <= 3): log_spot_full_combined_f64, pricers/rough_logsv/
 * split_simulation.py:335-356 (Strang splitting :249-278 over drift_ode_solve2 :86-128 and diffus_sde_solve_f64
 * :228-246; log-spot update :281-332).  In-place advance of (log_s[n], vol[n_factors][n], qvar[n]) over nb_steps of
 * size h.  nodes / weights / v0 are HOST arrays of n_factors entries (v0 = the factors' fixed reference level,
 * sigma0 / sum(weights) in the chain pricer :1187).  Z0 (factors) and Z1 (spot) are UNSCALED N(0,1), [nb_steps][ldw],
 * the reference's only interface for this model; pass both NULL to draw them on device (stream 3 of the
 * counter-based generator).  from_origin != 0 starts every path at (0, v0, 0) instead of reading the state arrays
 * (the chain pricer re-simulates each expiry from time 0, :1206-1216).  rho = beta / volvol, volvol = sqrt(beta^2 + orthog_vol^2) (:1190-1191). */
SVMC_API int svmc_rough_logsv_terminal(double *log_s, double *vol, double *qvar, size_t n_path, int nb_steps, double h,
                                       int n_factors, const double *nodes_host, const double *weights_host,
                                       const double *v0_host, double theta, double kappa1, double kappa2, double rho,
                                       double volvol, const double *Z0, const double *Z1, size_t ldw, uint64_t seed,
                                       uint32_t call_id, uint64_t path_offset, uint32_t step_offset, int from_origin,
                                       svmc_stream_t stream);
/* the same with the slice epilogue (x_snapshot <- log_s, qvar_snapshot <- qvar, spot sums): one expiry of
 * rough_logsv_mc_chain_pricer_fixed_randoms (pricers/logsv_pricer.py:1206-1230) in one stepping launch */
SVMC_API int svmc_rough_logsv_slice(double *log_s, double *vol, double *qvar, size_t n_path, int nb_steps, double h,
                                    int n_factors, const double *nodes_host, const double *weights_host,
                                    const double *v0_host, double theta, double kappa1, double kappa2, double rho,
                                    double volvol, const double *Z0, const double *Z1, size_t ldw, uint64_t seed,
                                    uint32_t call_id, uint64_t path_offset, uint32_t step_offset, int from_origin,
                                    double forward, double *x_snapshot, double *qvar_snapshot, double *spot_sums,
                                    void *workspace, size_t workspace_bytes, svmc_stream_t stream);
/* ALL expiries of rough_logsv_mc_chain_pricer_fixed_randoms (pricers/logsv_pricer.py:1206-1230) in ONE stepping launch: the
 * reference re-simulates every expiry from time 0 with its own step, so the expiries are independent simulations and run
 * side by side (grid.y = expiry).  Expiry i takes nb_steps_host[i] steps of hs_host[i] on rows 0 .. nb_steps_host[i] - 1 of
 * Z0 / Z1 (both NULL: drawn on device, stream 3, steps 0 ..); x_snapshots [n_expiries][n_path], qvar_snapshots the same or
 * NULL, spot_sums [2 n_expiries]; the state arrays receive the last expiry's terminal state.  Same bits per expiry as
 * svmc_rough_logsv_slice(from_origin = 1).  n_expiries <= 16. */
SVMC_API int svmc_rough_logsv_chain(double *log_s, double *vol, double *qvar, size_t n_path, int n_expiries,
                                    const int *nb_steps_host, const double *hs_host, const double *forwards_host,
                                    int n_factors, const double *nodes_host, const double *weights_host,
                                    const double *v0_host, double theta, double kappa1, double kappa2, double rho,
                                    double volvol, const double *Z0, const double *Z1, size_t ldw, uint64_t seed,
                                    uint32_t call_id, uint64_t path_offset, double *x_snapshots, double *qvar_snapshots,
                                    double *spot_sums, void *workspace, size_t workspace_bytes, svmc_stream_t stream);

/* ---- Heston generator: simulate_heston_x_vol_terminal, pricers/heston_pricer.py:334-381 ----------
 * `var` is the variance (the reference returns variance, not vol).  scheme = SVMC_HESTON_EULER_FLOOR
 * reproduces the reference (Euler, floor max(v, 1e-4)); SVMC_HESTON_QE is Andersen's QE-M. */
SVMC_API int svmc_heston_terminal_rng(double *x, double *var, double *qvar, size_t n_path, int nb_steps, double dt,
                             double theta, double kappa, double rho, double volvol, int scheme,
                             uint64_t seed, uint32_t call_id, uint64_t path_offset, uint32_t step_offset,
                             svmc_stream_t stream);
SVMC_API int svmc_heston_slice_rng(double *x, double *var, double *qvar, size_t n_path, int nb_steps, double dt,
                                   double theta, double kappa, double rho, double volvol, int scheme,
                                   uint64_t seed, uint32_t call_id, uint64_t path_offset, uint32_t step_offset,
                                   double forward, double *x_snapshot, double *qvar_snapshot, double *spot_sums,
                                   void *workspace, size_t workspace_bytes, svmc_stream_t stream);
/* all expiries of a Heston chain in one stepping launch (per 16 slices), as svmc_logsv_chain_rng: the expiry loop of
 * heston_mc_chain_pricer (pricers/heston_pricer.py:308-329); same bits as svmc_heston_slice_rng slice by slice */
SVMC_API int svmc_heston_chain_rng(double *x, double *var, double *qvar, size_t n_path, int n_slices,
                                   const int *nb_steps_host, const double *dts_host, const double *forwards_host,
                                   double theta, double kappa, double rho, double volvol, int scheme, uint64_t seed,
                                   uint32_t call_id, uint64_t path_offset, uint32_t step_offset, double *x_snapshots,
                                   double *qvar_snapshots, double *spot_sums, void *workspace, size_t workspace_bytes,
                                   svmc_stream_t stream);
/* The same four generators started from a UNIFORM state -- every path at (x0, vol0, qvar0), what a chain pricing begins with
 * (x0 = 0, sigma0 | v0, qvar0 = 0: pricers/logsv_pricer.py:823-826, pricers/heston_pricer.py:303-305) -- passed as three
 * constants: x / vol / qvar are then outputs only, and the svmc_fill_state launch (and its 24 bytes per path written, written
 * back and read again) disappears from the call. */
SVMC_API int svmc_logsv_slice_rng_from(double x0, double sigma0, double qvar0, double *x, double *sigma, double *qvar,
                                       size_t n_path, int nb_steps, double dt, double theta, double kappa1, double kappa2,
                                       double beta, double volvol, double vol_backbone_eta, int is_spot_measure,
                                       uint64_t seed, uint32_t call_id, uint64_t path_offset, uint32_t step_offset,
                                       double forward, double *x_snapshot, double *qvar_snapshot, double *spot_sums,
                                       void *workspace, size_t workspace_bytes, svmc_stream_t stream);
SVMC_API int svmc_logsv_chain_rng_from(double x0, double sigma0, double qvar0, double *x, double *sigma, double *qvar,
                                       size_t n_path, int n_slices, const int *nb_steps_host, const double *dts_host,
                                       const double *etas_host, const double *forwards_host, double theta, double kappa1,
                                       double kappa2, double beta, double volvol, int is_spot_measure, uint64_t seed,
                                       uint32_t call_id, uint64_t path_offset, uint32_t step_offset, double *x_snapshots,
                                       double *qvar_snapshots, double *spot_sums, void *workspace, size_t workspace_bytes,
                                       svmc_stream_t stream);
SVMC_API int svmc_heston_slice_rng_from(double x0, double var0, double qvar0, double *x, double *var, double *qvar,
                                        size_t n_path, int nb_steps, double dt, double theta, double kappa, double rho,
                                        double volvol, int scheme, uint64_t seed, uint32_t call_id, uint64_t path_offset,
                                        uint32_t step_offset, double forward, double *x_snapshot, double *qvar_snapshot,
                                        double *spot_sums, void *workspace, size_t workspace_bytes, svmc_stream_t stream);
SVMC_API int svmc_heston_chain_rng_from(double x0, double var0, double qvar0, double *x, double *var, double *qvar,
                                        size_t n_path, int n_slices, const int *nb_steps_host, const double *dts_host,
                                        const double *forwards_host, double theta, double kappa, double rho, double volvol,
                                        int scheme, uint64_t seed, uint32_t call_id, uint64_t path_offset,
                                        uint32_t step_offset, double *x_snapshots, double *qvar_snapshots, double *spot_sums,
                                        void *workspace, size_t workspace_bytes, svmc_stream_t stream);
SVMC_API int svmc_heston_terminal_w(double *x, double *var, double *qvar, size_t n_path, int nb_steps, double dt,
                           double theta, double kappa, double rho, double volvol, const double *W0,
                           const double *W1, size_t ldw, svmc_stream_t stream);
SVMC_API int svmc_heston_qe_terminal_w(double *x, double *var, double *qvar, size_t n_path, int nb_steps, double dt,
                              double theta, double kappa, double rho, double volvol, const double *Z0,
                              const double *Z1, const double *U, size_t ldw, svmc_stream_t stream);

/* ---- payoff reduction: compute_mc_vars_payoff, utils/mc_payoffs.py:10-88 -------------------------
 * Split at the two points where the reference needs a global quantity, so that a multi-GPU caller can
 * all-reduce the partial sums in between (sums are plain fp64 and add across ranks):
 *   1. svmc_spot_sums     spot_sums[0..1] = { sum over non-NaN of F*exp(x), count of non-NaN }  (:61-62)
 *   2. svmc_payoff_sums   per strike k, with d = payoff - shift_k over the non-NaN payoffs:
 *                         sums[3k..3k+2] = { sum d, sum d^2, count }; the recentring
 *                         c = spot_sums[0]/spot_sums[1] - F is read from device memory             (:63-86)
 *   3. svmc_payoff_finalize (host) price = DF*(shift + sum/cnt),
 *                         stderr = DF*sqrt(sum2/cnt - (sum/cnt)^2)/sqrt(N_total)                   (:85-88)
 * shifts_host (nullable = zeros) are any per-strike constants near the mean payoff (the host mirror uses
 * the intrinsic value at the forward); they only remove the cancellation in E[p^2] - E[p]^2.
 * `workspace` is a device scratch buffer of at least svmc_payoff_workspace_bytes() bytes. */
SVMC_API int svmc_payoff_workspace_bytes(size_t *bytes);
SVMC_API int svmc_slice_workspace_bytes(size_t n_path, size_t *bytes); /* covers the fused slice ops too */
SVMC_API int svmc_spot_sums(const double *x, size_t n_path, double forward, double *spot_sums, void *workspace,
                   size_t workspace_bytes, svmc_stream_t stream);
SVMC_API int svmc_payoff_sums(const double *x, const double *qvar, size_t n_path, double forward, double ttm,
                     const double *spot_sums, const double *strikes_host, const int8_t *types_host,
                     const double *shifts_host, size_t n_strikes, int variable_type, double *sums,
                     void *workspace, size_t workspace_bytes, svmc_stream_t stream);
/* svmc_payoff_sums for ALL expiries of a chain in one pair of launches (per 20 strike-chunks of 8): expiry i reads
 * the snapshots x_snapshots_host[i] (and qvar_snapshots_host[i] for Q_VAR; HOST arrays of DEVICE pointers), its
 * recentring sums spot_sums[2i..2i+1], forwards_host[i], ttms_host[i] and the strikes
 * [strike_offsets_host[i], strike_offsets_host[i+1]) of the concatenated strikes / types / shifts; sums gets the
 * 3 * strike_offsets_host[n_expiries] doubles in chain order.  Bit-identical to per-expiry svmc_payoff_sums. */
SVMC_API int svmc_payoff_sums_chain(const double *const *x_snapshots_host, const double *const *qvar_snapshots_host,
                                    size_t n_path, const double *forwards_host, const double *ttms_host,
                                    const double *spot_sums, int n_expiries, const double *strikes_host,
                                    const int8_t *types_host, const double *shifts_host,
                                    const size_t *strike_offsets_host, int variable_type, double *sums, void *workspace,
                                    size_t workspace_bytes, svmc_stream_t stream);
SVMC_API int svmc_payoff_finalize(const double *sums_host, const double *shifts_host, size_t n_strikes,
                         double discfactor, double n_path_total, double *prices_host, double *stderrs_host);
/* the same for all the strikes of a chain in one call: discfactors_host[k] is the discount factor of strike k's expiry
 * (the host mirror's chain driver finalises 8 x 21 strikes in one call instead of eight) */
SVMC_API int svmc_payoff_finalize_chain(const double *sums_host, const double *shifts_host, const double *discfactors_host,
                               size_t n_strikes, double n_path_total, double *prices_host, double *stderrs_host);

/* ---- fused single-GPU chain drivers: one call per option chain -----------------------------------------------
 * logsv_mc_chain_pricer (pricers/logsv_pricer.py:806-867) and heston_mc_chain_pricer (pricers/heston_pricer.py:
 * 285-331) as host C++ over the kernels above.  A session owns the resident state / snapshot / scratch buffers of
 * n_path paths on the current device and its own stream; chains of up to max_expiries maturities and
 * max_strikes_total strikes can be priced with it, any number of times.  Chain arrays are HOST arrays in the
 * reference's layout: ttms / forwards / discfactors [n_expiries], strikes and int8 payoff codes concatenated over the
 * expiries with strike_offsets[n_expiries + 1] delimiting each slice; prices / stderrs come back in the same
 * concatenated layout.  nb_steps_per_year is the reference's rule nb_steps_i = int((T_i - T_{i-1}) * spy) + 1
 * (utils/funcs.py:44).  vol_backbone_etas_host may be NULL (ones).  svmc_session_state copies the terminal state out
 * (x, sigma | variance, qvar; any pointer may be NULL).  Multi-GPU: give the session a communicator
 * (svmc_session_set_comm, below) and the same calls shard the job; the Python host mirror
 * (stochvolmodels_amd/mc_chain.py) places the same two all-reduces between the same kernels. */
SVMC_API int svmc_session_create(svmc_session_t *session, size_t n_path, int max_expiries, size_t max_strikes_total);
/* A session over state arrays and a stream the CALLER owns (device pointers x, vol, qvar of n_path doubles each; stream may be
 * NULL, the null stream): the session allocates its snapshots / sums / workspace only, every chain it prices leaves the terminal
 * state in the caller's arrays, and svmc_session_destroy frees neither them nor the stream.  path_offset = the global id of the
 * arrays' first path (a lone shard of a bigger job; 0 otherwise).  This is how the Python host prices a chain on ONE GPU: its
 * engine's resident state, one C-ABI call per chain instead of a dozen (logsv_mc_chain_pricer, pricers/logsv_pricer.py:806-867). */
SVMC_API int svmc_session_create_on(svmc_session_t *session, size_t n_path, int max_expiries, size_t max_strikes_total,
                                    double *x, double *vol, double *qvar, uint64_t path_offset, svmc_stream_t stream);
SVMC_API int svmc_session_destroy(svmc_session_t session);
/* Measurement: with timing enabled, svmc_logsv_chain_price / svmc_heston_chain_price bracket their stepping launch (and its
 * spot-sum reduce) with HIP events on the session's stream; svmc_session_last_stepping_ms returns the elapsed time of the last
 * such call (-1 if none was timed).  This is how bench.py times the dominant kernel inside its timed region without a profiler. */
SVMC_API int svmc_session_time_stepping(svmc_session_t session, int enable);
SVMC_API int svmc_session_last_stepping_ms(svmc_session_t session, float *ms);
SVMC_API int svmc_session_state(svmc_session_t session, double *x_host, double *vol_host, double *qvar_host);
SVMC_API int svmc_logsv_chain_price(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                    const double *discfactors_host, const double *vol_backbone_etas_host,
                                    int n_expiries, const double *strikes_host, const int8_t *types_host,
                                    const size_t *strike_offsets_host, double v0, double theta, double kappa1,
                                    double kappa2, double beta, double volvol, int is_spot_measure,
                                    int nb_steps_per_year, int variable_type, uint64_t seed, uint32_t call_id,
                                    double *prices_host, double *stderrs_host);
/* the same chain on supplied randoms resident in HBM: logsv_mc_chain_pricer_fixed_randoms, pricers/logsv_pricer.py:
 * 1100-1162.  W0s[i] / W1s[i] are DEVICE pointers to the UNSCALED N(0,1) of expiry i, [nb_steps_host[i]][ldw]; the
 * arrays of pointers, step counts and dts are host arrays of n_expiries entries.  This is the inner loop of an MC
 * calibration (:244-265): one call per optimizer iterate, nothing but the chain and the prices crosses PCIe. */
SVMC_API int svmc_logsv_chain_price_fixed(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                          const double *discfactors_host, const double *vol_backbone_etas_host,
                                          int n_expiries, const double *strikes_host, const int8_t *types_host,
                                          const size_t *strike_offsets_host, double v0, double theta, double kappa1,
                                          double kappa2, double beta, double volvol, int is_spot_measure,
                                          int variable_type, const double *const *W0s, const double *const *W1s,
                                          const int *nb_steps_host, const double *dts_host, size_t ldw,
                                          double *prices_host, double *stderrs_host);
/* the same call with the price -> implied-vol step of a calibration objective (data/option_chain.py:327-346) done where
 * the prices are: ivols_host [sum K_i] receives the Black-76 implied vols of the quotes of a LOG_RETURN chain ('IC' / 'IP':
 * of price x forward) on the bracket [1e-6, 10] (NaN outside it and for Q_VAR chains) -- on the graph route one more
 * kernel node and one more copy-back in the captured graph (svmc_black.h: the solver of svmc_black_implied_vols), on
 * the others the host routine after the prices.  ivols_host may be NULL (= svmc_logsv_chain_price_fixed). */
SVMC_API int svmc_logsv_chain_price_fixed_iv(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                             const double *discfactors_host, const double *vol_backbone_etas_host,
                                             int n_expiries, const double *strikes_host, const int8_t *types_host,
                                             const size_t *strike_offsets_host, double v0, double theta, double kappa1,
                                             double kappa2, double beta, double volvol, int is_spot_measure,
                                             int variable_type, const double *const *W0s, const double *const *W1s,
                                             const int *nb_steps_host, const double *dts_host, size_t ldw,
                                             double *prices_host, double *stderrs_host, double *ivols_host);
/* the same chain for SEVERAL PARAMETER SETS on the same resident randoms -- the base point of an optimizer iterate and its
 * finite-difference neighbours -- with the randoms read once: params_host [n_sets][6 + n_expiries] = {v0, theta, kappa1,
 * kappa2, beta, volvol, vol_backbone_eta of each expiry}, outputs [n_sets][sum K_i] (ivols_host may be NULL).  With 2..8
 * sets and a session created for n_sets chains (svmc_session_create(.., max_expiries >= n_sets * n_expiries,
 * max_strikes_total >= n_sets * sum K_i)) the replayed graph steps all sets in ONE launch, every lane carrying the n_sets
 * states of its path (the single-set launch is bound by reading the randoms); otherwise the sets are priced one after the
 * other.  Either way each set gets the bits svmc_logsv_chain_price_fixed_iv gives it. */
SVMC_API int svmc_logsv_chain_price_fixed_sets(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                               const double *discfactors_host, int n_expiries, const double *strikes_host,
                                               const int8_t *types_host, const size_t *strike_offsets_host, int n_sets,
                                               const double *params_host, int is_spot_measure, int variable_type,
                                               const double *const *W0s, const double *const *W1s,
                                               const int *nb_steps_host, const double *dts_host, size_t ldw,
                                               double *prices_host, double *stderrs_host, double *ivols_host);
/* The calibration chain with NO resident randoms: the fixed randoms of an MC calibration (pricers/logsv_pricer.py:244-265,
 * :520-527 draw them once and re-price on them at every optimizer iterate) are the counter-based stream of (seed, call_id),
 * regenerated in registers by every evaluation -- the same draws every time, nothing in HBM (10^5 paths x 364 steps of
 * resident W0 / W1 are 582 MB, and streaming them back is the floor of svmc_logsv_chain_price_fixed*).  n_sets parameter
 * sets (params_host [n_sets][6 + n_expiries] as for svmc_logsv_chain_price_fixed_sets) are stepped by ONE launch per 8 sets,
 * every lane drawing its path's normals once per step and advancing all the sets on them; outputs [n_sets][sum K_i].
 * Set q's prices are those of svmc_logsv_chain_price(seed, call_id) with set q's parameters on the grid (nb_steps_host,
 * dts_host), BIT FOR BIT (the same step arithmetic; tests/test_gpu_parity.py).  The session must be created for n_sets
 * chains (svmc_session_create(.., max_expiries >= min(n_sets, 8) x n_expiries, max_strikes_total >= min(n_sets, 8) x
 * sum K_i)).  The launches are captured into one hipGraph per set count and replayed; with a communicator attached
 * they are issued directly, the two all-reduces between them (global path ids: the job's result does not depend on the
 * sharding).  ivols_host may be NULL. */
SVMC_API int svmc_logsv_chain_price_frozen_sets(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                                const double *discfactors_host, int n_expiries, const double *strikes_host,
                                                const int8_t *types_host, const size_t *strike_offsets_host, int n_sets,
                                                const double *params_host, int is_spot_measure, int variable_type,
                                                const int *nb_steps_host, const double *dts_host, uint64_t seed,
                                                uint32_t call_id, double *prices_host, double *stderrs_host,
                                                double *ivols_host);
/* svmc_logsv_chain_price_fixed captures its launches (ONE stepping launch for all expiries that also initialises the
 * state and writes the spot sums' partials, their reduce, the payoff sums, D2H; a launch per expiry beyond 16 expiries)
 * into a hipGraph the first time it sees a (chain, randoms) combination and replays it afterwards -- the model
 * constants travel in a small device block the graph's first node refreshes.  On by default; results are identical
 * either way.  svmc_session_graph_launches counts the replays (diagnostics). */
SVMC_API int svmc_session_use_graphs(svmc_session_t session, int enable);
SVMC_API int svmc_session_graph_launches(svmc_session_t session, size_t *count);
SVMC_API int svmc_heston_chain_price(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                     const double *discfactors_host, int n_expiries, const double *strikes_host,
                                     const int8_t *types_host, const size_t *strike_offsets_host, double v0,
                                     double theta, double kappa, double rho, double volvol, int scheme,
                                     int nb_steps_per_year, int variable_type, uint64_t seed, uint32_t call_id,
                                     double *prices_host, double *stderrs_host);

/* ---- many independent jobs of one chain in one call ---------------------------------------------------------------
 * n_jobs jobs share the chain (ttms .. strike_offsets, n_expiries <= 16), the session's path count, the step grid and the
 * variable type (LogSV also is_spot_measure, Heston the scheme; Hawkes: SVMC_LOG_RETURN only); each has its own parameters and
 * random stream.  Job j's prices and standard errors (row j of prices_host / stderrs_host [n_jobs][sum K_i]) are those of
 * svmc_logsv_chain_price / svmc_heston_chain_price / svmc_hawkesjd_chain_price on the same session with job j's parameters,
 * seeds_host[j] and call_ids_host[j], BIT FOR BIT: ONE stepping launch steps every job (blockIdx.y = job), one payoff launch
 * and one finish launch serve them all.
 *   params_host  LogSV:  [n_jobs][6 + n_expiries]       v0 theta kappa1 kappa2 beta volvol, then the expiries' vol-backbone etas
 *                Heston: [n_jobs][5]                    v0 theta kappa rho volvol
 *                Hawkes: [n_jobs][SVMC_HAWKESJD_PARAMS] the block of svmc_hawkesjd_chain_price; both start intensities
 *                                                       (lambda_p, lambda_m) are per job
 * svmc_hawkesjd_chain_price_tilted_many is the same stepping launch followed, per job, by svmc_tilted_payoff_chain on that job's
 * snapshot rows (with recenter != 0 also its rows of the reduced spot sums), all on the session's stream and one synchronise:
 * job j equals svmc_hawkesjd_chain_price_tilted with its parameters, stream and gammas_host[j][0 .. n_gammas), bit for bit.
 * As there, no discount factors and no variable type (undiscounted prices of the log-return).  Outputs: prices_host /
 * stderrs_host [n_jobs][n_gammas][sum K_i], stats_host [n_jobs][n_gammas][n_expiries][SVMC_TILTED_STATS_DOUBLES].
 * Session: any single-GPU session whose max_expiries / max_strikes_total hold the chain (the sizes a single call of the chain
 * needs); the driver grows a per-job workspace of its own inside the session on demand -- about (1 or 2 with Q_VAR) x
 * n_jobs x n_expiries x n_path doubles of snapshots, kept until the session is destroyed -- and touches none of the
 * buffers, state arrays or graphs of the other drivers: a later single call returns what it would have returned.
 * At most SVMC_MANY_MAX_JOBS jobs per call (split longer lists).  Errors, all before anything is launched:
 *   SVMC_ERR_INVALID_ARGUMENT  n_jobs < 1 or > SVMC_MANY_MAX_JOBS, a null pointer (session included), n_expiries outside
 *                              [1, 16], a call id of 24 bits or more, an unknown scheme, a session with a communicator
 *                              or reducer attached (no sharded batch); Hawkes: a parameter block of ANY job that
 *                              svmc_hawkesjd_chain_price refuses (non-finite, sigma < 0, mean_p outside [0, 1), mean_m > 0),
 *                              and for the tilted call n_gammas outside 1 .. SVMC_TILTED_MAX_GAMMAS or a gamma, forward or
 *                              strike that is not finite;
 *   SVMC_ERR_UNSUPPORTED_VARIABLE  Hawkes: a variable_type other than SVMC_LOG_RETURN;
 *   SVMC_ERR_UNKNOWN_PAYOFF    the tilted call: a type code other than SVMC_CALL / SVMC_PUT;
 *   SVMC_ERR_WORKSPACE         a session too small for the chain (n_expiries > max_expiries or sum K_i > max_strikes_total);
 *   SVMC_ERR_HIP               the per-job workspace could not be allocated. */
#define SVMC_MANY_MAX_JOBS 64
SVMC_API int svmc_logsv_chain_price_many(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                         const double *discfactors_host, int n_expiries, const double *strikes_host,
                                         const int8_t *types_host, const size_t *strike_offsets_host, int n_jobs,
                                         const double *params_host, const uint64_t *seeds_host, const uint32_t *call_ids_host,
                                         int is_spot_measure, int nb_steps_per_year, int variable_type, double *prices_host,
                                         double *stderrs_host);
SVMC_API int svmc_heston_chain_price_many(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                          const double *discfactors_host, int n_expiries, const double *strikes_host,
                                          const int8_t *types_host, const size_t *strike_offsets_host, int n_jobs,
                                          const double *params_host, const uint64_t *seeds_host, const uint32_t *call_ids_host,
                                          int scheme, int nb_steps_per_year, int variable_type, double *prices_host,
                                          double *stderrs_host);
SVMC_API int svmc_hawkesjd_chain_price_many(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                            const double *discfactors_host, int n_expiries, const double *strikes_host,
                                            const int8_t *types_host, const size_t *strike_offsets_host, int n_jobs,
                                            const double *params_host, const uint64_t *seeds_host, const uint32_t *call_ids_host,
                                            int nb_steps_per_year, int variable_type, double *prices_host, double *stderrs_host);
SVMC_API int svmc_hawkesjd_chain_price_tilted_many(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                                   int n_expiries, const double *strikes_host, const int8_t *types_host,
                                                   const size_t *strike_offsets_host, int n_jobs, const double *params_host,
                                                   const uint64_t *seeds_host, const uint32_t *call_ids_host,
                                                   int nb_steps_per_year, const double *gammas_host, int n_gammas, int recenter,
                                                   double *prices_host, double *stderrs_host, double *stats_host);

/* ---- multi-GPU below the host language: RCCL over xGMI ----------------------------------------------------------
 * One process (or thread) per GPU.  Paths are independent, so rank r holds the global path ids
 * [path_offset, path_offset + n_path) of a job of n_path_total paths in its own session; the counter-based randoms
 * are indexed by the GLOBAL path id, so the job's result does not depend on how it is sharded.  The only cross-rank
 * couplings are the two reductions of compute_mc_vars_payoff -- the forward recentring's [sum F exp(x), count] per
 * expiry (utils/mc_payoffs.py:61-63) and [sum d, sum d^2, count] per strike (:85-86): with a communicator attached,
 * svmc_logsv_chain_price / svmc_heston_chain_price / svmc_logsv_chain_price_fixed issue them as two in-place fp64
 * ncclAllReduce(SUM) calls on the session's stream (2 M and 3 sum K_i doubles: a few KB, latency-bound on xGMI),
 * stream-ordered between the kernels, and every rank returns the job's prices and standard errors.
 * This is SURVEY.md 8b's design target `svmc_chain_price(... optional RCCL comm handle)`.
 *
 * RCCL is resolved at run time: the copy already mapped into the process if there is one (PyTorch-ROCm carries its
 * own), else librccl.so.1.  A communicator must be driven by the library that created it: create it with
 * svmc_rccl_comm_create, or make sure a foreign ncclComm_t comes from that same copy (svmc_rccl_origin says which).
 *   rank 0:     svmc_rccl_unique_id(id, sizeof id)  -> ship the SVMC_RCCL_UNIQUE_ID_BYTES to the other ranks
 *   every rank: svmc_set_device(r); svmc_rccl_comm_create(&comm, id, sizeof id, world, r);
 *               svmc_session_create(&s, n_local, ...); svmc_session_set_comm(s, comm, r, world, n_total, offset);
 *               svmc_logsv_chain_price(s, ...)      -> identical prices on every rank
 * svmc_session_set_comm(session, NULL, ...) detaches.  Graph replay of the fixed-randoms driver is bypassed while a
 * communicator is attached. */
#define SVMC_RCCL_UNIQUE_ID_BYTES 128
SVMC_API int svmc_rccl_available(void);              /* 1 when an RCCL could be resolved, else 0 (svmc_rccl_origin: why) */
SVMC_API const char *svmc_rccl_origin(void);         /* where RCCL was resolved from, or the reason it was not */
SVMC_API int svmc_rccl_unique_id(void *id_out, size_t bytes);
SVMC_API int svmc_rccl_comm_create(svmc_comm_t *comm, const void *id_bytes, size_t bytes, int world, int rank);
SVMC_API int svmc_rccl_comm_destroy(svmc_comm_t comm);
/* ncclCommCount / ncclCommUserRank of a communicator: the number of ranks RCCL itself sees in it (bench.py reports it as
 * rccl_ranks_seen) and this rank's index; rank_out may be NULL */
SVMC_API int svmc_rccl_comm_count(svmc_comm_t comm, int *world_out, int *rank_out);
SVMC_API int svmc_rccl_all_reduce_sum(svmc_comm_t comm, double *buf, size_t n, svmc_stream_t stream);
SVMC_API int svmc_session_set_comm(svmc_session_t session, svmc_comm_t comm, int rank, int world,
                                   uint64_t n_path_total, uint64_t path_offset);
/* The same sharding with the two sum all-reduces handed to the CALLER: fn(user, device_buf, n, stream) must leave in
 * device_buf (n doubles, written by kernels queued on `stream`) the element-wise sum over all ranks, visible to work queued
 * on `stream` afterwards, and return SVMC_OK -- MPI, a host-staged exchange, or several sessions of ONE process on one GPU
 * summing through host memory (tests/test_gpu_parity.py runs 2- and 3-shard jobs that way and requires the unsharded
 * session's prices to reduction-order rounding, 1e-12: the per-wave partial rows depend on where a shard starts).
 * fn == NULL detaches, as svmc_session_set_comm(session, NULL, ...). */
typedef int (*svmc_all_reduce_fn)(void *user, double *device_buf, size_t n, svmc_stream_t stream);
SVMC_API int svmc_session_set_reducer(svmc_session_t session, svmc_all_reduce_fn fn, void *user, int rank, int world,
                                      uint64_t n_path_total, uint64_t path_offset);

/* ---- single-process multi-device sessions ----------------------------------------------------------------------
 * The same sharding WITHOUT a process per GPU: logsv_mc_chain_pricer / heston_mc_chain_pricer (pricers/logsv_pricer.py:
 * 806-867, pricers/heston_pricer.py:285-331 -- one single-process NumPy loop in the reference) for a caller that owns
 * several devices from one process.  A multi-session is n_shards sessions of one job of n_path_total paths -- shard r
 * holds the global path ids [N r / R, N (r + 1) / R) on device devices_host[r] (NULL: r mod the visible devices), each
 * driven by its own host thread of the library -- and one svmc_multi_*_chain_price call prices the chain on all of them
 * concurrently and returns the job's prices (every shard finalises the same all-reduced sums; svmc_multi_info's
 * shards_agree says whether they came out bit-identical, as they must).  Arguments are those of svmc_logsv_chain_price /
 * svmc_heston_chain_price with the multi-session in place of the session.
 * reduce_mode picks the transport of the two sum all-reduces (utils/mc_payoffs.py:61-63, :85-86):
 *   SVMC_MULTI_REDUCE_RCCL  ncclCommInitAll, one communicator per device, the collectives issued on each shard's stream
 *                           (error if RCCL does not resolve or two shards share a device);
 *   SVMC_MULTI_REDUCE_HOST  a sum through page-locked host memory in rank order, one meeting point of the shard threads
 *                           per all-reduce -- no dependency beyond the HIP runtime, works with several shards on ONE
 *                           device (tests/test_gpu_multi.py prices C4's 8 x 2^21 shards that way on a one-GPU box);
 *   SVMC_MULTI_REDUCE_AUTO  RCCL where it can be had, else HOST; svmc_multi_info reports which one is in use.
 * Results equal one session of n_path_total paths up to the order of the final additions (the randoms are indexed by the
 * global path id) and do not depend on the transport.  A failing shard releases the others from the host meeting point
 * and the call returns its status and message; inside an RCCL collective a lost peer cannot be recovered from (RCCL's own
 * semantics).  Calls on one multi-session must not overlap; distinct multi-sessions are independent. */
typedef void *svmc_multi_t;
#define SVMC_MULTI_REDUCE_AUTO 0
#define SVMC_MULTI_REDUCE_HOST 1
#define SVMC_MULTI_REDUCE_RCCL 2
SVMC_API int svmc_multi_create(svmc_multi_t *multi, int n_shards, const int *devices_host, uint64_t n_path_total,
                               int max_expiries, size_t max_strikes_total, int reduce_mode);
SVMC_API int svmc_multi_destroy(svmc_multi_t multi);
/* any output may be NULL: shard count, transport in use (SVMC_MULTI_REDUCE_HOST / _RCCL), the ranks RCCL's warm-up
 * all-reduce counted (0 in host mode), and whether all shards returned identical bits in the last pricing call */
SVMC_API int svmc_multi_info(svmc_multi_t multi, int *n_shards, int *reduce_mode, int *rccl_ranks_seen, int *shards_agree);
/* shard r: its device, path range and the host wall time of its part of the last call (a slow device shows here) */
SVMC_API int svmc_multi_shard_info(svmc_multi_t multi, int shard, int *device, uint64_t *path_offset, uint64_t *n_path,
                                   double *last_call_ms);
SVMC_API int svmc_multi_logsv_chain_price(svmc_multi_t multi, const double *ttms_host, const double *forwards_host,
                                          const double *discfactors_host, const double *vol_backbone_etas_host,
                                          int n_expiries, const double *strikes_host, const int8_t *types_host,
                                          const size_t *strike_offsets_host, double v0, double theta, double kappa1,
                                          double kappa2, double beta, double volvol, int is_spot_measure,
                                          int nb_steps_per_year, int variable_type, uint64_t seed, uint32_t call_id,
                                          double *prices_host, double *stderrs_host);
SVMC_API int svmc_multi_heston_chain_price(svmc_multi_t multi, const double *ttms_host, const double *forwards_host,
                                           const double *discfactors_host, int n_expiries, const double *strikes_host,
                                           const int8_t *types_host, const size_t *strike_offsets_host, double v0,
                                           double theta, double kappa, double rho, double volvol, int scheme,
                                           int nb_steps_per_year, int variable_type, uint64_t seed, uint32_t call_id,
                                           double *prices_host, double *stderrs_host);
/* the terminal state of the whole job, shard by shard into [n_path_total] host arrays (any pointer may be NULL) */
SVMC_API int svmc_multi_state(svmc_multi_t multi, double *x_host, double *vol_host, double *qvar_host);

/* ---- analytic side: affine-expansion MGF + Fourier inversion ------------------
 * Complex arrays are interleaved (re, im) doubles, i.e. numpy.complex128 / C99 double complex, on the device.
 *   svmc_logsv_mgf_grid    compute_logsv_a_mgf_grid, pricers/logsv/affine_expansion.py:570-685 (numerical path):
 *                          per grid point integrate A' = A^T M A + L A + H (:67-205) over ttm from a[] (in: A at the
 *                          previous expiry, out: A at this one; [n_grid][5] for expansion_order 2, [n_grid][3] for 1)
 *                          and return log_mgf = sum_k A_k (sigma0 - theta)^k.  The reference calls SciPy RK45 at its
 *                          default rtol 1e-3 / atol 1e-6; here the Dormand-Prince 8(5,3) pair (DOP853) takes rtol/atol.
 *   svmc_heston_mgf_grid   compute_heston_mgf_grid, pricers/heston_pricer.py:183-214 (closed form; a, b carried).
 *   svmc_mgf_vanilla_slice the strike sums of vanilla_slice_pricer_with_mgf_grid, utils/mgf_pricer.py:174-221, for
 *                          grids with |Re phi| = 1/2: capped[k] = nansum_j Re[ w_j/(pi (p_j^2+1/4))
 *                          exp(-ln(F/K_k) phi_j + log_mgf_j) ] with the legacy Simpson weights (:158-171); the
 *                          payoff algebra on top (:208-219) is host code. */
SVMC_API int svmc_logsv_mgf_grid(const double *phi, const double *psi, size_t n_grid, double ttm, double sigma0,
                                 double theta, double kappa1, double kappa2, double beta, double volvol,
                                 int is_spot_measure, int expansion_order, double vol_backbone_eta, double *a,
                                 double *log_mgf, double rtol, double atol, svmc_stream_t stream);
/* Batched over parameter sets: n_sets independent LogSV models advance their transform grids over the same interval in
 * ONE launch (the five sets of config C5; the bumped parameter vectors of a finite-difference gradient).  Set s has its
 * own grid phi / psi [s][n_grid] (the grid scale follows sigma0), coefficients a [s][n_grid][n_coef] and output log_mgf
 * [s][n_grid]; params_host [s][SVMC_LOGSV_SET_DOUBLES] = {sigma0, theta, kappa1, kappa2, beta, volvol, vol_backbone_eta,
 * reserved}.  svmc_mgf_vanilla_slice_batch: the strike sums of every set for one (forward, strikes) slice, capped
 * [s][n_strikes].  Results are bit-identical to n_sets single calls. */
#define SVMC_LOGSV_SET_DOUBLES 8
SVMC_API int svmc_logsv_mgf_grid_batch(const double *phi, const double *psi, size_t n_grid, int n_sets, double ttm,
                                       const double *params_host, int is_spot_measure, int expansion_order, double *a,
                                       double *log_mgf, double rtol, double atol, svmc_stream_t stream);
SVMC_API int svmc_mgf_vanilla_slice_batch(const double *phi, const double *log_mgf, size_t n_grid, int n_sets,
                                          double forward, const double *strikes_host, size_t n_strikes, double *capped,
                                          svmc_stream_t stream);
SVMC_API int svmc_heston_mgf_grid(const double *phi, const double *psi, size_t n_grid, double ttm, double v0,
                                  double theta, double kappa, double volvol, double rho, double *a, double *b,
                                  int have_t0, double *log_mgf, svmc_stream_t stream);
/* the strike sums of slice_qvar_pricer_with_a_grid, utils/mgf_pricer.py:322-356 (options on the annualised quadratic
 * variance): capped[k] = nansum_j Re[ w_j/(pi psi_j^2) exp(K_k ttm psi_j + log_mgf_j) ], legacy Simpson weights */
SVMC_API int svmc_mgf_qvar_slice(const double *psi, const double *log_mgf, size_t n_grid, double ttm,
                                 const double *strikes_host, size_t n_strikes, double *capped,
                                 svmc_stream_t stream);
SVMC_API int svmc_mgf_vanilla_slice(const double *phi, const double *log_mgf, size_t n_grid, double forward,
                                    const double *strikes_host, size_t n_strikes, double *capped,
                                    svmc_stream_t stream);

/* ---- Hawkes jump-diffusion: pricers/hawkes_jd_pricer.py (F. Liu, N. Packham, A. Sepp 2025) ------------------------
 * params_host: SVMC_HAWKESJD_PARAMS doubles in the order of HawkesJDParams' fields = {mu, sigma, shift_p, mean_p, shift_m,
 * mean_m, lambda_p, theta_p, kappa_p, beta1_p, beta2_p, lambda_m, theta_m, kappa_m, beta1_m, beta2_m}; need sigma >= 0,
 * 0 <= mean_p < 1, mean_m <= 0.  Random streams 6 and 7 (src header svmc_rng.h): indexed by (global path id, chain-global step).
 *   svmc_hawkesjd_terminal_rng  simulate_hawkesjd_terminal (:715-779): nb_steps of dt on the state (x, lambda_p,
 *                               lambda_m) in place; the first step has the chain-global index step_offset.
 *   svmc_hawkesjd_chain_price   hawkesjd_mc_chain_pricer (:644-711) on a session: state (0, lambda_p, lambda_m) carried
 *                               over the expiries, per slice int((T_i - T_(i-1)) nb_steps_per_year) + 1 steps (the
 *                               reference hard-wires 1800 per year), payoffs as svmc_logsv_chain_price.  The session's
 *                               state arrays hold (x, lambda_p, lambda_m) afterwards.  variable_type SVMC_LOG_RETURN only.
 *                               With a communicator attached it issues the same two all-reduces.
 *   svmc_hawkesjd_mgf_grid      compute_hawkes_a_mgf_grid (:518-546): per grid point the three Riccati ODEs of
 *                               solve_ode_for_a (:582-640) over ttm from a[] ([n_grid][3] complex, in: the previous expiry's,
 *                               out: this one's) with DOP853 at rtol / atol; log_mgf = a0 + a1 lambda_p + a2 lambda_m.
 *   svmc_hawkesjd_mgf_grid_batch  the same for n_sets parameter sets side by side (the bumped vectors of a calibration's
 *                               finite-difference gradient): phi, psi [n_sets][n_grid] complex (each set its own grid),
 *                               params_host [n_sets][SVMC_HAWKESJD_PARAMS], a [n_sets][n_grid][3] complex, log_mgf
 *                               [n_sets][n_grid] complex.  Every set is checked before anything is launched; an invalid one
 *                               fails the whole call.  A grid point the integrator gives up on is NaN in its own set only.
 *                               Results are bit-identical to n_sets single calls.
 *   svmc_hawkesjd_risk_forwards_batch  hawkesjd_forwards_under_risk_kernel (:487-515) for n_sets parameter sets, each with its
 *                               own risk-premia gamma (gammas_host [n_sets]): per expiry the coefficient ODEs from zero over the
 *                               whole [0, ttm] at the real points phi = -gamma and -gamma - 1 (psi = 0); normalizer =
 *                               1 / exp(Re log E(-gamma)), gamma_forward = forward exp(Re log E(-gamma - 1)) normalizer.
 *                               normalizers, gamma_forwards: device [n_ttms][n_sets] (expiry-major).  ttms must be positive.
 *                               An ODE the integrator gives up on is NaN in its own set and expiry only.
 *   svmc_mgf_gamma_slice_batch  slice_pricer_with_mgf_grid_with_gamma (utils/mgf_pricer.py:273-321) of one expiry for n_sets
 *                               sets (phi, log_mgf [n_sets][n_grid] complex, each set its own grid): legacy Simpson weights,
 *                               the real shortcut (dp/pi)/(p^2 + 1/4) where shortcut_host[s] != 0, else the complex weight
 *                               -(dp/pi)/((phi + gamma + 1)(phi + gamma)); cap = nansum Re[w exp(-x phi + log E)], x =
 *                               log(forward / K); type code 0 ('C') gamma_forward - normalizer K^(1+gamma) cap, 1 ('P')
 *                               K - normalizer K^(1+gamma) cap, others SVMC_ERR_UNKNOWN_PAYOFF.  normalizers / gamma_forwards
 *                               are svmc_hawkesjd_risk_forwards_batch's device output, read at row `expiry`; prices: device
 *                               [n_sets][n_strikes], undiscounted. */
#define SVMC_HAWKESJD_PARAMS 16
SVMC_API int svmc_hawkesjd_terminal_rng(double *x, double *lambda_p, double *lambda_m, size_t n_path, int nb_steps,
                                        double dt, const double *params_host, uint64_t seed, uint32_t call_id,
                                        uint64_t path_offset, uint32_t step_offset, svmc_stream_t stream);
SVMC_API int svmc_hawkesjd_chain_price(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                       const double *discfactors_host, int n_expiries, const double *strikes_host,
                                       const int8_t *types_host, const size_t *strike_offsets_host,
                                       const double *params_host, int nb_steps_per_year, int variable_type, uint64_t seed,
                                       uint32_t call_id, double *prices_host, double *stderrs_host);
SVMC_API int svmc_hawkesjd_mgf_grid(const double *phi, const double *psi, size_t n_grid, double ttm,
                                    const double *params_host, double *a, double *log_mgf, double rtol, double atol,
                                    svmc_stream_t stream);
SVMC_API int svmc_hawkesjd_mgf_grid_batch(const double *phi, const double *psi, size_t n_grid, int n_sets, double ttm,
                                          const double *params_host, double *a, double *log_mgf, double rtol, double atol,
                                          svmc_stream_t stream);
SVMC_API int svmc_hawkesjd_risk_forwards_batch(const double *params_host, const double *gammas_host, int n_sets,
                                               const double *ttms_host, const double *forwards_host, size_t n_ttms,
                                               double *normalizers, double *gamma_forwards, double rtol, double atol,
                                               svmc_stream_t stream);
SVMC_API int svmc_mgf_gamma_slice_batch(const double *phi, const double *log_mgf, size_t n_grid, int n_sets,
                                        const double *gammas_host, const int *shortcut_host, const double *normalizers,
                                        const double *gamma_forwards, int expiry, double forward, const double *strikes_host,
                                        const int *type_codes_host, size_t n_strikes, double *prices, svmc_stream_t stream);

/* ---- densities, digital options, histograms (src svmc_density.hip) ---------------------------------------
 * The weights w are the legacy pricer weights of utils/mgf_pricer.py:157-171: Simpson 1,4,2,... with every odd index 4 (even-
 * length grids included), or with is_simpson = 0 half the first step on the first point and p_j - p_(j-1) on the others.  NaN
 * terms are dropped (nansum).  Batched like svmc_mgf_vanilla_slice_batch; a set of a batch is bit-equal to the set alone.
 *   svmc_mgf_pdf_slice_batch      pdf_with_mgf_grid (utils/mgf_pricer.py:361-384) for n_sets sets: var_grid, log_mgf device
 *                                 [n_sets][n_grid] complex (each set its own transform grid), space device [n_sets][n_space]
 *                                 (each set its own space grid, n_space >= 2), shifts_host / scales_host [n_sets];
 *                                 pdf[s][i] = (space[s][1] - space[s][0]) nansum_j Re[ (w_j / pi) exp(z u_j + log_mgf_j) ],
 *                                 z = (space[s][i] - shift[s]) / scale[s]; pdf: device [n_sets][n_space].
 *   svmc_mgf_digital_slice_batch  the strike sums of digital_slice_pricer_with_mgf_grid (:224-269): sums[s][k] = nansum_j
 *                                 Re[ p_j exp(-ln(F/K_k) phi_j + log_mgf_j) ], p_j = -(w_j / pi) / phi_j with negative_contour
 *                                 != 0 (every Re phi < 0: the sums are digital calls) and +(w_j / pi) / phi_j otherwise (puts);
 *                                 the complement 1 - sum for the other type and the discount factor are host code.  forward and
 *                                 strikes must be positive and finite.  sums: device [n_sets][n_strikes].
 *   svmc_histogram_uniform        np.histogram(values / divisor, bins = n_bins, range = (edges[0], edges[n_bins])) as integer
 *                                 counts: values outside the range and NaNs are dropped, the last bin owns its right edge, and
 *                                 the index is corrected against edges (device, n_bins + 1 doubles: the host's linspace) as NumPy
 *                                 corrects it, so the counts EQUAL NumPy's.  counts: device uint64 [n_bins], zeroed by the call;
 *                                 1 <= n_bins <= 8192; divisor 1 leaves the values as they are. */
SVMC_API int svmc_mgf_pdf_slice_batch(const double *var_grid, const double *log_mgf, size_t n_grid, int n_sets,
                                      const double *space, size_t n_space, const double *shifts_host, const double *scales_host,
                                      int is_simpson, double *pdf, svmc_stream_t stream);
SVMC_API int svmc_mgf_digital_slice_batch(const double *phi, const double *log_mgf, size_t n_grid, int n_sets, double forward,
                                          const double *strikes_host, size_t n_strikes, int negative_contour, int is_simpson,
                                          double *sums, svmc_stream_t stream);
SVMC_API int svmc_histogram_uniform(const double *values, size_t n, double divisor, const double *edges, int n_bins,
                                    uint64_t *counts, svmc_stream_t stream);

/* ---- Gaussian kernel density estimate of a resident vector (src svmc_density.hip) -------------------------
 * scipy.stats.gaussian_kde(kept)(points) of the samples values[i] / divisor (a division; 1 leaves them as they are):
 *   1. a sample v is dropped if it is NaN, if v > limit or if v < -limit (strict: +-limit itself is kept);
 *   2. mean = sum v / n_kept, then var = sum (v - mean)^2 / (n_kept - 1) over the kept samples (two passes, as np.cov);
 *   3. h = sqrt(var) factor, factor = bandwidth_factor where that is positive and Scott's n_kept^(-1/5) otherwise;
 *   4. density[j] = sum_i exp(-((points[j] - v_i) / h)^2 / 2) / (n_kept h sqrt(2 pi)).
 * values: device [n]; points, density: device [n_points], 1 <= n_points <= SVMC_KDE_MAX_POINTS; stats: device
 * [SVMC_KDE_STATS_DOUBLES] = {n_kept, n_nan, n_low, n_high, mean, var, h, factor}, the counts as doubles.  Six launches on
 * `stream`, no allocation, and no host round trip: the later launches read mean, h and n_kept from `stats` on the device.
 * Fewer than two kept samples, or a variance that is zero or not finite, are NOT errors of the call: the stats block reports
 * them, the density is whatever the arithmetic gives (NaN or inf), and the host decides.  Refused with
 * SVMC_ERR_INVALID_ARGUMENT: a null pointer, n < 1, n_points outside its range, a divisor or limit that is not positive and
 * finite, a non-finite bandwidth factor; with SVMC_ERR_WORKSPACE: a workspace below 8 (1280 + n_chunks n_points) bytes.
 * Deterministic: the order of every sum depends on n alone (the samples are cut into chunks whose length is a function of n;
 * a chunk's sum and then the chunks are added in a fixed order), so the density at a point is the same bits whichever other
 * points or vectors share the call.
 *   svmc_kde_workspace_bytes   host only: the workspace that serves any n_points <= SVMC_KDE_MAX_POINTS at this n, and (where
 *                              chunk_length is not NULL) the chunk length of this n. */
#define SVMC_KDE_TILE 8            /* evaluation points a thread of the density kernel keeps in registers */
#define SVMC_KDE_MAX_POINTS 4096
#define SVMC_KDE_STATS_DOUBLES 8
SVMC_API int svmc_kde_workspace_bytes(size_t n, size_t *bytes, size_t *chunk_length);
SVMC_API int svmc_kde_gaussian(const double *values, size_t n, double divisor, double limit, const double *points, int n_points,
                               double bandwidth_factor, double *density, double *stats, void *workspace, size_t workspace_bytes,
                               svmc_stream_t stream);

/* ---- weighted Gaussian kernel density estimate of a resident vector (src svmc_density.hip) ---------------
 * scipy.stats.gaussian_kde(kept, weights=w_kept)(points): svmc_kde_gaussian with a non-negative weight per sample.
 *   1. sample: v_i = values[i] / divisor (a division, as above);
 *   2. weight: w_i = (weights ? weights[i] : 1) * (tilt ? exp(gamma tilt[i]) : 1).  weights and tilt are device [n] or NULL;
 *      tilt is the UNdivided log-return, so qvar / ttm or the volatility can be weighted by exp(gamma x).  The exponential is
 *      inf above 746, +0 below -746 and NaN at NaN.  With both NULL no exponential is taken and w_i is the literal 1.0;
 *   3. sample i is kept iff v_i passes step 1 of svmc_kde_gaussian (not NaN, not beyond +-limit, strict comparisons), w_i >= 0,
 *      and w_i and w_i^2 are finite.  A dropped sample adds +0 to every sum.  A sample whose value fails is counted in n_nan /
 *      n_low / n_high whatever its weight; a sample whose value passes and whose weight fails (a NaN weight or tilt, a negative
 *      weight, an infinite weight, an overflowed exponential or square) is counted in n_bad_weight.  A zero weight is kept;
 *   4. sw = sum w, sw2 = sum w^2, neff = sw^2 / sw2 (formed as sw (sw / sw2)), mean = sum w v / sw, then var = sum w (v - mean)^2
 *      / (sw - sw2 / sw) over the kept samples (two passes, as np.cov(aweights=w, ddof=1));
 *   5. h = sqrt(var) factor, factor = bandwidth_factor where that is positive and Scott's neff^(-1/5) otherwise;
 *   6. density[j] = sum_i w_i exp(-((points[j] - v_i) / h)^2 / 2) / (sw h sqrt(2 pi)).
 * points, density: device [n_points], 1 <= n_points <= SVMC_KDE_MAX_POINTS; stats: device [SVMC_KDE_WEIGHTED_STATS_DOUBLES] =
 * {n_kept, n_nan, n_low, n_high, n_bad_weight, sum_w, neff, mean, var, h, factor, sum_w2}, the counts as doubles.  Six launches
 * on `stream`, no allocation, no host round trip.  Fewer than two kept samples, or a variance that is not positive and finite
 * (a single non-zero weight gives sw - sw2 / sw = 0), are NOT errors of the call: the stats block reports them, the density is
 * whatever the arithmetic gives, and the host decides.  Refused with SVMC_ERR_INVALID_ARGUMENT: a null values, points, density,
 * stats or workspace pointer, n < 1, n_points outside its range, a divisor or limit that is not positive and finite, a
 * non-finite bandwidth factor, a non-finite gamma (also where tilt is NULL); with SVMC_ERR_WORKSPACE: a workspace below
 * 8 (2048 + n_chunks n_points) bytes.
 * Deterministic: the chunk length and the order of every sum are svmc_kde_gaussian's and depend on n alone, so the density of a
 * (vector, weights, tilt, gamma) at a point is the same bits whichever other points, vectors or gammas share the stream.  With
 * weights == NULL and tilt == NULL every product with w = 1.0 is exact: the density, the four counts, mean, var, h and factor
 * EQUAL svmc_kde_gaussian's bit for bit (n_bad_weight = 0, sum_w = sum_w2 = neff = n_kept).  Several gammas are several calls.
 *   svmc_kde_weighted_workspace_bytes   host only: the workspace that serves any n_points <= SVMC_KDE_MAX_POINTS at this n (the
 *                                       first moment pass carries eight rows, so it is larger than svmc_kde_workspace_bytes),
 *                                       and (where chunk_length is not NULL) the chunk length, which is svmc_kde_gaussian's. */
#define SVMC_KDE_WEIGHTED_STATS_DOUBLES 12
SVMC_API int svmc_kde_weighted_workspace_bytes(size_t n, size_t *bytes, size_t *chunk_length);
SVMC_API int svmc_kde_gaussian_weighted(const double *values, const double *weights, const double *tilt, double gamma, size_t n,
                                        double divisor, double limit, const double *points, int n_points,
                                        double bandwidth_factor, double *density, double *stats, void *workspace,
                                        size_t workspace_bytes, svmc_stream_t stream);

/* ---- Monte Carlo prices under the exponential risk-premia kernel (src svmc_kernels.hip, svmc_chain.hip) ----
 * For one expiry with terminal log-returns x_j, forward F, strikes K_k of type 'C' / 'P' and one risk-premia gamma:
 *   w_j = exp(gamma x_j),  spot_j = F exp(x_j) - corr,  corr = 0, or with recenter != 0 the recentring of svmc_payoff_sums,
 *   spot_sums[0] / spot_sums[1] - F (the UNWEIGHTED mean of F exp(x) over the paths where it is not NaN, minus F);
 *   KEEP RULE: path j is kept iff x_j, w_j^2 and (w_j spot_j)^2 are all finite.  A dropped path adds nothing to any sum and is
 *   counted; every sum below runs over the kept paths.
 *   pay_jk = max(spot_j - K_k, 0) ('C') or max(K_k - spot_j, 0) ('P');
 *   price_k = sum_j w_j pay_jk / sum_j w_j  (undiscounted);
 *   stderr_k = sqrt(sum_j (w_j (pay_jk - price_k))^2) / sum_j w_j, the delta-method error of that ratio of sums, formed from
 *   sums of w d, (w d)^2 and w^2 d with d = pay - shift_k (shift_k: a host constant near the price, e.g. the intrinsic value at
 *   the forward; any finite value gives the same estimate, a near one keeps its error free of cancellation).
 * Per gamma and expiry the statistics block, SVMC_TILTED_STATS_DOUBLES doubles:
 *   {normalizer = n_kept / sum w, its error sqrt(sum (1 - normalizer w)^2) / sum w, gamma_forward = sum w spot / sum w, its error
 *    sqrt(sum (w (spot - gamma_forward))^2) / sum w, effective sample size (sum w)^2 / sum w^2, n_kept, n_dropped, sum w}.
 * No kept path, or kept paths of zero weight only, are NOT errors of the call: the prices are then 0/0 = NaN and the block says so.
 *   svmc_tilted_payoff_chain   model-agnostic: x_snapshots_host is a HOST array of n_expiries DEVICE pointers (as in
 *                              svmc_payoff_sums_chain); strikes / types / shifts concatenated, expiry i owning
 *                              [strike_offsets_host[i], strike_offsets_host[i + 1]); spot_sums: device [2 n_expiries], read
 *                              only when recenter != 0 (NULL otherwise).  prices, stderrs: [n_gammas][n_strikes], stats:
 *                              [n_gammas][n_expiries][SVMC_TILTED_STATS_DOUBLES], device memory or device-visible pinned host
 *                              memory.  Two launches on `stream` for a chain of up to 8 strike groups (a group: up to 22
 *                              strikes of one expiry) whose partial sums fit the workspace (svmc_payoff_workspace_bytes
 *                              always holds one gamma's), a pair more per further 8 groups or batch of gammas.  Every sum has
 *                              a fixed order that depends on n_path alone: a gamma's and an expiry's results are the same bits
 *                              whichever other gammas, strikes or expiries share the call.
 *   svmc_hawkesjd_chain_price_tilted   svmc_hawkesjd_chain_price's stepping launch ONCE for all gammas, then the launches above on
 *                              the session's snapshots; no path leaves the device.  Results land in host arrays of the shapes
 *                              above.  gamma = 0 with recenter != 0 is the plain measure (svmc_hawkesjd_chain_price at discount
 *                              factors 1).  Single-device sessions only.
 * Everything is checked before anything is launched: SVMC_ERR_INVALID_ARGUMENT for a null pointer, n_path < 1, n_expiries < 1,
 * n_gammas outside 1 .. SVMC_TILTED_MAX_GAMMAS, a gamma, forward, strike or shift that is not finite, recenter without
 * spot_sums; SVMC_ERR_UNKNOWN_PAYOFF for a type code other than SVMC_CALL / SVMC_PUT; SVMC_ERR_WORKSPACE for a workspace below
 * svmc_payoff_workspace_bytes. */
#define SVMC_TILTED_MAX_GAMMAS 16
#define SVMC_TILTED_STATS_DOUBLES 8
SVMC_API int svmc_tilted_payoff_chain(const double *const *x_snapshots_host, size_t n_path, const double *forwards_host,
                                      int n_expiries, const double *strikes_host, const int8_t *types_host,
                                      const double *shifts_host, const size_t *strike_offsets_host, const double *gammas_host,
                                      int n_gammas, int recenter, const double *spot_sums, double *prices, double *stderrs,
                                      double *stats, void *workspace, size_t workspace_bytes, svmc_stream_t stream);
SVMC_API int svmc_hawkesjd_chain_price_tilted(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                              int n_expiries, const double *strikes_host, const int8_t *types_host,
                                              const size_t *strike_offsets_host, const double *params_host,
                                              int nb_steps_per_year, uint64_t seed, uint32_t call_id, const double *gammas_host,
                                              int n_gammas, int recenter, double *prices_host, double *stderrs_host,
                                              double *stats_host);

/* ---- impermanent loss of a concentrated-liquidity range [pa, pb] (src svmc_density.hip, svmc_kernels.hip) ----
 * The payoff is the hold-minus-pool value of a unit-liquidity position opened at p0, per terminal spot S:
 *   pay(S) = -2 sqrt(S) 1{pa <= S <= pb} + sqrt(p0) (S / p0 + 1) + (pa - S)^+ / sqrt(pa) - (S - pb)^+ / sqrt(pb)
 *            - 2 sqrt(pa) 1{S < pa} - 2 sqrt(pb) 1{S > pb},
 * and the price is -(notional0 notional) E[pay], notional0 = 1 / (2 sqrt(p0) - p0 / sqrt(pb) - sqrt(pa)) (reference
 * papers/il_hedging/run_logsv_for_il_payoff.py: a put, a call, two digitals and a square-root payoff).
 *
 * TRANSFORM SIDE.  svmc_mgf_il_slice_batch: phi, log_mgf device [n_sets][n_grid] complex; x_host, xa_host, xb_host [n_cases] =
 * log p1, log pa, log pb (finite, xa < xb); sums: device [n_sets][n_cases][SVMC_IL_SLICE_SUMS], per case
 *   [0] nansum_j Re[ (v_j / pi) (exp((phi_j + 1/2) xb - phi_j x) - exp((phi_j + 1/2) xa - phi_j x)) / (phi_j + 1/2) exp(log_mgf_j) ]
 *   [1] nansum_j Re[ -(w_j / pi) / ((phi_j + 1) phi_j) exp(-(x - xa) phi_j + log_mgf_j) ]      [2] the same with xb
 *   [3] nansum_j Re[ (w_j / pi) / phi_j exp(-(x - xa) phi_j + log_mgf_j) ]                     [4] the same with xb
 * w: the legacy weights above; v: the validated weights of compute_integration_weights (utils/mgf_pricer.py:97-155) -- Simpson's
 * equal the legacy ones on the odd grids that rule accepts, with is_simpson = 0 one step on every point and half a step on the
 * first and the last (the host refuses the grids compute_integration_weights refuses).  [3], [4] are
 * svmc_mgf_digital_slice_batch's sums at negative_contour = 0; on a contour with every Re phi < 0 the host changes the sign of
 * the sum (the same bits as negated terms).  x - xa stands for the reference's log(p1 / pa): they differ by the rounding of the
 * logarithms.  The complement, forward - strike capped, the discount factor and the composition are host code.  Cases travel 32
 * to a launch; a case of a batch and a set of a batch are bit-equal to the case and the set alone.
 *
 * MONTE CARLO SIDE.  svmc_il_payoff on terminal log-returns x (device [n_path]) and the HOST table cases_host
 * [n_cases][SVMC_IL_CASE_DOUBLES] = {p1, p0, pa, pb, notional}, all positive and finite with pa < p0 < pb:
 *   KEEP RULE: path j is kept iff x_j and exp(x_j) are finite; a dropped path adds nothing and is counted;
 *   M = sum exp(x_j) / n_kept over the kept paths, ONE pass for all cases of the call;
 *   spot_j = p1 exp(x_j) - corr, corr = p1 M - p1 (compute_mc_vars_payoff's recentring: the spots' mean is p1).  Formed once per
 *   call, it differs from recentring every case by its own mean of p1 exp(x) by rounding only;
 *   pieces per kept path: sqrt(spot) where pa <= spot <= pb and 0 elsewhere (a negative recentred spot never reaches the square
 *   root), sqrt(p0) (spot / p0 + 1), (pa - spot)^+, (spot - pb)^+, 1{spot < pa}, 1{spot > pb}; pay_j as above;
 *   value = -(notional0 notional) mean(pay), formed as pay(p1) + mean(d), d_j = pay_j - pay(p1);
 *   stderr = (notional0 notional) sqrt(var / n_kept), var = max(mean(d^2) - mean(d)^2, 0) the population variance (0 at one kept path).
 * out_host [n_cases][SVMC_IL_OUT_DOUBLES] = {value, stderr, mean sqrt piece, mean linear piece, mean put, mean call, mean digital
 * put, mean digital call, n_kept, n_dropped}.  No kept path is not an error: the means are 0/0 = NaN and n_kept says so.  Three
 * launches on `stream`, one upload of the table, one download, one synchronize; `workspace` is device memory of
 * svmc_il_payoff_workspace_bytes(n_path, n_cases).  Every sum has a fixed order that depends on n_path alone: a case's results
 * are the same bits whichever other cases share the call.  Refused before anything is launched: SVMC_ERR_INVALID_ARGUMENT for a
 * null pointer, n_path < 1, n_cases outside 1 .. SVMC_IL_MAX_CASES, a case that breaks the conditions above; SVMC_ERR_WORKSPACE. */
#define SVMC_IL_SLICE_SUMS 5
#define SVMC_IL_CASE_DOUBLES 5
#define SVMC_IL_OUT_DOUBLES 10
#define SVMC_IL_MAX_CASES 65536
SVMC_API int svmc_mgf_il_slice_batch(const double *phi, const double *log_mgf, size_t n_grid, int n_sets, const double *x_host,
                                     const double *xa_host, const double *xb_host, size_t n_cases, int is_simpson, double *sums,
                                     svmc_stream_t stream);
SVMC_API int svmc_il_payoff_workspace_bytes(size_t n_path, size_t n_cases, size_t *bytes);
SVMC_API int svmc_il_payoff(const double *x, size_t n_path, const double *cases_host, size_t n_cases, double *out_host,
                            void *workspace, size_t workspace_bytes, svmc_stream_t stream);

/* ---- conditional Monte Carlo chain pricers, LogSV and Heston Euler (src svmc_cmc.hip, svmc_chain.hip) ----
 * Given the path of the volatility's driver b the log-return of the DISCRETISED schemes is exactly Gaussian.  LogSV
 * (pricers/logsv_pricer.py:1037-1045): the volatility moves on beta w0 + volvol w1 = vartheta b, the return on
 * w0 = rho b + sqrt(1 - rho^2) b_perp, rho = beta / vartheta, vartheta^2 = beta^2 + volvol^2 (vartheta = 0: rho = 0).  Heston Euler
 * (pricers/heston_pricer.py:372-379): the variance moves on b = rho w0 + rho_1 w1, the return on w0 = rho b + rho_1 b_perp.  So
 *   x_T | {b_t} ~ N(mu, cv),  mu = sum_t (alpha/2 eta^2 sigma_t^2 dt + rho eta sigma_t sqrt(dt) b_t),  cv = (1 - rho^2) sum_t eta^2 sigma_t^2 dt
 * over the values the steps START from (Heston: eta = 1, sigma_t^2 = v_t, alpha = -1), and integrating b_perp out leaves a Black-76
 * price per path: the estimator has the plain pricer's expectation for the same discretised model and a smaller variance.
 *
 * STEPPING.  svmc_logsv_chain_cmc / svmc_heston_chain_cmc advance the state (mu, cv, sigma | var, qvar), device [n_path] each, through
 * n_slices slices (any number: launches of 16) and write expiry i's mu and cv -- and qvar where qvar_snapshots is not null -- to row
 * i of mu_snapshots / cv_snapshots / qvar_snapshots ([n_slices][n_path]).  Arguments as svmc_logsv_chain_rng / svmc_heston_chain_rng
 * (Euler scheme) without the forwards, spot sums and workspace: the forward's statistics are svmc_cmc_payoff_chain's.  Randoms:
 * stream 8 of (seed, call_id), ONE normal per step, word step & 3 of call step >> 2 (chain-global step = step_offset + local
 * step); a chain sliced or continued differently sees the same bits.  Consecutive slices of one launch whose step constants (dt,
 * eta) are bit-equal are joined: the sums run on across the boundary and an expiry's values are the fold of the sums since the last
 * boundary that was not joined, so equal steps give the same values however they are cut into slices; ln sigma is derived once per
 * launch.  LogSV forms cv with the factor volvol^2 / vartheta^2 (1 when
 * vartheta = 0), Heston with 1 - rho^2.
 *
 * PAYOFF.  svmc_cmc_payoff_chain on any device arrays mu_snapshots_host[i], cv_snapshots_host[i] ([n_path], host arrays of device
 * pointers), strikes / types (SVMC_CALL | SVMC_PUT only: SVMC_ERR_UNKNOWN_PAYOFF otherwise) / strike_offsets as
 * svmc_payoff_sums_chain:
 *   KEEP RULE: a path is kept iff mu, cv and e = exp(mu + cv / 2) are finite and cv >= 0; a dropped path adds nothing and is counted;
 *   F_c = F e;  RECENTRING: corr = mean_kept(F_c) - F with recenter != 0 -- what the reference's nanmean(F exp(x)) - F becomes when
 *   b_perp is integrated out; it makes C - P = discfactor (F - K) hold per strike as the reference's does -- and corr = 0 otherwise;
 *   per (path, strike) the undiscounted Black-76 price of F_c against K' = K + corr at total variance cv, the call's formula for a
 *   call and the put's for a put, with ln F_c = ln F + mu + cv / 2 and ln K' formed once per strike;
 *   DEGENERATE: cv == 0 gives the intrinsic value of F_c against K'; K' <= 0 gives F_c - K' for a call and 0 for a put;
 *   price = discfactor x mean over the kept paths; error = discfactor x population deviation / sqrt(n_path), as
 *   compute_mc_vars_payoff divides.  The sums are taken of (price_j - shift), shift = the price of the expiry's path 0 (paths that
 *   agree to the bit then have error exactly 0), or the intrinsic value at F where that path is dropped.
 * prices_host, stderrs_host: [K] host; stats_host (nullable): [n_expiries][SVMC_CMC_STATS_DOUBLES] = {mean F_c, its standard error
 * (F x population deviation of e / sqrt(n_path)), corr, n_kept, n_dropped}.  One upload of the chain's table, four launches on
 * `stream` with no host round trip between them, the downloads, one synchronize.  Every sum has a fixed order that depends on
 * n_path alone (the path blocks of a launch are min(ceil(n_path / 256), 1024)): a strike's results are the same bits whichever other
 * strikes share the call.  `workspace`: device memory of svmc_cmc_payoff_workspace_bytes(n_path, n_expiries, total_strikes).
 *
 * FUSED.  svmc_logsv_chain_price_cmc / svmc_heston_chain_price_cmc: stepping from (0, 0, v0, 0) on the session's own state (its x
 * holds mu, its volatility array sigma | var afterwards) and the payoff in one call, arguments as svmc_logsv_chain_price /
 * svmc_heston_chain_price; stats_host as above, nullable.  LOG_RETURN only; a session that is part of a sharded job is refused
 * (SVMC_ERR_INVALID_ARGUMENT): cross-rank sums of the conditional estimator are a separate step. */
#define SVMC_CMC_STATS_DOUBLES 5
SVMC_API int svmc_logsv_chain_cmc(double *mu, double *cv, double *sigma, double *qvar, size_t n_path, int n_slices,
                                  const int *nb_steps_host, const double *dts_host, const double *etas_host, double theta,
                                  double kappa1, double kappa2, double beta, double volvol, int is_spot_measure, uint64_t seed,
                                  uint32_t call_id, uint64_t path_offset, uint32_t step_offset, double *mu_snapshots,
                                  double *cv_snapshots, double *qvar_snapshots, svmc_stream_t stream);
SVMC_API int svmc_heston_chain_cmc(double *mu, double *cv, double *var, double *qvar, size_t n_path, int n_slices,
                                   const int *nb_steps_host, const double *dts_host, double theta, double kappa, double rho,
                                   double volvol, uint64_t seed, uint32_t call_id, uint64_t path_offset, uint32_t step_offset,
                                   double *mu_snapshots, double *cv_snapshots, double *qvar_snapshots, svmc_stream_t stream);
SVMC_API int svmc_cmc_payoff_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, size_t *bytes);
SVMC_API int svmc_cmc_payoff_chain(const double *const *mu_snapshots_host, const double *const *cv_snapshots_host, size_t n_path,
                                   const double *forwards_host, const double *discfactors_host, int n_expiries,
                                   const double *strikes_host, const int8_t *types_host, const size_t *strike_offsets_host,
                                   int recenter, double *prices_host, double *stderrs_host, double *stats_host, void *workspace,
                                   size_t workspace_bytes, svmc_stream_t stream);
SVMC_API int svmc_logsv_chain_price_cmc(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                        const double *discfactors_host, const double *vol_backbone_etas_host, int n_expiries,
                                        const double *strikes_host, const int8_t *types_host, const size_t *strike_offsets_host,
                                        double v0, double theta, double kappa1, double kappa2, double beta, double volvol,
                                        int is_spot_measure, int nb_steps_per_year, int recenter, uint64_t seed, uint32_t call_id,
                                        double *prices_host, double *stderrs_host, double *stats_host);
SVMC_API int svmc_heston_chain_price_cmc(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                         const double *discfactors_host, int n_expiries, const double *strikes_host,
                                         const int8_t *types_host, const size_t *strike_offsets_host, double v0, double theta,
                                         double kappa, double rho, double volvol, int nb_steps_per_year, int recenter, uint64_t seed,
                                         uint32_t call_id, double *prices_host, double *stderrs_host, double *stats_host);

/* ---- conditional Monte Carlo Greeks: delta, dual delta, gamma and dual gamma (src svmc_cmc.hip, svmc_chain.hip) ----
 * The derivatives in F and K of the number svmc_cmc_payoff_chain returns, in closed form per path, each with a standard error.
 * Everything of the estimator above stands: the keep rule, h = mu + cv / 2, e = exp(h), F_c = F e, the mean over the kept paths.
 * c = mean_kept(e) - 1 with recentring and c = 0 without; K' = K + F c (= K + corr).  c depends on neither F nor K, so the formulas
 * below are the exact derivatives of the returned price.  Per kept path, s = +1 for a call and -1 for a put:
 *   sd = sqrt(cv);  d1 = (ln F_c - ln K') / sd + sd / 2;  d2 = d1 - sd
 *   B_f = N(d1) (call) | N(d1) - 1 (put);   B_k = -N(d2) (call) | N(-d2) (put)
 *   delta_i = e B_f + c B_k;   dual_delta_i = B_k;   dual_gamma_i = phi(d2) / (K' sd)
 *   gamma_i = e phi(d1) K^2 / (F sd K'^2) = (K / F)^2 dual_gamma_i, because F_c phi(d1) = K' phi(d2): dual gamma is accumulated and
 *   gamma and its error are scaled from it once per quote.
 *   DEGENERATE: cv == 0: B_f = s 1{s (F_c - K') > 0} (strict), B_k = -B_f, both gammas 0; such kept paths are counted per expiry
 *   (n_zero_cv).  K' <= 0: a call has B_f = 1, B_k = -1, a put has both 0; gammas 0.
 * Per quote value = discfactor x mean over the kept paths, error = discfactor x population deviation over the kept paths /
 * sqrt(n_path), the convention above.  The sums are taken of value_i - shift, shift = the value of the expiry's path 0 (paths that
 * agree to the bit have errors of exactly 0), or, where that path is dropped, the value at (mu, cv) = (0, 0): the intrinsic
 * quantities at F.  With recentring c is a sample mean and the errors ignore its noise, as the price's error does.  By construction,
 * to rounding: price = F delta + K dual_delta and F^2 gamma = K^2 dual_gamma.  Undiscounted, dual gamma is the simulated density of
 * the terminal spot at the strike, without a bandwidth.
 *   svmc_cmc_greeks_chain   arguments as svmc_cmc_payoff_chain, greeks_host [SVMC_CMC_GREEKS_ROWS][K] = {price, stderr, delta, its
 *                           error, dual delta, its error, gamma, its error, dual gamma, its error} in place of the two result
 *                           arrays; stats_host (nullable) [n_expiries][SVMC_CMC_GREEKS_STATS_DOUBLES]: the five statistics above,
 *                           then n_zero_cv.  price and stderr are the payoff entry's own four launches (bit-equal to it); then a
 *                           block column per path block and group of up to SVMC_CMC_GREEKS_KT strikes of one expiry and a finish
 *                           block per quote and expiry.  One upload, six launches, one download, one synchronize; every sum's
 *                           order depends on n_path alone, a quote's ten numbers are the same bits whichever strikes or expiries
 *                           share the call.  Refusals and status codes are svmc_cmc_payoff_chain's; `workspace`: device memory of
 *                           svmc_cmc_greeks_workspace_bytes(n_path, n_expiries, total_strikes).
 *   svmc_logsv_chain_price_cmc_greeks / svmc_heston_chain_price_cmc_greeks   the fused drivers: arguments as svmc_*_chain_price_cmc
 *                           with greeks_host for the two arrays; the session's workspace and page-locked block grow as theirs do;
 *                           a sharded session is refused.
 * Parameter sensitivities on this estimator: the row f14 block below; its calibration objective: the row f15 block.  Left out:
 * SVMC_INV_CALL / SVMC_INV_PUT, variables other than the log-return, the inverse measure, Heston QE, Hawkes, sharded sessions. */
#define SVMC_CMC_GREEKS_KT 4
#define SVMC_CMC_GREEKS_ROWS 10
#define SVMC_CMC_GREEKS_STATS_DOUBLES 6
SVMC_API int svmc_cmc_greeks_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, size_t *bytes);
SVMC_API int svmc_cmc_greeks_chain(const double *const *mu_snapshots_host, const double *const *cv_snapshots_host, size_t n_path,
                                   const double *forwards_host, const double *discfactors_host, int n_expiries,
                                   const double *strikes_host, const int8_t *types_host, const size_t *strike_offsets_host,
                                   int recenter, double *greeks_host, double *stats_host, void *workspace, size_t workspace_bytes,
                                   svmc_stream_t stream);
SVMC_API int svmc_logsv_chain_price_cmc_greeks(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                               const double *discfactors_host, const double *vol_backbone_etas_host, int n_expiries,
                                               const double *strikes_host, const int8_t *types_host,
                                               const size_t *strike_offsets_host, double v0, double theta, double kappa1,
                                               double kappa2, double beta, double volvol, int is_spot_measure, int nb_steps_per_year,
                                               int recenter, uint64_t seed, uint32_t call_id, double *greeks_host,
                                               double *stats_host);
SVMC_API int svmc_heston_chain_price_cmc_greeks(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                                const double *discfactors_host, int n_expiries, const double *strikes_host,
                                                const int8_t *types_host, const size_t *strike_offsets_host, double v0,
                                                double theta, double kappa, double rho, double volvol, int nb_steps_per_year,
                                                int recenter, uint64_t seed, uint32_t call_id, double *greeks_host,
                                                double *stats_host);

/* ---- Monte Carlo chain Greeks on common random numbers, LogSV and Heston (src svmc_greeks.hip, svmc_chain.hip) ----
 * One base job and, per requested parameter p with step h_p, a pair of jobs at theta_p + h_p (up) and theta_p - h_p (dn), all on
 * ONE random stream (the many-jobs block above: jobs of one (seed, call id) see the same draws and each is bit-equal to its single
 * call).  SVMC_CALL / SVMC_PUT on the log-return only.  Per expiry with forward F and discount factor DF, job j with terminal
 * log-returns x and reduced spot sums [sum F exp(x), count] over the paths where F exp(x) is not NaN:
 *   M_j = (sum / count) / F, the kept-path mean of exp(x);   e = (exp(x) - M_j) + 1;   spot = F e
 * -- compute_mc_vars_payoff's recentring F exp(x) - (mean - F) in its homogeneous form (it differs by rounding).  s = +1 for a
 * call, -1 for a put; pay = max(s (spot - K), 0), NaN where the spot is NaN.
 *   PRICE, STDERR of the base job: svmc_*_chain_price's own tail on job 0, bit-equal to the single call at the same seed.
 *   FORWARD DELTA (pathwise): g = s e 1{s (spot - K) > 0}; delta = DF mean(g), the exact derivative in F of the estimator the plain
 *     pricer computes (M does not depend on F); error = DF x population deviation of g / sqrt(n_path).  Means over ALL n_path paths:
 *     a path whose spot is NaN is out of the money (g = 0), as the plain payoff counts it.  The sums are taken of g - shift, shift =
 *     s 1{s (F - K) > 0}, g at the forward.
 *   DUAL DELTA: dual_delta = -s DF n_itm / n_path, n_itm the count of 1{s (spot - K) > 0}; error DF sqrt(q (1 - q) / n_path), q =
 *     n_itm / n_path (binomial).  The indicator is STRICT: a tie spot == K has payoff 0 and indicator 0.  By construction
 *     price = F delta + K dual_delta up to rounding.
 *   SENSITIVITY to parameter p: d = pay(x_up) - pay(x_dn) per path, each job recentred by its own M; KEEP RULE: a pair is kept iff
 *     both payoffs are not NaN; sens_p = DF mean_pairs(d) / (2 h_p); n_pairs is returned.  No kept pair is not an error: 0/0 = NaN
 *     and n_pairs says so.  ERROR: DF x population deviation over the pairs of dt / sqrt(n_path) / (2 h_p), dt = d - s (q_up
 *     (spot_up - F) - q_dn (spot_dn - F)), q_up / q_dn = n_itm / n_path of the up / dn job.  M_up and M_dn are sample means and a
 *     payoff moves by -s F 1{in the money} per unit of its M: dt is d with that delta-method term (its mean is 0 when every path
 *     is kept), without which the deviation of d misstates the error of the difference wherever paths end in the money -- an
 *     in-the-money call's several times over.
 * Left out: gamma (on this estimator a density estimate at the strike: the conditional estimator returns it, svmc_cmc_greeks_chain
 * above), SVMC_INV_CALL / SVMC_INV_PUT, variables other than the log-return, the inverse measure's payoffs, Hawkes, sharded sessions.
 *   svmc_greeks_payoff_chain   model-agnostic, on any device arrays: base_rows_host [n_expiries], up_rows_host / dn_rows_host
 *                              [n_params][n_expiries] HOST arrays of DEVICE pointers ([n_path] each); spot_sums: device
 *                              [1 + 2 n_params][n_expiries][2], the jobs in the order base, up_0, dn_0, up_1, ...; steps_host
 *                              [n_params] positive and finite.  greeks_host [SVMC_GREEKS_BASE_ROWS][K] = {delta, its error,
 *                              dual delta, its error, n_itm}, sens_host [n_params][SVMC_GREEKS_SENS_ROWS][K] = {sens, its error,
 *                              n_pairs} (counts as doubles; K = sum K_i).  One upload of the table, four launches on `stream`
 *                              (greeks_payoff_kernel: path blocks x groups of up to SVMC_GREEKS_KT strikes of one expiry, and
 *                              greeks_finish_kernel, over the 1 + 2 n_params jobs -- the deltas and every job's q; then the
 *                              same two over the n_params pairs), the downloads, one synchronize.  Every sum has a fixed
 *                              order that depends on n_path alone (path blocks: min(ceil(n_path / 256), 1024)): a quote's numbers
 *                              are the same bits whichever other strikes, expiries or bump pairs share the call.  `workspace`:
 *                              device memory of svmc_greeks_payoff_workspace_bytes(n_path, n_expiries, K, n_params).
 *   svmc_logsv_chain_price_greeks / svmc_heston_chain_price_greeks   the many-job stepping launch with the 1 + 2 n_params rows of
 *                              params_host (rows as svmc_*_chain_price_many: base, then up, dn per parameter; all on `seed` and
 *                              `call_id`), then the plain tail on job 0 and the tail above on the session's stream, the values
 *                              stored by the finish kernels in page-locked memory, ONE synchronize.  Session and workspace as
 *                              the many-job calls; later single calls are undisturbed.  sens_host may be NULL at n_params = 0.
 * Everything is checked before anything is launched: SVMC_ERR_INVALID_ARGUMENT for a null pointer, n_path < 1, n_expiries < 1 (the
 * fused calls: outside [1, 16]), n_params outside 0 .. SVMC_GREEKS_MAX_PARAMS, a step that is not positive and finite, a forward
 * that is not positive and finite, a discount factor or strike that is not finite, a sharded session; SVMC_ERR_UNKNOWN_PAYOFF for
 * a type code other than SVMC_CALL / SVMC_PUT; SVMC_ERR_WORKSPACE for a workspace (a session) too small. */
#define SVMC_GREEKS_KT 8
#define SVMC_GREEKS_MAX_PARAMS 31
#define SVMC_GREEKS_BASE_ROWS 5
#define SVMC_GREEKS_SENS_ROWS 3
SVMC_API int svmc_greeks_payoff_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, int n_params, size_t *bytes);
SVMC_API int svmc_greeks_payoff_chain(const double *const *base_rows_host, const double *const *up_rows_host,
                                      const double *const *dn_rows_host, size_t n_path, const double *forwards_host,
                                      const double *discfactors_host, int n_expiries, const double *strikes_host,
                                      const int8_t *types_host, const size_t *strike_offsets_host, int n_params,
                                      const double *steps_host, const double *spot_sums, double *greeks_host, double *sens_host,
                                      void *workspace, size_t workspace_bytes, svmc_stream_t stream);
SVMC_API int svmc_logsv_chain_price_greeks(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                           const double *discfactors_host, int n_expiries, const double *strikes_host,
                                           const int8_t *types_host, const size_t *strike_offsets_host, int n_params,
                                           const double *params_host, const double *steps_host, int is_spot_measure,
                                           int nb_steps_per_year, uint64_t seed, uint32_t call_id, double *prices_host,
                                           double *stderrs_host, double *greeks_host, double *sens_host);
SVMC_API int svmc_heston_chain_price_greeks(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                            const double *discfactors_host, int n_expiries, const double *strikes_host,
                                            const int8_t *types_host, const size_t *strike_offsets_host, int n_params,
                                            const double *params_host, const double *steps_host, int scheme, int nb_steps_per_year,
                                            uint64_t seed, uint32_t call_id, double *prices_host, double *stderrs_host,
                                            double *greeks_host, double *sens_host);

/* ---- conditional Monte Carlo: many jobs in one stepping launch, parameter sensitivities (src svmc_cmc.hip, svmc_chain.hip) ----
 * MANY JOBS.  svmc_logsv_chain_cmc_many / svmc_heston_chain_cmc_many step n_jobs independent conditional jobs of one step grid in ONE
 * launch (blockIdx.y = job): a path of job j starts from (mu, cv, vol, qvar) = (0, 0, vol0_j, 0) at step 0 of stream 8 of
 * (seeds_host[j], call_ids_host[j]) and expiry i goes to row j n_slices + i of mu_snapshots / cv_snapshots (device, caller-owned,
 * [n_jobs][n_slices][n_path]); nothing is written back.  params_host rows as svmc_*_chain_price_many ([n_jobs][6 + n_slices] /
 * [n_jobs][5]); every job has its own `joined` mask, by the rule of svmc_*_chain_cmc.  Row j n_slices + i is BIT-EQUAL to what
 * svmc_logsv_chain_cmc / svmc_heston_chain_cmc write for that job alone from a uniform start, in both launch forms (chosen by
 * n_jobs x n_path), whatever other jobs share the launch.  1 <= n_jobs <= SVMC_MANY_MAX_JOBS, 1 <= n_slices <= 16; `workspace`:
 * device memory of svmc_cmc_many_workspace_bytes(n_jobs, n_slices) for the job table; returns after the stream is synchronised.
 * svmc_logsv_chain_price_cmc_many / svmc_heston_chain_price_cmc_many: that launch on a session, then per job the tail of
 * svmc_cmc_payoff_chain on its rows: job j's prices_host / stderrs_host row ([n_jobs][sum K_i]) and stats_host block (nullable,
 * [n_jobs][n_expiries][SVMC_CMC_STATS_DOUBLES]) are those of svmc_*_chain_price_cmc with its parameters and stream, bit for bit.
 *
 * SENSITIVITIES.  The jobs are base, up_0, dn_0, up_1, ... as in the Greeks block above, on ONE (seed, call id) of stream 8 and
 * stepped by one launch.  Everything of the conditional estimator stands PER JOB j: the keep rule, e = exp(mu + cv / 2), c_j =
 * mean_kept_j(e) - 1 with recentring and 0 without, K'_j = K + F c_j, the degenerate cases.  B is the undiscounted per-path Black-76
 * price of the payoff block, B_k the per-path dual delta of the Greeks block.
 *   JOB PASS: every up and dn job gets its forward statistics as svmc_cmc_payoff_chain forms them (its own two kernels) and, per
 *     quote, q_j = mean_kept_j(B_k); q_j stays on the device.
 *   PAIR PASS, parameter p with step h_p: a pair (path i) is kept iff the path is kept in both jobs; d_i = B_i^up - B_i^dn;
 *     sens_p = DF mean_pairs(d) / (2 h_p); n_pairs is returned; no kept pair gives NaN with n_pairs = 0 and is not an error.
 *     ERROR: DF x population deviation over the pairs of dt / sqrt(n_path) / (2 h_p); with recentring dt_i = d_i + F (q_up (e_i^up
 *     - 1) - q_dn (e_i^dn - 1)), without it dt_i = d_i.  c_up and c_dn are sample means and a price moves by F B_k per unit of its
 *     own c: the extra term is the delta-method term of the two recentring means, without which the deviation of d misstates the
 *     error of the difference (an at-the-money put's several times over).
 *   The sums are taken of value_i - value_path0 (paths that agree to the bit give an error of exactly 0); where path 0 of the expiry
 *   is not a kept pair the shift is 0.  Every sum's order depends on n_path alone (path blocks min(ceil(n_path / 256), 1024), columns
 *   in row order): a quote's numbers are the same bits whichever strikes, expiries or pairs share the call.
 *   svmc_cmc_sens_chain   model-agnostic, on any device arrays: up_mu / up_cv / dn_mu / dn_cv [n_params][n_expiries] HOST arrays of
 *                         DEVICE pointers ([n_path] each); steps_host [n_params] positive and finite; sens_host
 *                         [n_params][SVMC_CMC_SENS_ROWS][K] = {sens, its error, n_pairs}.  One upload, six launches whatever
 *                         n_params (four without recentring: q is not read), one download, one synchronize.  `workspace`: device
 *                         memory of svmc_cmc_sens_workspace_bytes(n_path, n_expiries, K, n_params).  n_params in [1,
 *                         SVMC_GREEKS_MAX_PARAMS].
 *   svmc_logsv_chain_price_cmc_sens / svmc_heston_chain_price_cmc_sens   the fused drivers: arguments as svmc_*_chain_price_greeks
 *                         plus recenter; the 1 + 2 n_params rows of params_host on one stepping launch, the tail above on the bumped
 *                         jobs' rows, then svmc_cmc_greeks_chain's six launches on job 0's rows: greeks_host
 *                         [SVMC_CMC_GREEKS_ROWS][K] and stats_host (nullable) are bit-equal to svmc_*_chain_price_cmc_greeks at
 *                         the same seed.  Everything on the session's stream, ONE synchronize; the session grows a workspace of
 *                         its own on demand and later single calls are undisturbed.  sens_host may be NULL at n_params = 0.
 * Checked before anything is launched, status codes as the Greeks block above: a null pointer, counts out of range (the fused and
 * many-job calls: n_expiries outside [1, 16]), a step or forward that is not positive and finite, a strike or discount factor that
 * is not finite, a sharded session (SVMC_ERR_INVALID_ARGUMENT); a type other than SVMC_CALL / SVMC_PUT (SVMC_ERR_UNKNOWN_PAYOFF); a
 * workspace or session too small (SVMC_ERR_WORKSPACE).
 * Left out: SVMC_INV_CALL / SVMC_INV_PUT, variables other than the log-return, the inverse measure, Heston QE, Hawkes, sharded
 * sessions.  The conditional-MC calibration objective: the row f15 block below. */
#define SVMC_CMC_SENS_ROWS 3
SVMC_API int svmc_cmc_many_workspace_bytes(int n_jobs, int n_slices, size_t *bytes);
SVMC_API int svmc_logsv_chain_cmc_many(size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
                                       const double *params_host, int is_spot_measure, const uint64_t *seeds_host,
                                       const uint32_t *call_ids_host, uint64_t path_offset, double *mu_snapshots,
                                       double *cv_snapshots, void *workspace, size_t workspace_bytes, svmc_stream_t stream);
SVMC_API int svmc_heston_chain_cmc_many(size_t n_path, int n_jobs, int n_slices, const int *nb_steps_host, const double *dts_host,
                                        const double *params_host, const uint64_t *seeds_host, const uint32_t *call_ids_host,
                                        uint64_t path_offset, double *mu_snapshots, double *cv_snapshots, void *workspace,
                                        size_t workspace_bytes, svmc_stream_t stream);
SVMC_API int svmc_cmc_sens_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, int n_params, size_t *bytes);
SVMC_API int svmc_cmc_sens_chain(const double *const *up_mu_host, const double *const *up_cv_host, const double *const *dn_mu_host,
                                 const double *const *dn_cv_host, size_t n_path, const double *forwards_host,
                                 const double *discfactors_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                 const size_t *strike_offsets_host, int n_params, const double *steps_host, int recenter,
                                 double *sens_host, void *workspace, size_t workspace_bytes, svmc_stream_t stream);
SVMC_API int svmc_logsv_chain_price_cmc_many(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                             const double *discfactors_host, int n_expiries, const double *strikes_host,
                                             const int8_t *types_host, const size_t *strike_offsets_host, int n_jobs,
                                             const double *params_host, const uint64_t *seeds_host, const uint32_t *call_ids_host,
                                             int is_spot_measure, int nb_steps_per_year, int recenter, double *prices_host,
                                             double *stderrs_host, double *stats_host);
SVMC_API int svmc_heston_chain_price_cmc_many(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                              const double *discfactors_host, int n_expiries, const double *strikes_host,
                                              const int8_t *types_host, const size_t *strike_offsets_host, int n_jobs,
                                              const double *params_host, const uint64_t *seeds_host, const uint32_t *call_ids_host,
                                              int nb_steps_per_year, int recenter, double *prices_host, double *stderrs_host,
                                              double *stats_host);
SVMC_API int svmc_logsv_chain_price_cmc_sens(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                             const double *discfactors_host, int n_expiries, const double *strikes_host,
                                             const int8_t *types_host, const size_t *strike_offsets_host, int n_params,
                                             const double *params_host, const double *steps_host, int is_spot_measure,
                                             int nb_steps_per_year, int recenter, uint64_t seed, uint32_t call_id,
                                             double *greeks_host, double *stats_host, double *sens_host);
SVMC_API int svmc_heston_chain_price_cmc_sens(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                              const double *discfactors_host, int n_expiries, const double *strikes_host,
                                              const int8_t *types_host, const size_t *strike_offsets_host, int n_params,
                                              const double *params_host, const double *steps_host, int nb_steps_per_year,
                                              int recenter, uint64_t seed, uint32_t call_id, double *greeks_host,
                                              double *stats_host, double *sens_host);

/* ---- conditional Monte Carlo: the calibration objective on one replayed graph (src svmc_chain.hip, svmc_cmc.hip) ----
 * svmc_logsv_chain_price_cmc_sets / svmc_heston_chain_price_cmc_sets price one chain for n_sets parameter sets on ONE (seed, call_id)
 * of stream 8 and return, per set, prices, errors, forward statistics and Black-76 implied vols: what an optimizer iterate of a
 * calibration on a frozen stream needs -- its base point (one set) or the bumped neighbours of a forward-difference gradient.
 * params_host rows as svmc_*_chain_price_cmc_many ([n_sets][6 + n_expiries]: v0 theta kappa1 kappa2 beta volvol, then the expiries'
 * vol-backbone etas / [n_sets][5]: v0 theta kappa rho volvol); 1 <= n_sets <= SVMC_CMC_SETS_MAX.  Outputs [n_sets][sum K_i];
 * stats_host (nullable) [n_sets][n_expiries][SVMC_CMC_STATS_DOUBLES]; ivols_host (nullable) [n_sets][sum K_i].
 * CONTRACT.  Set q's prices, errors and statistics are those of svmc_*_chain_price_cmc(seed, call_id) with set q's parameters, BIT
 * FOR BIT, in both launch forms of the stepping kernel (chosen by n_sets x n_path).  Its vols are the library's Black-76 inversion
 * (svmc_black_implied_vols' routine, compiled for the device) of those prices on [1e-6, 10]: NaN outside the bracket, for a NaN
 * price and for K <= 0.  A set's numbers do not depend on which other sets share the call.
 * ONE EVALUATION IS ONE GRAPH REPLAY: a linear chain of nodes, no parallel branches -- (1) the upload of the job table, filled in
 * page-locked memory, so that a replay re-prices the chain for new parameters without a new capture; (2) the many-job stepping launch
 * of the row f14 block, whose arguments do not depend on the parameters; (3) the payoff tail ONCE for all sets, which are laid out as
 * one table of n_sets x n_expiries expiries and n_sets x sum K_i strikes, set-major, as row f14 lays out its bumped jobs: the forward,
 * forward-finish and payoff kernels of svmc_cmc_payoff_chain with a single call's statements; (4) cond_vols_finish_kernel, a block
 * per (set, quote): the two column sums in row order, price and error stored straight into the session's page-locked result block
 * with the statistics; (5) with ivols_host, cond_vols_invert_kernel, a lane per quote and 64 quotes side by side in a wave, which
 * stores the vols there too.  No copy node.  The table's image (expiry records with the snapshot rows' addresses, strike groups,
 * columns) depends on the chain and the buffers alone and is uploaded once per capture, outside the graph, into a workspace no other
 * call writes.  The session keeps one graph per n_sets; its key covers the chain's content, the model, n_sets, is_spot_measure, the
 * step grid, recenter, seed, call_id, whether vols are asked for and the address of every device and page-locked buffer the graph
 * captured.  The stepping buffers are shared with the row f14 calls: a call that regrows one drops the graphs that captured it.
 * svmc_session_use_graphs(s, 0) issues the same launches directly (the same bits); svmc_session_graph_launches counts the replays.
 * Checks and status codes are those of svmc_*_chain_price_cmc_many (1 to 16 expiries, an unsharded session, SVMC_CALL / SVMC_PUT, ...),
 * made before anything is launched; n_sets out of range: SVMC_ERR_INVALID_ARGUMENT.
 * Left out: a stepping kernel that shares the draw across sets (the conditional step consumes a quarter of a Philox call where the
 * plain step consumes two normals, so the share that made the plain sets kernel worth building is small here, and the many-job
 * kernel keeps the bit-equality for free); the objective summed on the device; SVMC_INV_CALL / SVMC_INV_PUT, variables other than the
 * log-return, the inverse measure, Heston QE, Hawkes, several GPUs. */
#define SVMC_CMC_SETS_MAX 8
SVMC_API int svmc_logsv_chain_price_cmc_sets(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                             const double *discfactors_host, int n_expiries, const double *strikes_host,
                                             const int8_t *types_host, const size_t *strike_offsets_host, int n_sets,
                                             const double *params_host, int is_spot_measure, int nb_steps_per_year, int recenter,
                                             uint64_t seed, uint32_t call_id, double *prices_host, double *stderrs_host,
                                             double *stats_host, double *ivols_host);
SVMC_API int svmc_heston_chain_price_cmc_sets(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                              const double *discfactors_host, int n_expiries, const double *strikes_host,
                                              const int8_t *types_host, const size_t *strike_offsets_host, int n_sets,
                                              const double *params_host, int nb_steps_per_year, int recenter, uint64_t seed,
                                              uint32_t call_id, double *prices_host, double *stderrs_host, double *stats_host,
                                              double *ivols_host);

/* ---- conditional Monte Carlo for the Hawkes jump-diffusion (src svmc_hawkes.hip, svmc_chain.hip) ----
 * The diffusion sigma w0 of the step of svmc_hawkesjd_terminal_rng has a constant sigma and is independent of both jump processes
 * and both intensities.  Given a path's jumps its discretised log-return is therefore exactly Gaussian,
 *   x_T | jumps ~ N(mu, cv),   mu = sum_t ((mu_drift - sigma^2 / 2) dt - comp_p dt lambda_p,t - comp_m dt lambda_m,t + J_P,t + J_M,t),
 *   cv = sigma^2 T -- ONE number for every path,
 * and integrating w0 out leaves a Black-76 price per path: the plain pricer's expectation for the same discretised model and a smaller
 * variance.  A path carries (mu, lambda_p, lambda_m); the stepping draws no normal; svmc_cmc_payoff_chain and svmc_cmc_greeks_chain
 * (rows f11, f13) serve unchanged on (mu, cv).
 *
 * STEPPING.  svmc_hawkesjd_chain_cond advances the caller's device state (mu, lambda_p, lambda_m), [n_path] each, through n_slices
 * slices (any number: launches of 16) of nb_steps_host[i] steps of dts_host[i], by the statements of svmc_hawkesjd_terminal_rng's step
 * without the normal: the jump tests on the intensities at the start of the step (1 - u < lambda dt screens the fp64 -ln u <
 * lambda dt), drift = (drift dt - comp_p dt lambda_p) - comp_m dt lambda_m, mu = ((mu + drift) + jump_p) + jump_m, the two
 * intensity statements with no floor; no product is fused into a sum.  Row i of mu_snapshots ([n_slices][n_path], device, nullable)
 * is mu at the end of slice i; row i of cv_snapshots (the same, nullable) holds cv_i on every path; cvs_host ([n_slices], host,
 * nullable) receives the cv_i.  The terminal state is written back.
 * Randoms: stream 9 of (seed, call_id) carries the jump uniforms, ONE call per TWO steps -- chain-global step s = step_offset +
 * local step reads words 2 (s & 1) and 2 (s & 1) + 1 of the call at index s >> 1 as u_p, u_m = (r + 1/2) 2^-32; stream 10's call at
 * index s, drawn only on a step where a side jumps, gives E_p, E_m from its words 0 and 1 as stream 7's.  Both are independent of
 * the plain pricer's streams 6 and 7 at equal (seed, call_id); streams 0 .. 8 are untouched: the stream version stays 4.
 * VARIANCE.  cv_i = cv_(i-1) + nb_steps_i (sigma sigma dt_i), formed on the host in double in slice order from cv_(-1) = cv_start,
 * each product and sum rounded once; the kernel does no variance arithmetic.
 * CONTINUATION.  A chain cut into several calls -- each with step_offset = the steps taken so far and cv_start = the last cv of
 * the call before -- gives the bits of the unbroken call, also where a cut falls between the two steps of one stream-9 call;
 * path_offset shards a job by the global path index the same way.
 * Refusals (SVMC_ERR_INVALID_ARGUMENT, before any launch): those of svmc_hawkesjd_terminal_rng (the parameter block, a null state
 * array, n_path = 0, a negative step count, a dt that is not positive and finite, call_id past 24 bits), no slices or null grids,
 * cv_start negative or not finite.
 *
 * FUSED.  svmc_hawkesjd_chain_price_cmc / svmc_hawkesjd_chain_price_cmc_greeks: the stepping from (0, lambda_p, lambda_m) on the
 * session's own state (x holds mu, its two other arrays lambda_p and lambda_m afterwards) on the step grid of
 * svmc_hawkesjd_chain_price, then the tail of svmc_cmc_payoff_chain / svmc_cmc_greeks_chain; arguments, outputs, refusals and status
 * codes as svmc_heston_chain_price_cmc / svmc_heston_chain_price_cmc_greeks with params_host for the model (its checks are made
 * first).  Bit-equal to svmc_hawkesjd_chain_cond followed by the tail entry on its rows.
 * Left out, each a later step: many-job and few-waves stepping forms, parameter sensitivities, SVMC_INV_CALL / SVMC_INV_PUT,
 * variables other than the log-return, several GPUs.  The estimator under the risk-premia kernel is DESIGN.md row f17 (svmc_ext.h);
 * many (sigma, gamma) sets on ONE stepping call at sigma = 0 and a calibration objective on them are row f20 (svmc_est.h,
 * svmc_jump_sets_payoff_chain). */
SVMC_API int svmc_hawkesjd_chain_cond(double *mu, double *lambda_p, double *lambda_m, size_t n_path, int n_slices,
                                      const int *nb_steps_host, const double *dts_host, const double *params_host, double cv_start,
                                      uint64_t seed, uint32_t call_id, uint64_t path_offset, uint32_t step_offset,
                                      double *mu_snapshots, double *cv_snapshots, double *cvs_host, svmc_stream_t stream);
SVMC_API int svmc_hawkesjd_chain_price_cmc(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                           const double *discfactors_host, int n_expiries, const double *strikes_host,
                                           const int8_t *types_host, const size_t *strike_offsets_host, const double *params_host,
                                           int nb_steps_per_year, int recenter, uint64_t seed, uint32_t call_id, double *prices_host,
                                           double *stderrs_host, double *stats_host);
SVMC_API int svmc_hawkesjd_chain_price_cmc_greeks(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                                  const double *discfactors_host, int n_expiries, const double *strikes_host,
                                                  const int8_t *types_host, const size_t *strike_offsets_host,
                                                  const double *params_host, int nb_steps_per_year, int recenter, uint64_t seed,
                                                  uint32_t call_id, double *greeks_host, double *stats_host);

#ifdef __cplusplus
}
#endif
#endif /* SVMC_H */
