/*
 * svmc_est.h -- C ABI of libsvmc_est.so, "estimators beside the core": the OPEN library of model-agnostic estimators on
 * caller-owned device arrays.
 *
 * libsvmc.so (svmc.h) is closed at 143 entry points and at its kernels; libsvmc_ext.so (svmc_ext.h) is closed at three exported
 * symbols and four kernels: existing tests pin each by count and by name.  This library is where the next estimator goes, so that
 * no fourth library is ever needed.  THE RULE that keeps it open:
 *   - it is one translation unit (stochvolmodels_amd/csrc/svmc_est.hip) on the header-only parts of csrc/ and links nothing from
 *     libsvmc.so or libsvmc_ext.so: no undefined svmc_ symbol;
 *   - its tests compare its exports and its Python binding TO WHAT THIS HEADER DECLARES (every SVMC_EST_API line), never to a
 *     literal list or a count, and ask of EVERY kernel in its metadata scratch_bytes == 0 without pinning how many kernels there
 *     are.  A new entry point is a declaration here, a definition in svmc_est.hip and a line in _lib._declare_est; a new kernel
 *     needs no test to change.
 * svmc.h is included for the status codes, svmc_stream_t, SVMC_CALL / SVMC_PUT and SVMC_TILTED_MAX_GAMMAS.
 *
 * Conventions: svmc.h's.  Every function returns an svmc status code; this library keeps no error message (svmc_last_error
 * belongs to the core), the refusals below say what each code means.  Device pointers are on the current HIP device.
 */
#ifndef SVMC_EST_H
#define SVMC_EST_H

#include "svmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVMC_EST_VERSION 100 /* 0.1.0 */

#if defined(__GNUC__) || defined(__clang__)
#define SVMC_EST_API __attribute__((visibility("default")))
#else
#define SVMC_EST_API
#endif

SVMC_EST_API int svmc_est_version(void);

/* ---- conditional Monte Carlo Greeks under the exponential risk-premia kernel (src svmc_est.hip) ----------
 * The derivatives in the forward and in the strike of svmc_tilted_cond_payoff_chain's price (svmc_ext.h, row f17), in closed form
 * per path.  Notation, inputs, keep rule and recentring are that entry's: device rows mu[j], cv[j], the forward F, strikes K_k of
 * type 'C' / 'P', up to SVMC_TILTED_MAX_GAMMAS gammas;
 *   W_j = exp(gamma mu_j + gamma^2 cv_j / 2),   e_t,j = exp(mu_j + (gamma + 1/2) cv_j),   F_t,j = F e_t,j;
 *   a path is kept iff f11's rule holds and W_j^2 and (W_j F_t,j)^2 are finite; a dropped path adds nothing to any sum;
 *   c = mean_kept_f11(exp(mu + cv / 2)) - 1 with recenter != 0 -- f11's UNWEIGHTED mean over the paths f11 keeps, the same bits as
 *   svmc_tilted_cond_payoff_chain's and svmc_cmc_payoff_chain's corr / F on these rows, whatever gamma is -- and 0 without;
 *   corr = F c, K' = K + corr.  The weight depends on neither F nor K and c on neither, so what follows are the EXACT derivatives of
 *   the price that entry returns on the same rows.
 * Per kept path, s = +1 call / -1 put, sd = sqrt(cv):
 *   d1 = (ln F_t - ln K') / sd + sd / 2,  d2 = d1 - sd
 *   B_f = N(d1) (call) | N(d1) - 1 (put),   B_k = -N(d2) (call) | N(-d2) (put)
 *   delta_j = e_t B_f + c B_k,   dual_delta_j = B_k,   dual_gamma_j = phi(d2) / (K' sd)
 *   DEGENERATE (row f13's): cv == 0: B_f = s 1{s (F_t - K') > 0} (strict), B_k = -B_f, dual_gamma_j = 0, and the path is counted
 *   per (expiry, gamma) as n_zero_cv;  K' <= 0: call B_f = 1, B_k = -1, put both 0, dual_gamma_j = 0.
 *   value = sum_j W_j v_j / sum_j W_j,   error = sqrt(sum_j (W_j (v_j - value))^2) / sum_j W_j
 *   gamma = (K / F)^2 dual_gamma, value and error scaled once per quote.
 * The error comes from the sums of W d, (W d)^2 and W^2 d with d = v - shift, exactly as row f17 forms a price's error; the shifts
 * are host constants per quote: s 1{s (F - K) > 0} for delta, its negative for dual delta, 0 for dual gamma.  One kept path gives
 * error 0.  No kept path, or kept paths of zero weight only, give NaN values and are NOT errors of the call.  The errors ignore
 * the noise of c, as f13's and f17's do.  All values are undiscounted.  An error is a difference of those sums: it keeps its digits where
 * the values lie near their shift and loses them as sum (W d)^2 exceeds sum (W (v - value))^2 -- a handful of paths that all lie across the
 * strike from the forward, or one dominating weight.
 * Every sum has a fixed order that depends on n_path alone: a gamma's, an expiry's and a strike's results are the same bits
 * whichever others share the call.  No atomics, no scratch, LDS for the block sums' exchange only.
 *
 * Two consequences, to rounding:
 *   HOMOGENEITY  price = F delta + K dual_delta with svmc_tilted_cond_payoff_chain's price; at one strike
 *                delta_C - delta_P = gamma_forward / F and dual_delta_C - dual_delta_P = -1 with its gamma_forward;
 *   THE DENSITY  with recenter = 0 and K = F exp(x):  K dual_gamma = sum_j W_j N(x; mu_j + gamma cv_j, cv_j) / sum_j W_j, the
 *                density of the simulated log-return under the kernel without a bandwidth, normalised by the weights: it
 *                integrates to the weight share of the kept paths with cv > 0.  Because
 *                W_j N(x; mu_j + gamma cv_j, cv_j) = e^{gamma x} N(x; mu_j, cv_j), the quantity pdf_gamma(x) sum W_gamma / e^{gamma x}
 *                is the same number for every gamma when no path is dropped.
 *
 * Price and error are NOT recomputed here: they are svmc_tilted_cond_payoff_chain's on the same rows.  A C caller makes two calls
 * (the Python routes call both tails).
 *
 *   svmc_tilted_cond_greeks_workspace_bytes   host only: the device workspace that serves any chain of n_expiries expiries and
 *                              total_strikes strikes at this n_path and n_gammas.
 *   svmc_tilted_cond_greeks_chain     mu_snapshots_host, cv_snapshots_host: HOST arrays of n_expiries DEVICE pointers; strikes /
 *                              types concatenated, expiry i owning [strike_offsets_host[i], strike_offsets_host[i + 1]).
 *                              greeks_host: [n_gammas][SVMC_TCG_ROWS][sum K_i] -- delta, its error, dual delta, its error, gamma,
 *                              its error, dual gamma, its error; stats_host: [n_gammas][n_expiries][SVMC_TCG_STATS_DOUBLES] --
 *                              sum W, n_kept, n_dropped, n_zero_cv; host arrays.  One upload of the chain's table, four launches
 *                              on `stream` with no host round trip between them (the forward pass and its finish with the
 *                              statements of rows f11 / f17, the Greeks kernel, the finish), one download, one synchronise.
 * Everything is checked before anything is launched, and a refused call leaves the output arrays untouched:
 * SVMC_ERR_INVALID_ARGUMENT for a null pointer (a null snapshot among them), n_path < 1, n_expiries < 1, n_gammas outside
 * 1 .. SVMC_TILTED_MAX_GAMMAS, strike offsets that do not start at 0 or decrease, a gamma, forward or strike that is not finite, a
 * forward that is not positive; SVMC_ERR_UNKNOWN_PAYOFF for a type code other than SVMC_CALL / SVMC_PUT; SVMC_ERR_WORKSPACE for a
 * workspace below svmc_tilted_cond_greeks_workspace_bytes; SVMC_ERR_HIP for a failure of the runtime.
 * Left out: the many-job form (different jump parameters per job), parameter sensitivities, IC / IP, several GPUs.  Many
 * (sigma, gamma) sets on one set of rows and the calibration objective on them: svmc_jump_sets_payoff_chain below (row f20), prices
 * only. */
#define SVMC_TCG_ROWS 8
#define SVMC_TCG_STATS_DOUBLES 4

SVMC_EST_API int svmc_tilted_cond_greeks_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, int n_gammas,
                                                         size_t *bytes);
SVMC_EST_API int svmc_tilted_cond_greeks_chain(const double *const *mu_snapshots_host, const double *const *cv_snapshots_host,
                                               size_t n_path, const double *forwards_host, int n_expiries,
                                               const double *strikes_host, const int8_t *types_host,
                                               const size_t *strike_offsets_host, const double *gammas_host, int n_gammas,
                                               int recenter, double *greeks_host, double *stats_host, void *workspace,
                                               size_t workspace_bytes, svmc_stream_t stream);

/* ---- the mixture density of the simulated log-return, under the kernel or not (src svmc_est.hip) -----------
 * THE DENSITY above as an estimator of its own: the "dedicated density kernel on the e^{gamma x} identity" of row f18's list.
 * Model-agnostic: any generator's per-path conditional mean mu[j] and variance cv[j] of the log-return.
 * Inputs: device rows mu[j], cv[j] per expiry; points x_p per expiry, concatenated, expiry i owning [point_offsets_host[i],
 * point_offsets_host[i + 1]) as strikes are laid out above; up to SVMC_TILTED_MAX_GAMMAS gammas.
 * Which paths count: a path passes iff f11's rule holds (mu, cv and exp(mu + cv / 2) finite, cv >= 0: the statement the Greeks
 * above share).  A passing path with cv == 0 is a point mass: it adds nothing to any x-sum, it is counted (n_zero_cv) and its
 * weight still enters sum W, as above.
 * Gamma-independent sums over the f11-kept paths with cv > 0, with n_jp = N(x_p; mu_j, cv_j) = exp(-z^2 / 2) / (sd_j sqrt(2 pi)),
 * z = (x_p - mu_j) / sd_j:
 *   S1_p = sum_j n_jp,   S2_p = sum_j n_jp^2                                   ONE exp per (path, point)
 * Per gamma, W_gj = exp(gamma mu_j + gamma^2 cv_j / 2):
 *   per (expiry, gamma): sum W, sum W^2 over the f11-kept paths whose W^2 is finite, and n_weight_dropped, the count of f11-kept
 *   paths whose W^2 is not;   per (point, gamma): C_pg = sum_j W_gj n_jp       one FMA, no transcendental
 * Results:
 *   pdf_g(x_p) = e^{gamma x_p} S1_p / sum W_g
 *   error      = sqrt(max(e^{2 gamma x_p} S2_p - 2 pdf e^{gamma x_p} C_pg + pdf^2 sum W_g^2, 0)) / sum W_g
 * Because W_j N(x; mu_j + gamma cv_j, cv_j) = e^{gamma x} N(x; mu_j, cv_j), pdf_g is the Greeks entry's K dual_gamma at K = exp(x),
 * F = 1, recenter = 0, and the error is its ratio-estimator error sqrt(sum_j (W_j (v_j - pdf))^2) / sum W, term for term (v_j the
 * path's Gaussian under the kernel: W_j v_j = e^{gamma x} n_jp).  One kept path gives error 0.  gamma = 0 has W = 1 and
 * e^{gamma x} = 1; 0 times anything is never formed.  pdf_g integrates to the weight share of the kept paths with cv > 0; it is not
 * normalised further.  No kept path gives NaN and is NOT an error of the call.
 * TWO DELIBERATE DIFFERENCES from the Greeks entry's keep rule:
 *   - that entry drops a path PER GAMMA when W^2 or (W F_t)^2 overflows and re-sums without it.  Here S1 and S2 are shared by all
 *     gammas, so a gamma with n_weight_dropped > 0 returns NaN for its pdf and its error and its statistics row says how many
 *     paths failed; the other gammas of the call are untouched, and the call is not refused.  The Greeks entry still serves such
 *     a gamma;
 *   - (W F_t)^2 is not part of the rule: no forward enters a density.
 * Statistics per (gamma, expiry): sum W, n_kept (f11's), n_dropped = n_path - n_kept, n_zero_cv, n_weight_dropped.
 * Every sum has a fixed order that depends on n_path alone: a gamma's, an expiry's and a point's results are the same bits
 * whichever others share the call; sum W, n_kept and n_zero_cv are the Greeks entry's bits on rows where it drops no weight.  No
 * atomics, no scratch, LDS for the block sums' exchange only.
 *
 *   svmc_cond_density_workspace_bytes   host only: the device workspace that serves any call of n_expiries expiries and
 *                              total_points points at this n_path and n_gammas (it holds a row of weights per (expiry, gamma)).
 *   svmc_cond_density_chain    mu_snapshots_host, cv_snapshots_host: HOST arrays of n_expiries DEVICE pointers.  pdf_host,
 *                              stderr_host: [n_gammas][sum P_i]; stats_host: [n_gammas][n_expiries][SVMC_CD_STATS_DOUBLES]; host
 *                              arrays.  One upload of the call's table, three launches on `stream` with no host round trip between
 *                              them (the weights with the statistics' sums, the Gaussians, the finish), one download, one
 *                              synchronise.  An expiry without points is legal: its statistics are still returned.
 * Everything is checked before anything is launched, and a refused call leaves the output arrays untouched:
 * SVMC_ERR_INVALID_ARGUMENT for a null pointer (a null snapshot among them), n_path < 1, n_expiries < 1, n_gammas outside
 * 1 .. SVMC_TILTED_MAX_GAMMAS, point offsets that do not start at 0 or decrease, a gamma or point that is not finite;
 * SVMC_ERR_WORKSPACE for a workspace below svmc_cond_density_workspace_bytes; SVMC_ERR_HIP for a failure of the runtime.
 * Left out: the many-job form, several GPUs, a derivative of the density (many (sigma, gamma) sets on one set of rows: row f20 below,
 * prices only). */
#define SVMC_CD_STATS_DOUBLES 5

SVMC_EST_API int svmc_cond_density_workspace_bytes(size_t n_path, int n_expiries, size_t total_points, int n_gammas, size_t *bytes);
SVMC_EST_API int svmc_cond_density_chain(const double *const *mu_snapshots_host, const double *const *cv_snapshots_host,
                                         size_t n_path, int n_expiries, const double *points_host,
                                         const size_t *point_offsets_host, const double *gammas_host, int n_gammas,
                                         double *pdf_host, double *stderr_host, double *stats_host, void *workspace,
                                         size_t workspace_bytes, svmc_stream_t stream);

/* ---- many (sigma, gamma) sets on ONE set of jump rows (src svmc_est.hip) ---------------------------------------
 * For a model whose conditional law of the log-return is N(a_j - v / 2, v) with v the SAME on every path -- the Hawkes
 * jump-diffusion: svmc_hawkesjd_chain_cond at sigma = 0 leaves a_j (drift, compensators, jumps), which depends on neither sigma nor
 * gamma, and v = cv_i(sigma) is one host number per expiry -- the estimator of svmc_tilted_cond_payoff_chain (svmc_ext.h, row f17)
 * on the rows (a - v / 2, v), for up to SVMC_JUMP_SETS_MAX sets (gamma_q, v_qi) from one pass over the rows.  Model-agnostic: any
 * rows a[j] serve.
 * Inputs: per expiry i a device row a[j] [n_path], the forward F_i, strikes K_k of type SVMC_CALL / SVMC_PUT; per set q a gamma g_q
 * and per (set, expiry) a variance v_qi >= 0.
 * Per path and set:
 *   e_j = exp(a_j),   w_qj = exp(g_q a_j),   c_qi = exp(g_q (g_q - 1) v_qi / 2),   W_qj = c_qi w_qj,
 *   F_t = (F_i exp(g_q v_qi)) e_j,   ln F_t = (ln F_i + g_q v_qi) + a_j.
 * c_qi, F_i exp(g_q v_qi), ln F_i + g_q v_qi, sd = sqrt(v_qi) and 1 / sd are host constants per (set, expiry); c_qi is the same on
 * every path, cancels in every price and is applied once in the finish.  Per path that leaves one exp(a) and one exp(g a), per
 * strike one Black-76 price: no sqrt, no division and one 8-byte load per path.
 * Keep rule (row f17's on the rows (a - v / 2, v), restated): a_j and e_j finite -- f11's rule through tc_keep_cmc(a, 0) of
 * csrc/svmc_tilted_cond.h -- and W^2 and (W F_t)^2 finite.  A dropped path adds nothing to any sum and is counted.
 * Recentring: with recenter != 0, corr_i = F_i mean over the f11-kept paths of (e_j - 1), else 0: ONE forward pass per expiry for
 * all sets, bit-equal to the corr that svmc_cmc_payoff_chain and svmc_tilted_cond_payoff_chain form on the rows (a, 0) (the forward
 * pass has their statements and order).  K' = K + corr; ln K' once per strike.
 * Price and error: B_qjk = Black-76 of F_t against K' at total variance v (tc_black, its degenerate cases included: v == 0 gives the
 * intrinsic value at F_t; K' <= 0 gives F_t - K' for a call and 0 for a put);
 *   price_qk = sum_j w B / sum_j w,   stderr_qk = sqrt(sum_j (w (B - price))^2) / sum_j w,
 * from the sums of w d, (w d)^2, w^2 d with d = B - shift_k, exactly as row f17 forms them; the shifts are one host constant per
 * strike, shared by the sets (any finite value gives the same estimate).
 * Statistics per (set, expiry): row f17's block of SVMC_TILTED_STATS_DOUBLES with its meanings in terms of W = c w -- normalizer
 * n_kept / sum W, its error, gamma forward F + sum W (F_t - corr - F) / sum W, its error, effective sample size, n_kept, n_dropped,
 * sum W -- and corr_i per expiry.  No kept path, or kept paths of zero weight only, give NaN and are NOT an error of the call.  All
 * values are undiscounted.
 * Every sum has a fixed order that depends on n_path alone: a set's, an expiry's and a strike's results are the same bits whichever
 * others share the call.  No atomics, no scratch, LDS for the block sums' exchange only.
 *
 *   svmc_jump_sets_workspace_bytes   host only: the device workspace that serves any chain of n_expiries expiries and
 *                              total_strikes strikes at this n_path and n_sets.
 *   svmc_jump_sets_payoff_chain   a_snapshots_host: a HOST array of n_expiries DEVICE pointers; strikes / types / shifts
 *                              concatenated, expiry i owning [strike_offsets_host[i], strike_offsets_host[i + 1]);
 *                              variances_host [n_sets][n_expiries], gammas_host [n_sets].  prices_host, stderrs_host:
 *                              [n_sets][sum K_i]; stats_host: [n_sets][n_expiries][SVMC_TILTED_STATS_DOUBLES]; corr_host:
 *                              [n_expiries]; host arrays.  One upload of the call's table, four launches on `stream` with no host
 *                              round trip between them (the forward pass and its finish, the payoff kernel, the finish), one
 *                              download, one synchronise.
 * Everything is checked before anything is launched, and a refused call leaves the output arrays untouched: the status codes of
 * svmc_tilted_cond_greeks_chain above (shifts must be finite as strikes must), and SVMC_ERR_INVALID_ARGUMENT for n_sets outside
 * 1 .. SVMC_JUMP_SETS_MAX and for a variance that is negative or not finite.
 * Left out: the many-JOB form (different jump parameters per job), parameter sensitivities, IC / IP, several GPUs. */
#define SVMC_JUMP_SETS_MAX 16

SVMC_EST_API int svmc_jump_sets_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, int n_sets, size_t *bytes);
SVMC_EST_API int svmc_jump_sets_payoff_chain(const double *const *a_snapshots_host, size_t n_path, const double *forwards_host,
                                             int n_expiries, const double *strikes_host, const int8_t *types_host,
                                             const double *shifts_host, const size_t *strike_offsets_host,
                                             const double *variances_host, const double *gammas_host, int n_sets, int recenter,
                                             double *prices_host, double *stderrs_host, double *stats_host, double *corr_host,
                                             void *workspace, size_t workspace_bytes, svmc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SVMC_EST_H */
