/*
 * svmc_ext.h -- C ABI of libsvmc_ext.so, the model-agnostic estimators that live BESIDE libsvmc.so.
 *
 * libsvmc.so is the closed core: its ABI is held at the 143 entry points of svmc.h and its kernels are pinned by name and
 * count.  Estimators on caller-owned device arrays that need no session of the core are added here: one translation unit
 * (stochvolmodels_amd/csrc/svmc_ext.hip) that includes the header-only parts of csrc/ and links nothing from libsvmc.so.
 * svmc.h is included for the status codes, svmc_stream_t, SVMC_CALL / SVMC_PUT and SVMC_TILTED_MAX_GAMMAS.
 *
 * Conventions: svmc.h's.  Every function returns an svmc status code; this library keeps no error message (svmc_last_error
 * belongs to the core), the refusals below say what each code means.  Device pointers are on the current HIP device.
 */
#ifndef SVMC_EXT_H
#define SVMC_EXT_H

#include "svmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVMC_EXT_VERSION 100 /* 0.1.0 */

#if defined(__GNUC__) || defined(__clang__)
#define SVMC_EXT_API __attribute__((visibility("default")))
#else
#define SVMC_EXT_API
#endif

SVMC_EXT_API int svmc_ext_version(void);

/* ---- conditional Monte Carlo under the exponential risk-premia kernel (src svmc_ext.hip) ----------------
 * Rows f8 and f11 of svmc.h joined in closed form.  Given a path's conditioning variables the log-return is Gaussian,
 * x ~ N(mu, cv), and the Esscher identity E[e^{gamma x} g(x)] = e^{gamma mu + gamma^2 cv / 2} E[g(y)], y ~ N(mu + gamma cv, cv),
 * turns f8's weighted payoff of a path into a weight with no diffusion noise in it times a Black-76 price at a shifted forward.
 *
 * For one expiry the inputs are device rows mu[j], cv[j] ([n_path]; any model's, cv may differ per path), the forward F, strikes
 * K_k of type 'C' / 'P', one risk-premia gamma and a host constant shift_k per strike:
 *   W_j = exp(gamma mu_j + gamma^2 cv_j / 2),   F_t,j = F exp(mu_j + (gamma + 1/2) cv_j);
 *   KEEP RULE: path j is kept iff f11's rule holds -- mu_j, cv_j and e_j = exp(mu_j + cv_j / 2) finite and cv_j >= 0 -- and W_j^2
 *   and (W_j F_t,j)^2 are finite.  A dropped path adds nothing to any sum and is counted; every sum below runs over the kept paths;
 *   RECENTRING: corr = mean(F e) - F with recenter != 0, f11's UNWEIGHTED conditional mean over the paths f11 keeps (the weight
 *   takes no part in it): it is svmc_cmc_payoff_chain's corr on the same rows, bit for bit, whatever gamma is.  corr = 0
 *   otherwise.  K'_k = K_k + corr;
 *   B_jk = the undiscounted Black-76 price of F_t,j against K'_k at total variance cv_j, the call's formula for a call and the
 *   put's for a put, with ln F_t = ln F + mu + (gamma + 1/2) cv and ln K' formed once per strike.  Degenerate cases as f11's:
 *   cv_j == 0 gives the intrinsic value, K'_k <= 0 gives F_t,j - K'_k for a call and 0 for a put;
 *   price_k = sum_j W_j B_jk / sum_j W_j  (undiscounted, as f8's);
 *   stderr_k = sqrt(sum_j (W_j (B_jk - price_k))^2) / sum_j W_j, formed from the sums of W d, (W d)^2 and W^2 d with
 *   d = B - shift_k as f8 forms it (any finite shift gives the same estimate; one near the price keeps its error free of
 *   cancellation).
 * Per gamma and expiry the statistics block, SVMC_TILTED_STATS_DOUBLES doubles in f8's order and with f8's meanings:
 *   {normalizer = n_kept / sum W, its error sqrt(sum (1 - normalizer W)^2) / sum W, gamma_forward = sum W (F_t - corr) / sum W, its
 *    error sqrt(sum (W (F_t - corr - gamma_forward))^2) / sum W, effective sample size (sum W)^2 / sum W^2, n_kept, n_dropped, sum W}.
 * No kept path, or kept paths of zero weight only, are NOT errors of the call: the prices are then NaN and the block says so.
 * Two identities hold to rounding: at gamma = 0 the price is svmc_cmc_payoff_chain's at discount factor 1; on rows with cv = 0
 * everything is svmc_tilted_payoff_chain's on x = mu.
 *
 *   svmc_tilted_cond_workspace_bytes   host only: the device workspace that serves any chain of n_expiries expiries and
 *                              total_strikes strikes at this n_path and n_gammas.
 *   svmc_tilted_cond_payoff_chain      mu_snapshots_host, cv_snapshots_host: HOST arrays of n_expiries DEVICE pointers (as in
 *                              svmc_cmc_payoff_chain); strikes / types / shifts concatenated, expiry i owning
 *                              [strike_offsets_host[i], strike_offsets_host[i + 1]).  prices_host, stderrs_host:
 *                              [n_gammas][sum K_i], stats_host: [n_gammas][n_expiries][SVMC_TILTED_STATS_DOUBLES], host arrays.
 *                              One upload of the chain's table, four launches on `stream` with no host round trip between
 *                              them, one download, one synchronise.  Every sum has a fixed order that depends on n_path alone:
 *                              a gamma's, an expiry's and a strike's results are the same bits whichever other gammas, strikes
 *                              or expiries share the call.
 * Everything is checked before anything is launched: SVMC_ERR_INVALID_ARGUMENT for a null pointer (a null snapshot among them),
 * n_path < 1, n_expiries < 1, n_gammas outside 1 .. SVMC_TILTED_MAX_GAMMAS, strike offsets that do not start at 0 or decrease, a
 * gamma, forward, strike or shift that is not finite, a forward that is not positive; SVMC_ERR_UNKNOWN_PAYOFF for a type code
 * other than SVMC_CALL / SVMC_PUT; SVMC_ERR_WORKSPACE for a workspace below svmc_tilted_cond_workspace_bytes; SVMC_ERR_HIP for
 * a failure of the runtime.
 * Left out: the many-job form (different jump parameters per job), IC / IP, several GPUs.  Many (sigma, gamma) sets on one set of rows
 * and the calibration objective on them are DESIGN.md row f20: svmc_jump_sets_payoff_chain of libsvmc_est.so (svmc_est.h).  Greeks
 * and densities under the kernel are DESIGN.md row f18:
 * svmc_tilted_cond_greeks_chain of libsvmc_est.so (svmc_est.h), on the same rows and with this entry's keep rule, weight and corr. */
SVMC_EXT_API int svmc_tilted_cond_workspace_bytes(size_t n_path, int n_expiries, size_t total_strikes, int n_gammas, size_t *bytes);
SVMC_EXT_API int svmc_tilted_cond_payoff_chain(const double *const *mu_snapshots_host, const double *const *cv_snapshots_host,
                                               size_t n_path, const double *forwards_host, int n_expiries,
                                               const double *strikes_host, const int8_t *types_host, const double *shifts_host,
                                               const size_t *strike_offsets_host, const double *gammas_host, int n_gammas,
                                               int recenter, double *prices_host, double *stderrs_host, double *stats_host,
                                               void *workspace, size_t workspace_bytes, svmc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SVMC_EXT_H */
