"""
stochvolmodels_amd -- MI355X-native Monte Carlo engine for the StochVolModels hot path.

Module layout and public names mirror the reference package (`stochvolmodels`) for the Monte Carlo path:
    stochvolmodels_amd.pricers.logsv_pricer   LogSVPricer, logsv_mc_chain_pricer(_fixed_randoms, _many, _conditional, _conditional_many, _conditional_sets),
                                              logsv_mc_chain_greeks(_conditional), simulate_logsv_x_vol_terminal,
                                              get_randoms_for_chain_valuation
    stochvolmodels_amd.pricers.heston_pricer  HestonPricer, HestonParams, heston_mc_chain_pricer(_many, _conditional, _conditional_many, _conditional_sets),
                                              heston_mc_chain_greeks(_conditional), simulate_heston_x_vol_terminal
    stochvolmodels_amd.pricers.hawkes_jd_pricer  HawkesJDPricer, HawkesJDParams, hawkesjd_mc_chain_pricer,
                                              hawkesjd_chain_pricer(_batch), simulate_hawkesjd_terminal,
                                              hawkesjd_forwards_under_risk_kernel, hawkesjd_pdf_under_risk_kernel,
                                              hawkesjd_chain_pricer_with_risk_premia(_batch),
                                              hawkesjd_mc_chain_pricer_with_risk_premia(_gammas),
                                              hawkesjd_mc_chain_pricer_many,
                                              hawkesjd_mc_chain_pricer_with_risk_premia_gammas_many,
                                              hawkesjd_mc_chain_pricer_conditional, hawkesjd_mc_chain_greeks_conditional,
                                              hawkesjd_mc_chain_pricer_conditional_with_risk_premia(_gammas),
                                              hawkesjd_mc_chain_greeks_conditional_with_risk_premia(_gammas),
                                              hawkesjd_jump_rows, HawkesJumpRows, hawkesjd_mc_chain_pricer_conditional_sets
    stochvolmodels_amd.pricers.il_pricer      logsv_il_pricer(_vector, _batch), square_root_payoff_pricer_with_mgf_grid,
                                              compute_mc_il_payoff
    stochvolmodels_amd.utils.mc_payoffs       compute_mc_vars_payoff, compute_mc_vars_payoff_with_gamma,
                                              compute_mc_vars_payoff_conditional(_with_gamma), compute_mc_vars_greeks(_conditional(_with_gamma)),
                                              compute_mc_vars_sens_conditional, compute_mc_vars_payoff_jump_sets
    stochvolmodels_amd.utils.funcs            set_time_grid, set_seed, timer
    stochvolmodels_amd.utils.config           OptionType, VariableType
    stochvolmodels_amd.data.option_chain      OptionChain
All arithmetic runs in libsvmc.so (hand-written HIP for gfx950, C ABI in include/svmc.h, closed at 143 entry points) and in
libsvmc_ext.so and libsvmc_est.so beside it (include/svmc_ext.h, include/svmc_est.h: estimators on caller-owned device arrays);
there is no CPU fallback.  Names resolve lazily so importing the package does not load the GPU library.
"""
import importlib

__version__ = "0.3.0"
# the counter-based random stream the generators draw from (include/svmc.h SVMC_RNG_STREAM_VERSION, CHANGELOG.md): results
# for a given seed are reproducible within one stream version
RNG_STREAM_VERSION = 4

_EXPORTS = {
    "OptionType": "utils.config", "VariableType": "utils.config",
    "set_time_grid": "utils.funcs", "set_seed": "utils.funcs", "timer": "utils.funcs",
    "to_flat_np_array": "utils.funcs",
    "compute_mc_vars_payoff": "utils.mc_payoffs",
    "compute_mc_vars_payoff_with_gamma": "utils.mc_payoffs",
    "compute_mc_vars_payoff_conditional": "utils.mc_payoffs",
    "compute_mc_vars_payoff_conditional_with_gamma": "utils.mc_payoffs",
    "compute_mc_vars_greeks_conditional_with_gamma": "utils.mc_payoffs",
    "compute_mc_vars_payoff_jump_sets": "utils.mc_payoffs",
    "compute_mc_vars_greeks": "utils.mc_payoffs",
    "compute_mc_vars_greeks_conditional": "utils.mc_payoffs",
    "compute_mc_vars_pdf_conditional": "utils.mc_payoffs",
    "compute_mc_vars_sens_conditional": "utils.mc_payoffs",
    "hawkesjd_mc_chain_pricer_with_risk_premia": "pricers.hawkes_jd_pricer",
    "hawkesjd_mc_chain_pricer_with_risk_premia_gammas": "pricers.hawkes_jd_pricer",
    "hawkesjd_mc_chain_pricer_many": "pricers.hawkes_jd_pricer",
    "hawkesjd_mc_chain_pricer_with_risk_premia_gammas_many": "pricers.hawkes_jd_pricer",
    "hawkesjd_pdf_under_risk_kernel": "pricers.hawkes_jd_pricer",
    "hawkesjd_mc_chain_pricer_conditional": "pricers.hawkes_jd_pricer",
    "hawkesjd_mc_chain_greeks_conditional": "pricers.hawkes_jd_pricer",
    "hawkesjd_mc_chain_pricer_conditional_with_risk_premia": "pricers.hawkes_jd_pricer",
    "hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas": "pricers.hawkes_jd_pricer",
    "hawkesjd_mc_chain_greeks_conditional_with_risk_premia": "pricers.hawkes_jd_pricer",
    "hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas": "pricers.hawkes_jd_pricer",
    "HawkesJumpRows": "pricers.hawkes_jd_pricer",
    "hawkesjd_jump_rows": "pricers.hawkes_jd_pricer",
    "hawkesjd_mc_chain_pricer_conditional_sets": "pricers.hawkes_jd_pricer",
    "OptionChain": "data.option_chain",
    "ModelParams": "pricers.model_pricer", "ModelPricer": "pricers.model_pricer",
    "LogSvParams": "pricers.logsv.logsv_params",
    "LogSVPricer": "pricers.logsv_pricer", "LOGSV_BTC_PARAMS": "pricers.logsv_pricer",
    "logsv_mc_chain_pricer": "pricers.logsv_pricer",
    "logsv_mc_chain_pricer_many": "pricers.logsv_pricer",
    "logsv_mc_chain_pricer_conditional": "pricers.logsv_pricer",
    "logsv_mc_chain_greeks": "pricers.logsv_pricer",
    "logsv_mc_chain_greeks_conditional": "pricers.logsv_pricer",
    "logsv_mc_chain_pricer_conditional_many": "pricers.logsv_pricer",
    "logsv_mc_chain_pricer_conditional_sets": "pricers.logsv_pricer",
    "logsv_mc_chain_pricer_fixed_randoms": "pricers.logsv_pricer",
    "simulate_logsv_x_vol_terminal": "pricers.logsv_pricer",
    "simulate_vol_paths": "pricers.logsv_pricer",
    "vol_path_moments": "pricers.logsv_pricer",
    "get_randoms_for_chain_valuation": "pricers.logsv_pricer",
    "upload_fixed_randoms": "pricers.logsv_pricer",
    "draw_fixed_randoms_on_device": "pricers.logsv_pricer",
    "logsv_mc_chain_pricer_fixed_randoms_batch": "pricers.logsv_pricer",
    "get_randoms_for_rough_vol_chain_valuation": "pricers.logsv_pricer",
    "rough_logsv_mc_chain_pricer_fixed_randoms": "pricers.logsv_pricer",
    "rough_logsv_mc_chain_pricer": "pricers.logsv_pricer",
    "upload_rough_randoms": "pricers.logsv_pricer",
    "LogsvModelCalibrationType": "pricers.logsv_pricer",
    "ConstraintsType": "pricers.logsv_pricer",
    "CalibrationEngine": "pricers.logsv_pricer",
    "CalibrationError": "utils.calibration",
    "logsv_chain_pricer": "pricers.logsv_pricer", "set_vol_scaler": "pricers.logsv_pricer",
    "logsv_chain_pricer_batch": "pricers.logsv_pricer",
    "ExpansionOrder": "pricers.logsv.affine_expansion", "compute_logsv_a_mgf_grid": "pricers.logsv.affine_expansion",
    "heston_chain_pricer": "pricers.heston_pricer", "compute_heston_mgf_grid": "pricers.heston_pricer",
    "HestonPricer": "pricers.heston_pricer", "HestonParams": "pricers.heston_pricer",
    "BTC_HESTON_PARAMS": "pricers.heston_pricer", "heston_mc_chain_pricer": "pricers.heston_pricer",
    "heston_mc_chain_pricer_many": "pricers.heston_pricer",
    "heston_mc_chain_pricer_conditional": "pricers.heston_pricer",
    "heston_mc_chain_greeks": "pricers.heston_pricer",
    "heston_mc_chain_greeks_conditional": "pricers.heston_pricer",
    "heston_mc_chain_pricer_conditional_many": "pricers.heston_pricer",
    "heston_mc_chain_pricer_conditional_sets": "pricers.heston_pricer",
    "simulate_heston_x_vol_terminal": "pricers.heston_pricer",
    "compute_analytic_qvar": "pricers.logsv.vol_moments_ode",
    "compute_analytic_vol_moments": "pricers.logsv.vol_moments_ode",
    "fit_model_vol_backbone_to_varswaps": "pricers.logsv.vol_moments_ode",
    "compute_var_swap_strike": "utils.var_swap_pricer",
    "HawkesJDParams": "pricers.hawkes_jd_pricer", "HawkesJDPricer": "pricers.hawkes_jd_pricer",
    "logsv_pdfs": "pricers.logsv_pricer", "logsv_pdfs_batch": "pricers.logsv_pricer",
    "get_init_conditions_a": "pricers.logsv.affine_expansion",
    "pdf_with_mgf_grid": "utils.mgf_pricer", "digital_slice_pricer_with_mgf_grid": "utils.mgf_pricer",
    "compute_histogram_data": "utils.funcs",
    "logsv_il_pricer": "pricers.il_pricer", "logsv_il_pricer_vector": "pricers.il_pricer",
    "logsv_il_pricer_batch": "pricers.il_pricer", "square_root_payoff_pricer_with_mgf_grid": "pricers.il_pricer",
    "compute_mc_il_payoff": "pricers.il_pricer", "il_payoff": "pricers.il_pricer",
    "get_transform_var_grid": "utils.mgf_pricer", "compute_integration_weights": "utils.mgf_pricer",
}

__all__ = sorted(_EXPORTS)


def __getattr__(name):
    mod = _EXPORTS.get(name)
    if mod is None:
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    value = getattr(importlib.import_module(f"{__name__}.{mod}"), name)
    globals()[name] = value
    return value


def __dir__():
    return sorted(list(globals()) + list(_EXPORTS))
