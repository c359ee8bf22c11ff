"""
Hawkes jump-diffusion on MI355X: the reference's pricers/hawkes_jd_pricer.py (F. Liu, N. Packham, A. Sepp 2025) with its
names, keyword signatures, defaults and return containers.

Log-returns follow a diffusion plus two jump streams (shifted-exponential sizes, positive and negative) whose intensities are
self- and cross-exciting Hawkes processes.  Two pricers:
  - Monte Carlo (hawkesjd_mc_chain_pricer, simulate_hawkesjd_terminal; reference :643-776): the reference's Euler step at
    its hard-wired 1800 steps per year, one GPU lane per path, randoms drawn on the device (csrc/svmc_hawkes.hip,
    streams 6 and 7 of the counter-based generator).  Extensions: `seed=` and `nb_steps_per_year=`.
  - Fourier (hawkesjd_chain_pricer, compute_hawkes_a_mgf_grid; :365-417, :518-640): the three complex Riccati ODEs
    integrated per transform-grid point on the device with DOP853 at rtol 1e-10 / atol 1e-12 (the reference calls SciPy at
    its default rtol 1e-3), inverted by the existing vanilla slice kernel.
Calibration (HawkesJDPricer.calibrate_model_params_to_chain; :230-302): SLSQP on the vega-weighted squared vol error of 8
parameters, each objective evaluation one Fourier chain pricing on the device.  The forward-difference gradient SLSQP needs at
an iterate (the base point and 8 bumped vectors) is priced in one batch of launches per expiry (hawkesjd_chain_pricer_batch,
csrc/svmc_hawkes.hip's hawkes_mgf_grid_batch_kernel), bit-identical to one pricing per vector.
Risk-premia (Esscher-type) kernel (hawkesjd_forwards_under_risk_kernel, hawkesjd_pdf_under_risk_kernel, hawkesjd_chain_pricer_with_risk_premia,
HawkesJDPricer.calibrate_risk_premia_gamma_to_chain; :304-357, :420-515): the normalizers and gamma forwards of every expiry in
one launch (hawkes_risk_forwards_kernel: the coefficient ODEs from zero over each whole ttm at phi = -gamma and -gamma - 1),
the chained coefficient ODEs on the grid of real part -0.5 - gamma, and per expiry one inversion launch that finishes the
prices on the device (mgf_gamma_slice_kernel); hawkesjd_chain_pricer_with_risk_premia_batch prices several (sigma, gamma) sets
side by side for the calibration's gradient.
Monte Carlo under that kernel (hawkesjd_mc_chain_pricer_with_risk_premia(_gammas), not in the reference, whose users weight
downloaded paths by hand): one stepping launch, then the exponentially weighted payoff reduction of the resident snapshots for
every gamma at once (tilted_payoff_group_kernel), with delta-method standard errors, the normalizer, the gamma forward and the
effective sample size per expiry.
Many independent Monte Carlo jobs of one chain (hawkesjd_mc_chain_pricer_many, hawkesjd_mc_chain_pricer_with_risk_premia_gammas_many
and the pricer methods over them; not in the reference): every job has its own parameter set -- both start intensities included --
and its own random stream, ONE launch steps them all (hawkesjd_chain_rng_many_kernel), and each job's results are bit-equal to
its single call.
Conditional Monte Carlo (hawkesjd_mc_chain_pricer_conditional, hawkesjd_mc_chain_greeks_conditional and the pricer methods over them;
not in the reference): the diffusion is independent of the jumps and the intensities, so each path carries the conditional mean of
its log-return, the variance sigma^2 T is one number per expiry, and a path contributes a Black-76 price, its delta and gammas and
the density at the strike instead of a payoff (hawkes_chain_cond_kernel, streams 9 and 10; the tails of the LogSV / Heston
conditional pricers).
Conditional Monte Carlo under the risk-premia kernel (hawkesjd_mc_chain_pricer_conditional_with_risk_premia(_gammas); not in the
reference): the two rows above joined by the Esscher identity -- a path's weight exp(gamma mu + gamma^2 cv / 2) carries no diffusion
noise and multiplies a Black-76 price at the forward shifted by gamma cv (include/svmc_ext.h, libsvmc_ext.so's
tilted_cond_payoff_kernel on the rows hawkes_chain_cond_kernel leaves).
Its Greeks and the bandwidth-free density under the kernel (hawkesjd_mc_chain_greeks_conditional_with_risk_premia(_gammas),
HawkesJDPricer.get_log_return_mc_pdf_conditional_under_risk_kernel; not in the reference): the weight depends on neither the forward
nor the strike, so the derivatives are weighted means of per-path Black-76 derivatives at the shifted forward (include/svmc_est.h,
libsvmc_est.so's tilted_cond_greeks_kernel on the same rows).
The reference's quirks are kept: `risk_premia_gamma` is accepted and unused by hawkesjd_mc_chain_pricer, `is_spot_measure` is ignored
by it, and a variable_type other than LOG_RETURN raises (the reference would price the log-return as a variance).  Under the
risk-premia kernel: the forwards follow zip(ttms, forwards) (entries beyond the shorter stay 1.0), discfactors are ignored
(the prices are undiscounted), and the calibration mutates and returns params0.
Not switched (yet): price_chain, price_chain_batch and compute_chain_prices_with_vols still raise NotImplementedError when
params.risk_premia_gamma is set, where the reference dispatches to the risk-premia pricer; the calibration calls that pricer
directly.  Switching that dispatch changes existing behaviour and is a separate change.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from dataclasses import asdict, dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .. import _lib
from .. import dist as svdist
from ..analytic import ODE_ATOL, ODE_RTOL, AnalyticGrid, chain_prices_from_sums, chain_sums
from ..data.option_chain import OptionChain
from ..engine import (JUMP_SETS_MAX, DeviceBuffer, get_engine, marshalled_chain, option_type_codes, tilted_chain_arrays,
                      tilted_gammas, tilted_greeks_stats_dicts, tilted_type_codes)
from ..mc_chain import chain_shaped, check_many_args, many_job_chunks, many_job_streams, many_jobs_shaped, variable_type_code
from ..utils import mgf_pricer as mgfp
from ..utils.calibration import ImpliedVolObjective, chain_calibration_weights
from ..utils.config import VariableType
from ..utils.funcs import chain_step_grid, next_rng_call, time_grid_steps, timer, to_flat_np_array
from .logsv_pricer import (check_conditional_request, conditional_greeks_shaped, conditional_log_return_pdf,
                           mixture_log_return_pdf, refuse_sharded_paths)
from .model_pricer import ModelParams, ModelPricer

MAX_PHI = 500
# the reference's hard-wired step count (:753): "need small dt step for large intensities"
NB_STEPS_PER_YEAR = 5 * 360
LOG_RETURN = 1
# include/svmc.h SVMC_HAWKESJD_PARAMS: the order of the dataclass fields
PARAM_NAMES = ("mu", "sigma", "shift_p", "mean_p", "shift_m", "mean_m", "lambda_p", "theta_p", "kappa_p", "beta1_p", "beta2_p",
               "lambda_m", "theta_m", "kappa_m", "beta1_m", "beta2_m")


@dataclass
class HawkesJDParams(ModelParams):
    """parameters of the 2-factor Hawkes jump-diffusion, annualised (reference :40-118)"""
    mu: float = 0.0
    sigma: float = 0.45
    # jumps
    shift_p: float = 0.06
    mean_p: float = 0.03
    shift_m: float = -0.06
    mean_m: float = -0.03
    # positive jumps intensity
    lambda_p: float = 6.55
    theta_p: float = 6.55
    kappa_p: float = 22.29
    beta1_p: float = 76.0
    beta2_p: float = -67.58
    # minus jumps intensity
    lambda_m: float = 8.50
    theta_m: float = 8.50
    kappa_m: float = 29.0
    beta1_m: float = 104.55
    beta2_m: float = -109.6
    risk_premia_gamma: float = None

    def __post_init__(self):
        self.compensator_p = np.exp(self.shift_p) / (1.0 - self.mean_p) - 1.0
        self.compensator_m = np.exp(self.shift_m) / (1.0 - self.mean_m) - 1.0

    def to_dict(self) -> Dict[str, Any]:
        return asdict(self)

    def print(self) -> None:
        for k, v in self.to_dict().items():
            print(f"{k}={v}")
        print('condifions')
        print(f"jump1={self.jump1_cond:0.4f} > 0")
        print(f"jump2={self.jump2_cond:0.4f} > 0")

    @property
    def jump1_cond(self) -> float:
        """stationarity margin of the positive-jump intensity: kappa_p - beta1_p E[J_p] - beta2_p E[J_m]"""
        return self.kappa_p - self.beta1_p * self.exp_jump_p - self.beta2_p * self.exp_jump_m

    @property
    def jump2_cond(self) -> float:
        """stationarity margin of the negative-jump intensity"""
        return self.kappa_m - self.beta2_m * self.exp_jump_m - self.beta1_m * self.exp_jump_p

    @property
    def exp_jump_p(self) -> float:
        return self.shift_p + self.mean_p

    @property
    def exp_jump_m(self) -> float:
        return self.shift_m + self.mean_m

    @property
    def jumps_var_m(self) -> float:
        return np.square(self.shift_m) + np.square(self.mean_m)

    @property
    def jumps_var_p(self) -> float:
        return np.square(self.shift_p) + np.square(self.mean_p)


def params_block(**kw) -> np.ndarray:
    """the SVMC_HAWKESJD_PARAMS doubles of the C ABI from keyword parameters (extra keywords are ignored)"""
    return params_block_of(kw)


def params_block_of(values) -> np.ndarray:
    """params_block from a mapping that holds the sixteen names among others: a pricer passes its locals()"""
    return np.array([float(values[k]) for k in PARAM_NAMES], dtype=np.float64)


def forwards_triples(stats) -> list:
    """what return_forwards=True adds: per gamma (or set) the (normalizers, gamma_forwards, stats) of stats [n_expiries, 8]"""
    return [(st[:, 0].copy(), st[:, 2].copy(), st) for st in stats]


def _at_one_gamma(gammas_pricer, args: dict):
    """a *_gammas pricer at the ONE gamma of a single-gamma wrapper, so the two agree bit for bit; args: the wrapper's locals()"""
    args = dict(args)
    args.update(args.pop("kwargs"))
    risk_premia_gamma = args.pop("risk_premia_gamma")
    if risk_premia_gamma is None:
        raise ValueError("risk_premia_gamma must be set for the risk-premia pricer")
    return gammas_pricer(risk_premia_gammas=[risk_premia_gamma], **args)


def _check_variable_type(variable_type) -> None:
    if variable_type_code(variable_type) != LOG_RETURN:
        # the reference passes x as sigma0 and qvar0 to the payoff (:701), i.e. would price the log-return as a variance
        raise NotImplementedError(f"variable_type={variable_type}: the Hawkes jump-diffusion prices LOG_RETURN only")


class HawkesJDPricer(ModelPricer):

    def price_chain(self, option_chain: OptionChain, params: HawkesJDParams, is_spot_measure: bool = True, **kwargs
                    ) -> List[np.ndarray]:
        """analytic chain prices (reference :125-153).  With params.risk_premia_gamma set this still raises rather than
        dispatch to hawkesjd_chain_pricer_with_risk_premia as the reference does (a separate, behaviour-changing step): call
        that pricer directly"""
        if params.risk_premia_gamma is not None:
            raise NotImplementedError("price_chain does not dispatch to the risk-premia pricer: call "
                                      "hawkesjd_chain_pricer_with_risk_premia(_batch) directly")
        return hawkesjd_chain_pricer(model_params=params, ttms=option_chain.ttms, forwards=option_chain.forwards,
                                     discfactors=option_chain.discfactors, strikes_ttms=option_chain.strikes_ttms,
                                     optiontypes_ttms=option_chain.optiontypes_ttms, is_spot_measure=is_spot_measure, **kwargs)

    @timer
    def model_mc_price_chain(self, option_chain: OptionChain, params: HawkesJDParams, nb_path: int = 100000, **kwargs
                             ) -> Tuple[List[np.ndarray], List[np.ndarray]]:
        """Monte Carlo chain prices (reference :156-170); extensions seed=, nb_steps_per_year=, comm="""
        return hawkesjd_mc_chain_pricer(ttms=option_chain.ttms, forwards=option_chain.forwards,
                                        discfactors=option_chain.discfactors, strikes_ttms=option_chain.strikes_ttms,
                                        optiontypes_ttms=option_chain.optiontypes_ttms, nb_path=nb_path,
                                        **params.to_dict(), **kwargs)

    def model_mc_price_chain_conditional(self, option_chain: OptionChain, params: HawkesJDParams, nb_path: int = 100000, **kwargs):
        """model_mc_price_chain by conditional Monte Carlo (hawkesjd_mc_chain_pricer_conditional); seed=, nb_steps_per_year=,
        recenter= and return_stats= are passed on"""
        return hawkesjd_mc_chain_pricer_conditional(ttms=option_chain.ttms, forwards=option_chain.forwards,
                                                    discfactors=option_chain.discfactors, strikes_ttms=option_chain.strikes_ttms,
                                                    optiontypes_ttms=option_chain.optiontypes_ttms, nb_path=nb_path,
                                                    **params.to_dict(), **kwargs)

    def model_mc_chain_greeks_conditional(self, option_chain: OptionChain, params: HawkesJDParams, nb_path: int = 100000, **kwargs
                                          ) -> dict:
        """model_mc_price_chain_conditional with delta, dual delta, gamma and dual gamma (hawkesjd_mc_chain_greeks_conditional)"""
        return hawkesjd_mc_chain_greeks_conditional(ttms=option_chain.ttms, forwards=option_chain.forwards,
                                                    discfactors=option_chain.discfactors, strikes_ttms=option_chain.strikes_ttms,
                                                    optiontypes_ttms=option_chain.optiontypes_ttms, nb_path=nb_path,
                                                    **params.to_dict(), **kwargs)

    def get_log_return_mc_pdf_conditional(self, params: HawkesJDParams, ttm: float, x_grid: np.ndarray, nb_path: int = 100000,
                                          seed: Optional[int] = None, recenter: bool = False, return_stderr: bool = False,
                                          nb_steps_per_year: int = NB_STEPS_PER_YEAR):
        """the density of the simulated log-return at x_grid from the conditional estimator's dual gamma, without a bandwidth
        (logsv_pricer.conditional_log_return_pdf): each path adds a Gaussian of variance sigma^2 ttm around its jump path.
        UN-NORMALISED: it integrates by itself to the share of the kept paths (1 when none is dropped; 0 at sigma = 0, where every
        path is a point mass).  recenter=False: the density of the simulated x itself.  With return_stderr=True (pdf, its standard
        error)."""
        def route(**chain):
            return hawkesjd_mc_chain_greeks_conditional(nb_path=nb_path, nb_steps_per_year=nb_steps_per_year, seed=seed,
                                                        recenter=recenter, **_model_kwargs(params), **chain)
        return conditional_log_return_pdf(route, ttm, x_grid, return_stderr)

    def price_chain_batch(self, option_chain: OptionChain, params_list: Sequence[HawkesJDParams], is_spot_measure: bool = True,
                          **kwargs) -> List[List[np.ndarray]]:
        """price_chain for several parameter sets in one batch of launches (hawkesjd_chain_pricer_batch)"""
        if any(p.risk_premia_gamma is not None for p in params_list):
            raise NotImplementedError("price_chain does not dispatch to the risk-premia pricer: call "
                                      "hawkesjd_chain_pricer_with_risk_premia(_batch) directly")
        return hawkesjd_chain_pricer_batch(params_list=params_list, ttms=option_chain.ttms, forwards=option_chain.forwards,
                                           discfactors=option_chain.discfactors, strikes_ttms=option_chain.strikes_ttms,
                                           optiontypes_ttms=option_chain.optiontypes_ttms, is_spot_measure=is_spot_measure,
                                           **kwargs)

    def calibration_objective(self, option_chain: OptionChain, params0: HawkesJDParams, is_vega_weighted: bool = True,
                              is_unit_ttm_vega: bool = False, **kwargs) -> ImpliedVolObjective:
        """the objective of calibrate_model_params_to_chain as a callable of the optimizer's 8-vector (reference :280-285),
        with its batched gradient unless batched_gradient=False; ode_rtol= / ode_atol= as there"""
        _, market_vols_ttms = option_chain.get_chain_data_as_xy()
        market_vols = to_flat_np_array(market_vols_ttms)
        weights = chain_calibration_weights(option_chain, market_vols, is_vega_weighted, is_unit_ttm_vega)
        tol = {k: kwargs[k] for k in ("ode_rtol", "ode_atol") if k in kwargs}

        def model_vols(pars):
            return self.compute_model_ivols_for_chain(option_chain=option_chain,
                                                      params=unpack_calibration_vector(pars, params0), **tol)

        def model_vols_batch(pars_list):
            prices = self.price_chain_batch(option_chain=option_chain,
                                            params_list=[unpack_calibration_vector(p, params0) for p in pars_list], **tol)
            return [option_chain.compute_model_ivols_from_chain_data(model_prices=pr) for pr in prices]

        batched = bool(kwargs.get("batched_gradient", True))
        return ImpliedVolObjective(model_vols, market_vols, weights, model_vols_batch=model_vols_batch if batched else None,
                                   bounds=CALIBRATION_BOUNDS)

    @timer
    def calibrate_model_params_to_chain(self, option_chain: OptionChain, params0: HawkesJDParams,
                                        is_vega_weighted: bool = True, is_unit_ttm_vega: bool = False, **kwargs
                                        ) -> HawkesJDParams:
        """fit sigma, mean_p, mean_m, theta_p, theta_m, one kappa for both sides, beta_p (beta1_p = -beta2_p) and beta_m
        (beta1_m = -beta2_m) to the chain's mid implied vols, with shift_p, shift_m, lambda_p, lambda_m from params0 and
        mu = 0 (reference :230-302): SLSQP (ftol 1e-8) on the np.nansum of per-slice-normalised vega-weighted squared vol
        errors, subject to jump1_cond + jump2_cond >= 0 (calibration_start_vector, CALIBRATION_BOUNDS,
        unpack_calibration_vector, calibration_constraint).  As in the reference, the transform grid follows each
        candidate's own sigma, and the optimizer's vector is returned whatever SLSQP's exit status.
        `kwargs`: disp= (SLSQP printing, default True as in the reference); batched_gradient= (default True: SLSQP's
        forward-difference gradient -- the same points it would evaluate itself -- from one hawkesjd_chain_pricer_batch per
        iterate); ode_rtol= / ode_atol= (the coefficient ODEs' tolerances, default 1e-10 / 1e-12).
        `self.last_calibration` keeps {"n_eval", "n_gradient_batches", "objective"} of the run."""
        from scipy.optimize import minimize
        objective = self.calibration_objective(option_chain, params0, is_vega_weighted, is_unit_ttm_vega, **kwargs)
        batched = objective.model_vols_batch is not None
        extra = dict(jac=objective.gradient) if batched else {}
        res = minimize(objective, calibration_start_vector(params0), args=None, method="SLSQP",
                       constraints={"type": "ineq", "fun": lambda pars: calibration_constraint(pars, params0)},
                       bounds=CALIBRATION_BOUNDS, options={"disp": bool(kwargs.get("disp", True)), "ftol": 1e-8}, **extra)
        self.last_calibration = dict(n_eval=objective.n_eval, n_gradient_batches=objective.n_batches,
                                     objective=objective(res.x), success=bool(res.success), message=str(res.message))
        return unpack_calibration_vector(res.x, params0)

    def risk_premia_calibration_objective(self, option_chain: OptionChain, params0: HawkesJDParams,
                                          is_vega_weighted: bool = True, is_unit_ttm_vega: bool = False,
                                          print_iter: bool = True, **kwargs) -> ImpliedVolObjective:
        """the objective of calibrate_risk_premia_gamma_to_chain as a callable of the optimizer's (sigma, gamma / 8)
        (reference :336-342): every call unpacks into params0 IN PLACE, as there; with its batched gradient at SLSQP's step
        0.025 unless batched_gradient=False; ode_rtol= / ode_atol= as in hawkesjd_chain_pricer.  estimator="conditional" (with nb_path=,
        nb_steps_per_year=, seed=, recenter_forward=): the model prices by conditional Monte Carlo on jump rows stepped once, here
        (calibrate_risk_premia_gamma_to_chain states the mode); the handle is the returned objective's .jump_rows"""
        estimator = kwargs.get("estimator", "fourier")
        if estimator not in ("fourier", "conditional"):
            raise ValueError(f"estimator={estimator!r}: 'fourier' or 'conditional'")
        if params0.risk_premia_gamma is None:
            raise ValueError("params0.risk_premia_gamma must be set: it is the start value of the fit")
        _, market_vols_ttms = option_chain.get_chain_data_as_xy()
        market_vols = to_flat_np_array(market_vols_ttms)
        weights = risk_premia_calibration_weights(option_chain, market_vols, is_vega_weighted, is_unit_ttm_vega)
        tol = {k: kwargs[k] for k in ("ode_rtol", "ode_atol") if k in kwargs}
        chain = dict(ttms=option_chain.ttms, forwards=option_chain.forwards, discfactors=option_chain.discfactors,
                     strikes_ttms=option_chain.strikes_ttms, optiontypes_ttms=option_chain.optiontypes_ttms,
                     return_forwards=True, **tol)

        def unpack(pars) -> HawkesJDParams:
            params = unpack_risk_premia_vector(pars, params0)
            if print_iter:
                print(f"unpack_pars: sigma={pars[0]}, gamma={params.risk_premia_gamma}")
            return params

        def ivols(prices_ttms, gamma_forwards):             # inverted against the gamma forwards (:173-191)
            # an expiry whose forward ODE the integrator gave up on (NaN) has NaN prices and NaN vols, dropped by the nansum
            ok = np.isfinite(gamma_forwards) & (gamma_forwards > 0.0)
            vols = option_chain.compute_model_ivols_from_chain_data(model_prices=prices_ttms,
                                                                    forwards=np.where(ok, gamma_forwards, 1.0))
            return [v if good else np.full_like(v, np.nan) for v, good in zip(vols, ok)]

        if estimator == "conditional":
            # the model prices by conditional Monte Carlo on jump rows stepped ONCE, here, on one (seed, call id): an evaluation is a
            # tail (HawkesJumpRows.price_sets); codec, bounds, weights and the inversion above are the Fourier objective's
            check_conditional_request("risk_premia_calibration_objective", VariableType.LOG_RETURN, kwargs.get("comm"),
                                      kwargs.get("devices"), option_chain.optiontypes_ttms)
            model = {k: v for k, v in params0.to_dict().items() if k not in ("sigma", "risk_premia_gamma")}
            rows = hawkesjd_jump_rows(option_chain.ttms, nb_path=int(kwargs.get("nb_path", 100000)),
                                      nb_steps_per_year=int(kwargs.get("nb_steps_per_year", NB_STEPS_PER_YEAR)),
                                      seed=kwargs.get("seed"), **model)
            recenter = bool(kwargs.get("recenter_forward", False))

            def sets_vols(params_list):
                prices, _, fwds = rows.price_sets([p.sigma for p in params_list], [p.risk_premia_gamma for p in params_list],
                                                  option_chain.forwards, option_chain.strikes_ttms, option_chain.optiontypes_ttms,
                                                  recenter_forward=recenter, return_forwards=True)
                return [ivols(pr, gf) for pr, (_, gf, _) in zip(prices, fwds)]

            def model_vols(pars):
                return sets_vols([unpack(pars)])[0]

            def model_vols_batch(pars_list):
                # each vector priced with its own copy of params0 as unpack leaves it; params0 ends at the last vector
                return sets_vols([dataclasses.replace(unpack(pars)) for pars in pars_list])
        else:
            def model_vols(pars):
                prices, (_, gamma_forwards) = hawkesjd_chain_pricer_with_risk_premia(model_params=unpack(pars), **chain)
                return ivols(prices, gamma_forwards)

            def model_vols_batch(pars_list):
                # each vector priced with its own copy of params0 as unpack leaves it; params0 ends at the last vector
                params_list = [dataclasses.replace(unpack(pars)) for pars in pars_list]
                prices, forwards = hawkesjd_chain_pricer_with_risk_premia_batch(params_list=params_list, **chain)
                return [ivols(pr, gf) for pr, (_, gf) in zip(prices, forwards)]

        batched = bool(kwargs.get("batched_gradient", True))
        objective = ImpliedVolObjective(model_vols, market_vols, weights, model_vols_batch=model_vols_batch if batched else None,
                                        bounds=RISK_PREMIA_BOUNDS, fd_step=RISK_PREMIA_FD_STEP)
        if estimator == "conditional":
            objective.jump_rows = rows                           # the handle lives as long as the objective
        return objective

    @timer
    def calibrate_risk_premia_gamma_to_chain(self, option_chain: OptionChain, params0: HawkesJDParams,
                                             is_vega_weighted: bool = True, is_unit_ttm_vega: bool = False, maxiter: int = 100,
                                             print_iter: bool = True, **kwargs) -> HawkesJDParams:
        """fit sigma and risk_premia_gamma to the chain's mid implied vols with every other parameter from params0 (reference
        :304-357): SLSQP on the optimizer vector (sigma, gamma / 8) in RISK_PREMIA_BOUNDS, options {'disp': True, 'ftol':
        1e-16, 'maxiter': maxiter, 'eps': 0.025} and tol=1e-16, no constraint and no result check; the objective is
        np.nansum(w (model - market)^2) with w = 10000 x the per-slice normalised vegas (or 10000 x ones), the model vols
        inverted against the gamma forwards (risk_premia_calibration_objective).  Each evaluation is one
        hawkesjd_chain_pricer_with_risk_premia on the device.  As in the reference, every unpack MUTATES params0 (sigma,
        risk_premia_gamma), the fit is params0 itself, and print_iter prints one line per evaluated vector.
        `kwargs`: disp= (SLSQP printing, default True); batched_gradient= (default True: SLSQP's forward-difference
        gradient at its step 0.025 -- the same points it would evaluate -- from one
        hawkesjd_chain_pricer_with_risk_premia_batch of the bumped vectors per iterate; False lets SLSQP difference itself);
        ode_rtol= / ode_atol= (default 1e-10 / 1e-12); estimator= ("fourier", the default: everything above; "conditional": the
        model prices by conditional Monte Carlo on jump rows stepped ONCE at construction -- hawkesjd_jump_rows with nb_path=,
        nb_steps_per_year=, seed= -- so that every evaluation, and every gradient batch of SLSQP's bumped points, is
        one HawkesJumpRows.price_sets with recenter_forward=; codec, bounds, weights, options and the inversion are unchanged,
        and last_calibration gains estimator and n_stepping_calls = 1; any other value: ValueError).
        `self.last_calibration` keeps {"n_eval", "n_gradient_batches", "objective", "success", "status", "message", "nit",
        "nfev", "x"} of the run."""
        from scipy.optimize import minimize
        objective = self.risk_premia_calibration_objective(option_chain, params0, is_vega_weighted, is_unit_ttm_vega,
                                                           print_iter, **kwargs)
        extra = dict(jac=objective.gradient) if objective.model_vols_batch is not None else {}
        options = {"disp": bool(kwargs.get("disp", True)), "ftol": 1e-16, "maxiter": maxiter, "eps": RISK_PREMIA_FD_STEP}
        res = minimize(objective, risk_premia_start_vector(params0), args=None, method="SLSQP", bounds=RISK_PREMIA_BOUNDS,
                       options=options, tol=1e-16, **extra)
        self.last_calibration = dict(n_eval=objective.n_eval, n_gradient_batches=objective.n_batches, objective=float(res.fun),
                                     success=bool(res.success), status=int(res.status), message=str(res.message),
                                     nit=int(res.nit), nfev=int(res.nfev), x=np.array(res.x, dtype=float))
        if kwargs.get("estimator", "fourier") == "conditional":
            self.last_calibration.update(estimator="conditional", n_stepping_calls=1)
            objective.jump_rows.free()
        fit = unpack_risk_premia_vector(res.x, params0)
        if print_iter:
            print(f"unpack_pars: sigma={res.x[0]}, gamma={fit.risk_premia_gamma}")
        return fit

    @timer
    def model_mc_price_chain_with_risk_premia(self, option_chain: OptionChain, params: HawkesJDParams, nb_path: int = 100000,
                                              **kwargs) -> Tuple[List[np.ndarray], List[np.ndarray]]:
        """Monte Carlo chain prices under the risk-premia kernel of params.risk_premia_gamma
        (hawkesjd_mc_chain_pricer_with_risk_premia); extensions seed=, nb_steps_per_year=, recenter_forward=, return_forwards="""
        if params.risk_premia_gamma is None:
            raise ValueError("risk_premia_gamma must be set for the risk-premia pricer")
        return hawkesjd_mc_chain_pricer_with_risk_premia(ttms=option_chain.ttms, forwards=option_chain.forwards,
                                                         discfactors=option_chain.discfactors,
                                                         strikes_ttms=option_chain.strikes_ttms,
                                                         optiontypes_ttms=option_chain.optiontypes_ttms, nb_path=nb_path,
                                                         **params.to_dict(), **kwargs)

    def model_mc_price_chain_conditional_with_risk_premia(self, option_chain: OptionChain, params: HawkesJDParams,
                                                          nb_path: int = 100000, **kwargs):
        """model_mc_price_chain_with_risk_premia by conditional Monte Carlo
        (hawkesjd_mc_chain_pricer_conditional_with_risk_premia); extensions seed=, nb_steps_per_year=, recenter_forward=,
        return_forwards="""
        if params.risk_premia_gamma is None:
            raise ValueError("risk_premia_gamma must be set for the risk-premia pricer")
        return hawkesjd_mc_chain_pricer_conditional_with_risk_premia(ttms=option_chain.ttms, forwards=option_chain.forwards,
                                                                     discfactors=option_chain.discfactors,
                                                                     strikes_ttms=option_chain.strikes_ttms,
                                                                     optiontypes_ttms=option_chain.optiontypes_ttms, nb_path=nb_path,
                                                                     **params.to_dict(), **kwargs)

    def model_mc_price_chain_conditional_sets(self, option_chain: OptionChain, params: HawkesJDParams, sigmas, risk_premia_gammas,
                                              nb_path: int = 100000, **kwargs):
        """the chain at every (sigma_q, gamma_q) with the other parameters from params, from ONE stepping launch
        (hawkesjd_mc_chain_pricer_conditional_sets); extensions seed=, nb_steps_per_year=, recenter_forward=, return_forwards="""
        return hawkesjd_mc_chain_pricer_conditional_sets(sigmas, risk_premia_gammas, ttms=option_chain.ttms,
                                                         forwards=option_chain.forwards, discfactors=option_chain.discfactors,
                                                         strikes_ttms=option_chain.strikes_ttms,
                                                         optiontypes_ttms=option_chain.optiontypes_ttms, nb_path=nb_path,
                                                         **params.to_dict(), **kwargs)

    def model_mc_chain_greeks_conditional_with_risk_premia(self, option_chain: OptionChain, params: HawkesJDParams,
                                                           nb_path: int = 100000, **kwargs) -> dict:
        """model_mc_price_chain_conditional_with_risk_premia with delta, dual delta, gamma and dual gamma under the kernel
        (hawkesjd_mc_chain_greeks_conditional_with_risk_premia); the gamma is the parameter set's; extensions seed=,
        nb_steps_per_year=, recenter_forward=, return_stats="""
        if params.risk_premia_gamma is None:
            raise ValueError("risk_premia_gamma must be set for the risk-premia pricer")
        return hawkesjd_mc_chain_greeks_conditional_with_risk_premia(ttms=option_chain.ttms, forwards=option_chain.forwards,
                                                                     discfactors=option_chain.discfactors,
                                                                     strikes_ttms=option_chain.strikes_ttms,
                                                                     optiontypes_ttms=option_chain.optiontypes_ttms, nb_path=nb_path,
                                                                     **params.to_dict(), **kwargs)

    def get_log_return_mc_pdf_conditional_under_risk_kernel(self, params: HawkesJDParams, ttm: float, x_grid: np.ndarray,
                                                            risk_premia_gammas, nb_path: int = 100000, seed: Optional[int] = None,
                                                            return_stderr: bool = False,
                                                            nb_steps_per_year: int = NB_STEPS_PER_YEAR):
        """the density of the simulated log-return under exp(gamma x) at x_grid for every gamma, WITHOUT a bandwidth: the dual
        gamma of the conditional estimator under the kernel at K = exp(x), F = 1, no recentring --
        pdf_gamma(x) = sum_j W_j N(x; mu_j + gamma sigma^2 ttm, sigma^2 ttm) / sum_j W_j.  Normalised by the weights: it integrates
        to the weight share of the kept paths (1 when none is dropped; 0 at sigma = 0, where every path is a point mass).  One
        stepping call for all gammas.  Returns pdf [gamma][x] (x in x_grid's shape), with return_stderr=True (pdf, its standard
        error)."""
        x = np.asarray(x_grid, dtype=np.float64)
        strikes = np.exp(x.ravel())
        out = hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas(
            ttms=np.array([float(ttm)]), forwards=np.array([1.0]), discfactors=np.array([1.0]), strikes_ttms=[strikes],
            optiontypes_ttms=[np.full(strikes.size, "C")], risk_premia_gammas=risk_premia_gammas, nb_path=nb_path,
            nb_steps_per_year=nb_steps_per_year, seed=seed, recenter_forward=False, **_model_kwargs(params))
        pdf = np.array([(strikes * g["dual_gamma"][0]).reshape(x.shape) for g in out])
        if return_stderr:
            return pdf, np.array([(strikes * g["dual_gamma_stderr"][0]).reshape(x.shape) for g in out])
        return pdf

    def get_log_return_mc_pdf_mixture(self, params: HawkesJDParams, ttm: float, x_grid: np.ndarray, risk_premia_gammas=None,
                                      nb_path: int = 100000, seed: Optional[int] = None, return_stderr: bool = False,
                                      return_stats: bool = False, nb_steps: Optional[int] = None,
                                      variable_type: VariableType = VariableType.LOG_RETURN, comm=None, devices=None):
        """the density of the simulated log-return at x_grid as the mixture of the paths' conditional Gaussians, without a bandwidth
        (logsv_pricer.mixture_log_return_pdf; LogSVPricer.get_log_return_mc_pdf_mixture states the returns): the paths of
        model_mc_price_chain_conditional at this seed, nb_steps steps per year (default NB_STEPS_PER_YEAR), each a Gaussian of
        variance sigma^2 ttm around its jump path.  risk_premia_gammas: get_log_return_mc_pdf_conditional_under_risk_kernel's
        densities, [gamma][x], with one exponential per (path, point) instead of that route's Greeks tail per gamma.  The
        log-return and one GPU only."""
        block = params_block(**_model_kwargs(params))

        def step_rows(eng, rng_seed, call_id):
            eng.step_hawkesjd_chain_cond_rows({"ttms": np.array([float(ttm)]), "m": 1}, np.ascontiguousarray(block, dtype=np.float64),
                                              int(nb_steps or NB_STEPS_PER_YEAR), rng_seed, call_id)
        return mixture_log_return_pdf("HawkesJDPricer.get_log_return_mc_pdf_mixture", step_rows, x_grid, risk_premia_gammas, nb_path, seed,
                                      return_stderr, return_stats, variable_type, comm, devices)

    def model_mc_price_chain_many(self, option_chain: OptionChain, params_list: Sequence[HawkesJDParams], nb_path: int = 100000,
                                  seeds: Optional[Sequence[int]] = None, nb_steps_per_year: int = NB_STEPS_PER_YEAR, **kwargs
                                  ) -> List[Tuple[List[np.ndarray], List[np.ndarray]]]:
        """model_mc_price_chain for several parameter sets, each with its own stream (hawkesjd_mc_chain_pricer_many): job j
        equals model_mc_price_chain(option_chain, params_list[j], seed=seeds[j]) bit for bit"""
        return hawkesjd_mc_chain_pricer_many(params_list=params_list, ttms=option_chain.ttms, forwards=option_chain.forwards,
                                             discfactors=option_chain.discfactors, strikes_ttms=option_chain.strikes_ttms,
                                             optiontypes_ttms=option_chain.optiontypes_ttms, nb_path=nb_path, seeds=seeds,
                                             nb_steps_per_year=nb_steps_per_year, **kwargs)

    def model_mc_price_chain_with_risk_premia_many(self, option_chain: OptionChain, params_list: Sequence[HawkesJDParams],
                                                   nb_path: int = 100000, seeds: Optional[Sequence[int]] = None,
                                                   nb_steps_per_year: int = NB_STEPS_PER_YEAR, **kwargs):
        """model_mc_price_chain_with_risk_premia for several parameter sets, job j under its own params_list[j].risk_premia_gamma
        (hawkesjd_mc_chain_pricer_with_risk_premia_gammas_many at one gamma per job): per job what the single method returns,
        bit for bit; extensions recenter_forward=, return_forwards="""
        params_list = list(params_list)
        if any(p.risk_premia_gamma is None for p in params_list):
            raise ValueError("risk_premia_gamma must be set for the risk-premia pricer")
        out = hawkesjd_mc_chain_pricer_with_risk_premia_gammas_many(
            params_list=params_list, ttms=option_chain.ttms, forwards=option_chain.forwards, discfactors=option_chain.discfactors,
            strikes_ttms=option_chain.strikes_ttms, optiontypes_ttms=option_chain.optiontypes_ttms,
            risk_premia_gammas=[[p.risk_premia_gamma] for p in params_list], nb_path=nb_path, seeds=seeds,
            nb_steps_per_year=nb_steps_per_year, **kwargs)
        return [tuple(o[0] for o in job) for job in out]

    @timer
    def simulate_terminal_values(self, params: HawkesJDParams, ttm: float = 1.0, nb_path: int = 100000,
                                 is_spot_measure: bool = True, **kwargs) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """terminal (x, lambda_p, lambda_m) from (0, lambda_p, lambda_m) (reference :193-227)"""
        p = params.to_dict()
        p.pop("risk_premia_gamma")
        lambda_p, lambda_m = p.pop("lambda_p"), p.pop("lambda_m")
        return simulate_hawkesjd_terminal(ttm=ttm, x0=np.zeros(nb_path), lambda_p0=lambda_p * np.ones(nb_path),
                                          lambda_m0=lambda_m * np.ones(nb_path), nb_path=nb_path, **p,
                                          nb_steps_per_year=kwargs.get("nb_steps_per_year", NB_STEPS_PER_YEAR),
                                          seed=kwargs.get("seed"))

    def model_mc_il_payoff(self, params: HawkesJDParams, ttm: float, p1, p0, pa, pb, nb_path: int = 100000, nb_steps: Optional[int] = None,
                           seed: Optional[int] = None, notional=1000000, return_pieces: bool = False, **kwargs):
        """the Monte Carlo impermanent loss of the range [pa, pb] opened at p0, at the forward p1, under this model: the terminal
        log-returns of simulate_terminal_values stay on the device and svmc_il_payoff reduces them (include/svmc.h: recentred
        spots, value = -(notional0 notional) mean(pay), its standard error).  p1, p0, pa, pb, notional broadcast together and
        share one path set.  nb_steps: the number of time steps (default: the model's daily grid).  Returns (value, stderr), and
        with return_pieces=True a dict of the six piece means, n_kept and n_dropped.  params.risk_premia_gamma is not applied.  A sharded request (comm=, devices=) raises
        NotImplementedError.  Not in the reference, which has no Monte Carlo side for this payoff."""
        from .il_pricer import il_cases, refuse_sharded_il
        refuse_sharded_il("model_mc_il_payoff", kwargs)
        il_cases(p1, p0, pa, pb, notional)                       # ValueError before any device work
        p = params.to_dict()
        p.pop("risk_premia_gamma")
        lambda_p, lambda_m = p.pop("lambda_p"), p.pop("lambda_m")
        eng = hawkesjd_terminal_on_engine(ttm=ttm, x0=np.zeros(nb_path), lambda_p0=lambda_p * np.ones(nb_path),
                                          lambda_m0=lambda_m * np.ones(nb_path), nb_path=nb_path, **p, seed=seed, nb_steps=nb_steps)
        return eng.il_payoffs(p1, p0, pa, pb, notional, return_pieces=return_pieces)

    def get_log_return_mc_pdf_device(self, ttm: float, params: HawkesJDParams, x_grid: np.ndarray, nb_path: int = 100000,
                                     **kwargs) -> np.ndarray:
        """get_log_return_mc_pdf (LOG_RETURN, the model's one priced variable) with the state left on the device and the
        kernel estimate summed there; seed= / nb_steps_per_year= as simulate_terminal_values.  params.risk_premia_gamma is
        IGNORED, as it always was here; only the explicit keyword risk_premia_gamma= (a float or up to 16 gammas) weights the
        estimate by exp(gamma x) -> [n_gammas][n_grid]; return_stats= as engine_log_return_mc_pdf"""
        from .logsv_pricer import engine_log_return_mc_pdf, refuse_sharded_kde
        refuse_sharded_kde("get_log_return_mc_pdf_device", kwargs)
        p = params.to_dict()
        p.pop("risk_premia_gamma")
        lambda_p, lambda_m = p.pop("lambda_p"), p.pop("lambda_m")
        eng = hawkesjd_terminal_on_engine(ttm=ttm, x0=np.zeros(nb_path), lambda_p0=lambda_p * np.ones(nb_path),
                                          lambda_m0=lambda_m * np.ones(nb_path), nb_path=nb_path, **p,
                                          nb_steps_per_year=kwargs.get("nb_steps_per_year", NB_STEPS_PER_YEAR),
                                          seed=kwargs.get("seed"))
        return engine_log_return_mc_pdf(eng, x_grid, kwargs.get("risk_premia_gamma"), kwargs.get("return_stats", False))


# ---- the calibration's codec (reference :246-290): the optimizer's 8-vector <-> HawkesJDParams --------------------------------
# (sigma, mean_p, mean_m, theta_p, theta_m, kappa, beta_p, beta_m)
CALIBRATION_BOUNDS = ((0.10, 2.0), (0.01, 0.99), (-0.99, -0.01), (0.01, 100.0), (0.01, 100.0), (1.0, 100.0), (1.0, 100.0),
                      (1.0, 100.0))


def calibration_start_vector(params0: HawkesJDParams) -> np.ndarray:
    """the start vector of the reference (:251-254), its beta_m0 = (beta2_p - beta2_m) / 2 included"""
    return np.array([params0.sigma, params0.mean_p, params0.mean_m, params0.theta_p, params0.theta_m,
                     0.5 * (params0.kappa_p + params0.kappa_m), 0.5 * (params0.beta1_p - params0.beta2_p),
                     0.5 * (params0.beta2_p - params0.beta2_m)])


def unpack_calibration_vector(pars: np.ndarray, params0: HawkesJDParams) -> HawkesJDParams:
    """the optimizer's vector as model parameters (:258-278): mu = 0, one kappa for both sides, beta2_p = -beta_p,
    beta2_m = -beta_m, shift_p / shift_m / lambda_p / lambda_m from params0"""
    sigma, mean_p, mean_m, theta_p, theta_m, kappa, beta_p, beta_m = (pars[0], pars[1], pars[2], pars[3], pars[4], pars[5],
                                                                      pars[6], pars[7])
    return HawkesJDParams(mu=0.0, sigma=sigma, shift_p=params0.shift_p, mean_p=mean_p, shift_m=params0.shift_m, mean_m=mean_m,
                          lambda_p=params0.lambda_p, theta_p=theta_p, kappa_p=kappa, beta1_p=beta_p, beta2_p=-beta_p,
                          lambda_m=params0.lambda_m, theta_m=theta_m, kappa_m=kappa, beta1_m=beta_m, beta2_m=-beta_m)


def calibration_constraint(pars: np.ndarray, params0: HawkesJDParams) -> float:
    """the inequality constraint (>= 0) of the calibration: the sum of both intensities' stationarity margins (:287-290)"""
    params = unpack_calibration_vector(pars, params0)
    return params.jump1_cond + params.jump2_cond


# ---- the risk-premia calibration's codec (reference :320-335): the optimizer's (sigma, gamma / 8) <-> HawkesJDParams ---------
RISK_PREMIA_GAMMA_SCALER = 8.0
RISK_PREMIA_BOUNDS = ((0.01, 1.5), (-1.0, 1.0))
RISK_PREMIA_FD_STEP = 0.025                   # SLSQP's `eps` in the reference's options


def risk_premia_start_vector(params0: HawkesJDParams) -> np.ndarray:
    return np.array([params0.sigma, params0.risk_premia_gamma / RISK_PREMIA_GAMMA_SCALER])


def unpack_risk_premia_vector(pars: np.ndarray, params0: HawkesJDParams) -> HawkesJDParams:
    """the reference's unpack_pars: sets params0.sigma and params0.risk_premia_gamma IN PLACE and returns params0"""
    params0.sigma = pars[0]
    params0.risk_premia_gamma = RISK_PREMIA_GAMMA_SCALER * pars[1]
    return params0


def risk_premia_calibration_weights(option_chain: OptionChain, market_vols: np.ndarray, is_vega_weighted: bool,
                                    is_unit_ttm_vega: bool) -> np.ndarray:
    """10000 x the per-slice normalised vegas, or 10000 x ones (:316-322)"""
    return 10000.0 * chain_calibration_weights(option_chain, market_vols, is_vega_weighted, is_unit_ttm_vega)


def set_vol_scaler(sigma0: float, ttm: float) -> float:
    """the transform grid's scale from the diffusion volatility (reference :360-362)"""
    return np.clip(sigma0, 0.2, 0.5) * np.sqrt(np.minimum(ttm, 1.0 / 12.0))


def _model_block(model_params: HawkesJDParams) -> np.ndarray:
    return params_block(**model_params.to_dict())


def compute_hawkes_a_mgf_grid(ttm: float, phi_grid: np.ndarray, model_params: HawkesJDParams,
                              psi_grid: Optional[np.ndarray] = None, a_t0: Optional[np.ndarray] = None,
                              is_stiff_solver: bool = False, ode_rtol: Optional[float] = None, ode_atol: Optional[float] = None,
                              **kwargs) -> Tuple[np.ndarray, np.ndarray]:
    """(a_t1 [n, 3], log_mgf [n]) over the grid from a_t0 (reference :518-546).  is_stiff_solver is accepted and answered by the
    same integrator (DOP853 at rtol 1e-10: the tolerance, not the method, decides the answer here)"""
    phi_grid = np.asarray(phi_grid, dtype=np.complex128).ravel()
    psi_grid = np.zeros_like(phi_grid) if psi_grid is None else np.asarray(psi_grid, dtype=np.complex128).ravel()
    grid = AnalyticGrid(phi_grid, psi_grid, 3)
    try:
        if a_t0 is not None:
            grid.set_a(np.asarray(a_t0, dtype=np.complex128).reshape(1, -1, 3))
        grid.hawkes_advance(float(ttm), _model_block(model_params)[None, :], ode_rtol, ode_atol)
        return grid.get_a()[0], grid.get_log_mgf()[0]
    finally:
        grid.close()


def hawkesjd_chain_pricer(model_params: HawkesJDParams, ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                          strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray],
                          is_stiff_solver: bool = False, is_spot_measure: bool = True,
                          variable_type: VariableType = VariableType.LOG_RETURN, vol_scaler: float = None,
                          ode_rtol: Optional[float] = None, ode_atol: Optional[float] = None) -> List[np.ndarray]:
    """analytic chain prices by Fourier inversion of the coefficient-ODE MGF (reference :365-417), a_t0 chained over the
    expiries; ode_rtol / ode_atol: the integrator's tolerances (default 1e-10 / 1e-12).  This is hawkesjd_chain_pricer_batch
    at one set."""
    return hawkesjd_chain_pricer_batch(params_list=[model_params], ttms=ttms, forwards=forwards, discfactors=discfactors,
                                       strikes_ttms=strikes_ttms, optiontypes_ttms=optiontypes_ttms,
                                       is_spot_measure=is_spot_measure, variable_type=variable_type, vol_scaler=vol_scaler,
                                       ode_rtol=ode_rtol, ode_atol=ode_atol)[0]


def hawkesjd_chain_pricer_batch(params_list: Sequence[HawkesJDParams], ttms: np.ndarray, forwards: np.ndarray,
                                discfactors: np.ndarray, strikes_ttms: Sequence[np.ndarray],
                                optiontypes_ttms: Sequence[np.ndarray], is_spot_measure: bool = True,
                                variable_type: VariableType = VariableType.LOG_RETURN, vol_scaler: float = None,
                                ode_rtol: Optional[float] = None, ode_atol: Optional[float] = None) -> List[List[np.ndarray]]:
    """hawkesjd_chain_pricer for SEVERAL parameter sets on one chain: [set][expiry] -> prices, bit-identical to one
    hawkesjd_chain_pricer call per set.  Each set keeps its own transform grid (set_vol_scaler follows its sigma unless
    vol_scaler is given); per expiry the sets advance in one launch and are inverted in one launch, and the chain's sums come
    back in one download.  Not in the reference API: the batched form of a calibration's finite-difference gradient."""
    if int(getattr(variable_type, "value", variable_type)) != LOG_RETURN:
        raise NotImplementedError(f"variable_type={variable_type}")
    ttms = np.asarray(ttms, dtype=np.float64)
    n_sets = len(params_list)
    if n_sets == 0:
        return []
    grids = [mgfp.get_transform_var_grid(variable_type=variable_type, max_phi=MAX_PHI,
                                         vol_scaler=(set_vol_scaler(sigma0=p.sigma, ttm=np.min(ttms))
                                                     if vol_scaler is None else vol_scaler)) for p in params_list]
    rows = np.stack([_model_block(p) for p in params_list])
    grid = AnalyticGrid.acquire([g[0] for g in grids], [g[1] for g in grids], 3)
    try:
        sums = chain_sums(grid, ttms, forwards, strikes_ttms,
                          lambda i, dt: grid.hawkes_advance(float(dt), rows, ode_rtol, ode_atol))
    finally:
        grid.release()
    return chain_prices_from_sums(sums, "vanilla", ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms, is_spot_measure)


def _risk_ttms_forwards(ttms, forwards) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(ttms as float64, the first min(len(ttms), len(forwards)) ttms and forwards): the reference's zip"""
    ttms = np.asarray(ttms, dtype=np.float64)
    forwards = np.asarray(forwards, dtype=np.float64).ravel()
    n = min(len(ttms), forwards.size)
    return ttms, np.ascontiguousarray(ttms.ravel()[:n]), np.ascontiguousarray(forwards[:n])


def hawkesjd_forwards_under_risk_kernel(model_params: HawkesJDParams, risk_premia_gamma: float, ttms: np.ndarray,
                                        forwards: np.ndarray, is_stiff_solver: bool = False, ode_rtol: Optional[float] = None,
                                        ode_atol: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(normalizers, gamma_forwards) of the risk-premia kernel (reference :487-515): per (ttm, forward) of zip(ttms, forwards)
    the coefficient ODEs from zero over the whole [0, ttm] at phi = -gamma and -gamma - 1; normalizer = 1 / exp(Re log E(-gamma)),
    gamma_forward = forward exp(Re log E(-gamma - 1)) normalizer.  Both have the shape of ttms and are pre-filled with ones, so
    entries beyond the shorter of ttms and forwards stay 1.0 (the paper passes forwards=np.array([1.0]) with 12 ttms).  One
    launch (svmc_hawkesjd_risk_forwards_batch); is_stiff_solver is answered by the same integrator, ode_rtol / ode_atol as in
    hawkesjd_chain_pricer."""
    ttms, t, f = _risk_ttms_forwards(ttms, forwards)
    normalizers, gamma_forwards = np.ones_like(ttms), np.ones_like(ttms)
    if t.size == 0:
        return normalizers, gamma_forwards
    lib = _lib.load()
    rows = _model_block(model_params).reshape(1, -1)
    gammas = np.array([float(risk_premia_gamma)])
    buf = DeviceBuffer(2 * t.size)
    try:
        pf = C.POINTER(C.c_double)
        _lib.check(lib.svmc_hawkesjd_risk_forwards_batch(rows.ctypes.data_as(pf), gammas.ctypes.data_as(pf), 1, t.ctypes.data_as(pf),
                                                         f.ctypes.data_as(pf), t.size, buf.ptr, buf.offset(t.size),
                                                         ODE_RTOL if ode_rtol is None else float(ode_rtol),
                                                         ODE_ATOL if ode_atol is None else float(ode_atol), None))
        out = np.empty(2 * t.size)
        _lib.check(lib.svmc_memcpy_d2h(out.ctypes.data, buf.ptr, out.nbytes, None))
        _lib.check(lib.svmc_stream_synchronize(None))
    finally:
        buf.free()
    normalizers.ravel()[:t.size] = out[:t.size]
    gamma_forwards.ravel()[:t.size] = out[t.size:]
    return normalizers, gamma_forwards


def hawkesjd_pdf_under_risk_kernel(model_params: HawkesJDParams, risk_premia_gamma: float, ttm: float, x_grid: np.ndarray,
                                   vol_scaler: float = None, ode_rtol: Optional[float] = None, ode_atol: Optional[float] = None
                                   ) -> np.ndarray:
    """the model density of the log-return under the risk-premia kernel on `x_grid`, as bin masses: exp(gamma x) p(x) normalizer,
    p the bin masses pdf_with_mgf_grid gives from the Hawkes log-MGF on the transform grid of hawkesjd_chain_pricer
    (compute_hawkes_a_mgf_grid over [0, ttm]) and normalizer = 1 / E[exp(gamma x)] from hawkesjd_forwards_under_risk_kernel.
    Host composition of existing launches; the Fourier counterpart of get_log_return_mc_pdf_device(risk_premia_gamma=).  Not in
    the reference API."""
    x_grid = np.asarray(x_grid, dtype=np.float64)
    if vol_scaler is None:
        vol_scaler = set_vol_scaler(sigma0=model_params.sigma, ttm=ttm)
    phi_grid = mgfp.get_transform_var_grid(variable_type=VariableType.LOG_RETURN, max_phi=MAX_PHI, vol_scaler=vol_scaler)[0]
    log_mgf = compute_hawkes_a_mgf_grid(ttm=ttm, phi_grid=phi_grid, model_params=model_params, ode_rtol=ode_rtol,
                                        ode_atol=ode_atol)[1]
    pdf = mgfp.pdf_with_mgf_grid(log_mgf_grid=log_mgf, transform_var_grid=phi_grid, space_grid=x_grid)
    normalizers, _ = hawkesjd_forwards_under_risk_kernel(model_params, risk_premia_gamma, np.array([float(ttm)]), np.array([1.0]),
                                                         ode_rtol=ode_rtol, ode_atol=ode_atol)
    return np.exp(float(risk_premia_gamma) * x_grid) * pdf * normalizers[0]


def hawkesjd_chain_pricer_with_risk_premia(model_params: HawkesJDParams, ttms: np.ndarray, forwards: np.ndarray,
                                           discfactors: np.ndarray, strikes_ttms: Sequence[np.ndarray],
                                           optiontypes_ttms: Sequence[np.ndarray], is_stiff_solver: bool = False,
                                           is_spot_measure: bool = True, variable_type: VariableType = VariableType.LOG_RETURN,
                                           vol_scaler: float = None, ode_rtol: Optional[float] = None,
                                           ode_atol: Optional[float] = None, return_forwards: bool = False):
    """chain prices under the risk-premia kernel of model_params.risk_premia_gamma (reference :420-484): the normalizers and
    gamma forwards of hawkesjd_forwards_under_risk_kernel, the coefficient ODEs chained over the expiries on the transform grid
    of real part -0.5 - gamma (the plain ODE: the reference's risk_premia_gamma= keyword is swallowed by **kwargs), each slice
    by slice_pricer_with_mgf_grid_with_gamma.  discfactors are ignored (undiscounted prices, as in the reference); LOG_RETURN
    only.  Extensions: ode_rtol / ode_atol, and return_forwards=True -> (prices, (normalizers, gamma_forwards)).  This is
    hawkesjd_chain_pricer_with_risk_premia_batch at one set, so the two agree bit for bit."""
    prices, fwds = hawkesjd_chain_pricer_with_risk_premia_batch(
        params_list=[model_params], ttms=ttms, forwards=forwards, discfactors=discfactors, strikes_ttms=strikes_ttms,
        optiontypes_ttms=optiontypes_ttms, is_stiff_solver=is_stiff_solver, is_spot_measure=is_spot_measure,
        variable_type=variable_type, vol_scaler=vol_scaler, ode_rtol=ode_rtol, ode_atol=ode_atol, return_forwards=True)
    return (prices[0], fwds[0]) if return_forwards else prices[0]


def hawkesjd_chain_pricer_with_risk_premia_batch(params_list: Sequence[HawkesJDParams], ttms: np.ndarray, forwards: np.ndarray,
                                                 discfactors: np.ndarray, strikes_ttms: Sequence[np.ndarray],
                                                 optiontypes_ttms: Sequence[np.ndarray], is_stiff_solver: bool = False,
                                                 is_spot_measure: bool = True,
                                                 variable_type: VariableType = VariableType.LOG_RETURN,
                                                 vol_scaler: float = None, ode_rtol: Optional[float] = None,
                                                 ode_atol: Optional[float] = None, return_forwards: bool = False):
    """hawkesjd_chain_pricer_with_risk_premia for SEVERAL parameter sets (each its own sigma and risk_premia_gamma, so its own
    grid: real part -0.5 - gamma, scale from its sigma unless vol_scaler is given) on one chain: [set][expiry] -> prices, and
    with return_forwards=True also [set] -> (normalizers, gamma_forwards).  One forwards launch, then per expiry one advance
    launch and one inversion launch for all sets, then one download.  Everything the reference would reject is rejected on
    the host before any device call.  Not in the reference API: the batched form of the risk-premia calibration's gradient."""
    if int(getattr(variable_type, "value", variable_type)) != LOG_RETURN:
        raise NotImplementedError(f"variable_type={variable_type}")
    n_sets = len(params_list)
    if n_sets == 0:
        return ([], []) if return_forwards else []
    for p in params_list:
        if p.risk_premia_gamma is None:
            raise ValueError("risk_premia_gamma must be set for the risk-premia pricer")
    ttms, t_fwd, f_fwd = _risk_ttms_forwards(ttms, forwards)
    n_exp = min(t_fwd.size, len(strikes_ttms), len(optiontypes_ttms))
    strikes = [np.asarray(k, dtype=np.float64) for k in list(strikes_ttms)[:n_exp]]
    codes = []
    for k, types in zip(strikes, list(optiontypes_ttms)[:n_exp]):   # the slice pricer's ValueErrors, up front
        if k.size and not is_spot_measure:
            raise ValueError("not implemented")
        codes.append(mgfp.gamma_type_codes(np.asarray(types).ravel()))
        if codes[-1].size != k.size:
            raise ValueError("strikes and optiontypes of a slice differ in length")
    gammas = np.array([float(p.risk_premia_gamma) for p in params_list])
    grids = [mgfp.get_transform_var_grid(variable_type=variable_type, max_phi=MAX_PHI,
                                         vol_scaler=(set_vol_scaler(sigma0=p.sigma, ttm=np.min(ttms))
                                                     if vol_scaler is None else vol_scaler), real_phi=-0.5 - g)
             for p, g in zip(params_list, gammas)]
    shortcut = np.array([mgfp.gamma_shortcut(g[0], gm) for g, gm in zip(grids, gammas)], dtype=np.int32)
    rows = np.stack([_model_block(p) for p in params_list])
    normalizers = [np.ones_like(ttms) for _ in params_list]
    gamma_forwards = [np.ones_like(ttms) for _ in params_list]
    out = [[] for _ in params_list]
    if t_fwd.size == 0:
        return (out, list(zip(normalizers, gamma_forwards))) if return_forwards else out
    grid = AnalyticGrid.acquire([g[0] for g in grids], [g[1] for g in grids], 3)
    try:
        grid.risk_forwards(rows, gammas, t_fwd, f_fwd, ode_rtol, ode_atol)
        sums, norms, gfwds = chain_sums(grid, t_fwd, f_fwd, strikes,
                                        lambda i, dt: grid.hawkes_advance(float(dt), rows, ode_rtol, ode_atol),
                                        "gamma", (gammas, shortcut, codes))
    finally:
        grid.release()
    for s in range(n_sets):
        normalizers[s].ravel()[:t_fwd.size] = norms[:, s]
        gamma_forwards[s].ravel()[:t_fwd.size] = gfwds[:, s]
        out[s] = [prices.reshape(k.shape).copy() for prices, k in zip(sums[s], strikes)]
    return (out, list(zip(normalizers, gamma_forwards))) if return_forwards else out


def hawkesjd_mc_chain_pricer(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                             strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray], lambda_p: float,
                             lambda_m: float, mu: float, sigma: float, shift_p: float, mean_p: float, shift_m: float,
                             mean_m: float, theta_p: float, kappa_p: float, beta1_p: float, beta2_p: float, theta_m: float,
                             kappa_m: float, beta1_m: float, beta2_m: float, risk_premia_gamma: float = 0.0,
                             nb_path: int = 100000, variable_type: VariableType = VariableType.LOG_RETURN,
                             nb_steps_per_year: int = NB_STEPS_PER_YEAR, seed: Optional[int] = None, comm=None
                             ) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """chain Monte Carlo (reference :643-711): all expiries in one stepping launch, the state carried over them, payoffs by the
    chain payoff kernels.  risk_premia_gamma is accepted and unused, as in the reference.  comm: the paths sharded over the
    ranks of a communicator that carries a C-ABI session (stochvolmodels_amd.dist); with none given and a default
    communicator of world > 1 this raises rather than price the whole job on every rank."""
    _check_variable_type(variable_type)
    if comm is None and svdist.get_default_comm().world > 1:
        raise NotImplementedError("hawkesjd_mc_chain_pricer: pass comm= explicitly to shard the paths over the ranks")
    if comm is not None and comm.world > 1:
        raise NotImplementedError("hawkesjd_mc_chain_pricer: sharded runs go through the C ABI (svmc_session_set_comm)")
    strikes_ttms = [np.asarray(k, dtype=np.float64) for k in strikes_ttms]
    optiontypes_ttms = [np.asarray(t) for t in optiontypes_ttms]
    block = params_block_of(locals())
    eng = get_engine(int(nb_path))
    rng_seed, call_id = next_rng_call(seed)
    ch = marshalled_chain(np.asarray(ttms), np.asarray(forwards), np.asarray(discfactors), strikes_ttms,
                          [option_type_codes(t) for t in optiontypes_ttms])
    prices, stderrs = eng.price_hawkesjd_chain_fused(ch, block, int(nb_steps_per_year), LOG_RETURN, rng_seed, call_id)
    return chain_shaped(prices, strikes_ttms), chain_shaped(stderrs, strikes_ttms)


def hawkesjd_mc_chain_pricer_conditional(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                                         strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray],
                                         lambda_p: float, lambda_m: float, mu: float, sigma: float, shift_p: float, mean_p: float,
                                         shift_m: float, mean_m: float, theta_p: float, kappa_p: float, beta1_p: float,
                                         beta2_p: float, theta_m: float, kappa_m: float, beta1_m: float, beta2_m: float,
                                         risk_premia_gamma: float = 0.0, nb_path: int = 100000,
                                         variable_type: VariableType = VariableType.LOG_RETURN,
                                         nb_steps_per_year: int = NB_STEPS_PER_YEAR, seed: Optional[int] = None, comm=None,
                                         devices=None, recenter: bool = True, return_stats: bool = False):
    """hawkesjd_mc_chain_pricer by CONDITIONAL Monte Carlo (include/svmc.h): the diffusion sigma w0 is independent
    of the jumps and the intensities, so given a path's jumps the discretised log-return is Gaussian with one variance sigma^2 T for
    every path, and each path contributes a Black-76 price instead of a payoff -- the same expectation for the same discretised
    model, a smaller variance, no normal drawn (random streams 9 and 10, not the plain pricer's: the two are independent estimates
    at equal seeds).  Same signature and (prices, stderrs) lists; return_stats=True adds per expiry the dict of
    engine.CMC_STATS_FIELDS.  recenter=False prices against the unrecentred strikes.  risk_premia_gamma is accepted and unused, as
    in the plain pricer.  'C' / 'P', LOG_RETURN and one GPU only (logsv_pricer.check_conditional_request).  Not in the reference
    API."""
    codes = check_conditional_request("hawkesjd_mc_chain_pricer_conditional", variable_type, comm, devices, optiontypes_ttms)
    block = params_block_of(locals())
    rng_seed, call_id = next_rng_call(seed)
    ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, codes)
    prices, stderrs, stats = get_engine(int(nb_path)).price_hawkesjd_chain_cmc_fused(ch, block, int(nb_steps_per_year), recenter,
                                                                                     rng_seed, call_id)
    out = (chain_shaped(prices, strikes_ttms), chain_shaped(stderrs, strikes_ttms))
    return out + (stats,) if return_stats else out


def hawkesjd_mc_chain_greeks_conditional(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                                         strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray],
                                         lambda_p: float, lambda_m: float, mu: float, sigma: float, shift_p: float, mean_p: float,
                                         shift_m: float, mean_m: float, theta_p: float, kappa_p: float, beta1_p: float,
                                         beta2_p: float, theta_m: float, kappa_m: float, beta1_m: float, beta2_m: float,
                                         risk_premia_gamma: float = 0.0, nb_path: int = 100000,
                                         variable_type: VariableType = VariableType.LOG_RETURN,
                                         nb_steps_per_year: int = NB_STEPS_PER_YEAR, seed: Optional[int] = None, comm=None,
                                         devices=None, recenter: bool = True, return_stats: bool = False,
                                         wrt: Optional[Sequence[str]] = ()) -> dict:
    """hawkesjd_mc_chain_pricer_conditional with the derivatives of its prices in the forward and the strike (DESIGN.md rows f13,
    f16): a dict of chain-shaped lists -- price, stderr (bit-equal to hawkesjd_mc_chain_pricer_conditional at the same seed), delta,
    dual_delta, gamma, dual_gamma, each with its _stderr -- and with return_stats=True "stats", per expiry the dict of
    engine.CMC_GREEKS_STATS_FIELDS.  sigma = 0 makes every path a point mass: both gammas are then 0.  Parameter sensitivities are
    not built: a non-empty wrt raises NotImplementedError.  Refusals: hawkesjd_mc_chain_pricer_conditional's.  Not in the reference
    API."""
    who = "hawkesjd_mc_chain_greeks_conditional"
    codes = check_conditional_request(who, variable_type, comm, devices, optiontypes_ttms)
    if wrt is None or isinstance(wrt, str) or len(wrt) > 0:
        raise NotImplementedError(f"{who}: wrt=: parameter sensitivities of the Hawkes conditional estimator are not covered")
    block = params_block_of(locals())
    rng_seed, call_id = next_rng_call(seed)
    ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, codes)
    fields, stats = get_engine(int(nb_path)).price_hawkesjd_chain_cmc_greeks_fused(ch, block, int(nb_steps_per_year), recenter,
                                                                                   rng_seed, call_id)
    return conditional_greeks_shaped(fields, stats, strikes_ttms, return_stats)


def hawkesjd_mc_chain_pricer_with_risk_premia_gammas(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                                                     strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray],
                                                     lambda_p: float, lambda_m: float, mu: float, sigma: float, shift_p: float,
                                                     mean_p: float, shift_m: float, mean_m: float, theta_p: float,
                                                     kappa_p: float, beta1_p: float, beta2_p: float, theta_m: float,
                                                     kappa_m: float, beta1_m: float, beta2_m: float,
                                                     risk_premia_gammas: Sequence[float] = (0.0,), nb_path: int = 100000,
                                                     variable_type: VariableType = VariableType.LOG_RETURN,
                                                     nb_steps_per_year: int = NB_STEPS_PER_YEAR, seed: Optional[int] = None,
                                                     recenter_forward: bool = False, return_forwards: bool = False, comm=None,
                                                     devices=None, risk_premia_gamma=None):
    """Monte Carlo chain prices under the exponential risk-premia kernel exp(gamma x) for SEVERAL gammas from ONE stepping launch
    (svmc_hawkesjd_chain_price_tilted): the paths of hawkesjd_mc_chain_pricer on this seed, then per gamma the weighted payoff
    reduction of include/svmc.h (svmc_tilted_payoff_chain: the estimator, its keep rule and its delta-method errors) on the
    resident snapshots -- no path leaves the device.  Returns (prices, stderrs), each [gamma][expiry] in the strikes' shapes;
    with return_forwards=True a third item [gamma] -> (normalizers, gamma_forwards, stats), the Monte Carlo counterparts of
    hawkesjd_forwards_under_risk_kernel per expiry and stats [n_expiries, 8] in the order of engine.TILTED_STATS_FIELDS
    (normalizer, its error, gamma forward, its error, effective sample size, n_kept, n_dropped, sum of weights).
    Prices are UNDISCOUNTED like the Fourier risk-premia pricer's: discfactors are accepted and ignored.  'C' / 'P' only (others:
    ValueError("not implemented")), LOG_RETURN only.  recenter_forward: spot = F exp(x) - (nanmean(F exp(x)) - F), as
    compute_mc_vars_payoff recentres; gamma = 0 with it is hawkesjd_mc_chain_pricer at discount factors 1.  A gamma's results
    are the same bits whichever other gammas share the call.  risk_premia_gamma= is accepted and unused here (the keyword of
    HawkesJDParams.to_dict()).
    Against the Fourier pricer: hawkesjd_chain_pricer_with_risk_premia multiplies its capped sum by K^(1+gamma), not
    K^(1+gamma) F^(-gamma), so it equals the payoff expectation priced here only at F = 1 (the paper's case); this function
    prices the payoff as written for any F."""
    _check_variable_type(variable_type)
    _refuse_sharded("hawkesjd_mc_chain_pricer_with_risk_premia", comm, devices)
    strikes_ttms = [np.asarray(k, dtype=np.float64) for k in strikes_ttms]
    codes = [tilted_type_codes(t) for t in optiontypes_ttms]                # ValueError("not implemented")
    ch = tilted_chain_arrays(forwards, strikes_ttms, codes, risk_premia_gammas, ttms=ttms)
    block = params_block_of(locals())
    eng = get_engine(int(nb_path))
    rng_seed, call_id = next_rng_call(seed)
    prices, stderrs, stats = eng.price_hawkesjd_chain_tilted_fused(ch, block, int(nb_steps_per_year), rng_seed, call_id,
                                                                   ch["gammas"], bool(recenter_forward))
    if not return_forwards:
        return prices, stderrs
    return prices, stderrs, forwards_triples(stats)


def hawkesjd_mc_chain_pricer_with_risk_premia(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                                              strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray],
                                              risk_premia_gamma: float = None, nb_path: int = 100000,
                                              nb_steps_per_year: int = NB_STEPS_PER_YEAR, seed: Optional[int] = None,
                                              recenter_forward: bool = False, return_forwards: bool = False, **kwargs):
    """hawkesjd_mc_chain_pricer_with_risk_premia_gammas at ONE gamma, so the two agree bit for bit: (prices, stderrs) per
    expiry, with return_forwards=True also (normalizers, gamma_forwards, stats).  kwargs: the model parameters (and
    variable_type=, comm=, devices=) of that function."""
    return tuple(o[0] for o in _at_one_gamma(hawkesjd_mc_chain_pricer_with_risk_premia_gammas, locals()))


def hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                                                                 strikes_ttms: Sequence[np.ndarray],
                                                                 optiontypes_ttms: Sequence[np.ndarray], lambda_p: float,
                                                                 lambda_m: float, mu: float, sigma: float, shift_p: float,
                                                                 mean_p: float, shift_m: float, mean_m: float, theta_p: float,
                                                                 kappa_p: float, beta1_p: float, beta2_p: float, theta_m: float,
                                                                 kappa_m: float, beta1_m: float, beta2_m: float,
                                                                 risk_premia_gammas: Sequence[float] = (0.0,),
                                                                 nb_path: int = 100000,
                                                                 variable_type: VariableType = VariableType.LOG_RETURN,
                                                                 nb_steps_per_year: int = NB_STEPS_PER_YEAR,
                                                                 seed: Optional[int] = None, recenter_forward: bool = False,
                                                                 return_forwards: bool = False, comm=None, devices=None,
                                                                 risk_premia_gamma=None):
    """hawkesjd_mc_chain_pricer_with_risk_premia_gammas by CONDITIONAL Monte Carlo (include/svmc_ext.h): given a
    path's jumps x ~ N(mu, sigma^2 T), and the Esscher identity turns exp(gamma x) payoff(x) into the weight
    exp(gamma mu + gamma^2 cv / 2) -- no diffusion noise in it -- times a Black-76 price at the forward shifted by gamma cv.  The
    paths are those of hawkesjd_mc_chain_pricer_conditional at this seed (streams 9 and 10 of (seed, call id): no normal is drawn,
    and the mu rows are bit-equal to that pricer's), stepped ONCE for all gammas; then svmc_tilted_cond_payoff_chain on the
    resident rows.  Two C calls, not one: sessions belong to the closed core, the tail to the library beside it.
    Signature, return shapes and return_forwards= are hawkesjd_mc_chain_pricer_with_risk_premia_gammas's: (prices, stderrs), each
    [gamma][expiry] in the strikes' shapes, and with return_forwards=True a third item [gamma] -> (normalizers, gamma_forwards,
    stats [n_expiries, 8] in the order of engine.TILTED_COND_STATS_FIELDS).  Prices are UNDISCOUNTED: discfactors are accepted
    and ignored.  recenter_forward: K + (mean F exp(mu + cv / 2) - F), the conditional pricer's recentring, the same number
    whatever gamma is.  'C' / 'P' only (others: ValueError("not implemented")), LOG_RETURN only, one GPU only
    (NotImplementedError), each refused before any engine is asked for.  risk_premia_gamma= is accepted and unused here.  Not in
    the reference API."""
    codes = check_conditional_request("hawkesjd_mc_chain_pricer_conditional_with_risk_premia", variable_type, comm, devices,
                                      optiontypes_ttms)
    strikes_ttms = [np.asarray(k, dtype=np.float64) for k in strikes_ttms]
    ch = tilted_chain_arrays(forwards, strikes_ttms, codes, risk_premia_gammas, ttms=ttms)
    block = params_block_of(locals())
    eng = get_engine(int(nb_path))
    rng_seed, call_id = next_rng_call(seed)
    prices, stderrs, stats = eng.price_hawkesjd_chain_tilted_cond(ch, block, int(nb_steps_per_year), rng_seed, call_id, ch["gammas"],
                                                                  bool(recenter_forward))
    if not return_forwards:
        return prices, stderrs
    return prices, stderrs, forwards_triples(stats)


def jump_sets_request(sigmas, risk_premia_gammas) -> Tuple[np.ndarray, np.ndarray]:
    """the (sigma, gamma) sets of one request as two float64 vectors of one length >= 1: ValueError for unequal lengths, a negative
    or non-finite sigma, a non-finite gamma"""
    s = np.atleast_1d(np.asarray(sigmas, dtype=np.float64)).ravel()
    g = np.atleast_1d(np.asarray(risk_premia_gammas, dtype=np.float64)).ravel()
    if s.size != g.size or s.size < 1:
        raise ValueError(f"one sigma and one risk-premia gamma per set, got {s.size} and {g.size}")
    if not (np.all(np.isfinite(s)) and np.all(s >= 0.0)):
        raise ValueError("sigmas must be finite and not negative")
    if not np.all(np.isfinite(g)):
        raise ValueError("risk-premia gammas must be finite")
    return s, g


# (steps, dt) per expiry: the fused drivers' grid, the one engine.step_hawkesjd_chain_cond_rows steps on
jump_step_grid = chain_step_grid


def jump_sets_variances(sigma: float, nb_steps: Sequence[int], dts: Sequence[float]) -> np.ndarray:
    """v_i = cv_i(sigma) per expiry by the host formula of svmc_hawkesjd_chain_cond (include/svmc.h): cv_i = cv_{i-1} +
    nb_steps_i (sigma sigma dt_i) in double, in slice order from 0, each product and sum rounded once -- the bits of that entry's
    cv row"""
    sigma2 = float(sigma) * float(sigma)
    out, cv = [], 0.0
    for nb, dt in zip(nb_steps, dts):
        cv = cv + float(int(nb)) * (sigma2 * float(dt))
        out.append(cv)
    return np.array(out, dtype=np.float64)


class HawkesJumpRows:
    """The jump rows of a Hawkes chain, stepped ONCE (hawkesjd_jump_rows): per expiry a_j = drift, compensators and jumps of path j,
    which depend on neither sigma nor risk_premia_gamma, in a device buffer of its own (m x nb_path doubles: no other call on the
    engine writes it), with the step grid, so that every (sigma, gamma) is priced by price_sets without another stepping launch
    (include/svmc_est.h svmc_jump_sets_payoff_chain)."""

    def __init__(self, engine, rows: DeviceBuffer, ttms: np.ndarray, nb_steps: Sequence[int], dts: Sequence[float], seed: int,
                 call_id: int):
        self.engine, self.rows = engine, rows
        self.ttms = np.array(ttms, dtype=np.float64)
        self.nb_steps, self.dts = [int(n) for n in nb_steps], [float(d) for d in dts]
        self.nb_path, self.seed, self.call_id = int(engine.n_path), int(seed), int(call_id)

    @property
    def n_expiries(self) -> int:
        return self.ttms.size

    def row_ptrs(self) -> List[int]:
        return [self.rows.offset(i * self.nb_path) for i in range(self.n_expiries)]

    def variances(self, sigma: float) -> np.ndarray:
        """v_i(sigma) per expiry: jump_sets_variances on this handle's step grid"""
        return jump_sets_variances(sigma, self.nb_steps, self.dts)

    def numpy(self) -> np.ndarray:
        """the rows on the host, [n_expiries, nb_path]"""
        return self.engine.download(self.rows.ptr, self.n_expiries * self.nb_path).reshape(self.n_expiries, self.nb_path)

    def price_sets(self, sigmas, risk_premia_gammas, forwards, strikes_ttms: Sequence[np.ndarray],
                   optiontypes_ttms: Sequence[np.ndarray], recenter_forward: bool = False, return_forwards: bool = False):
        """the chain under exp(gamma x) by conditional Monte Carlo at every (sigma_q, gamma_q) on these rows: (prices, stderrs), each
        [set][expiry] in the strikes' shapes, undiscounted; with return_forwards=True a third item [set] -> (normalizers,
        gamma_forwards, stats [n_expiries, 8] in the order of engine.TILTED_COND_STATS_FIELDS), as
        hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas returns per gamma.  Any number of sets: calls of
        engine.JUMP_SETS_MAX; a set's numbers are the same bits whichever others share the request.  'C' / 'P' only."""
        codes = [tilted_type_codes(t) for t in optiontypes_ttms]            # ValueError("not implemented")
        s, g = jump_sets_request(sigmas, risk_premia_gammas)
        strikes_ttms = [np.asarray(k, dtype=np.float64) for k in strikes_ttms]
        if len(strikes_ttms) != self.n_expiries:
            raise ValueError("chain arrays must have one entry per maturity of the rows")
        var = np.array([self.variances(x) for x in s]).reshape(s.size, self.n_expiries)
        prices, stderrs, extra = [], [], []
        for q0 in range(0, s.size, JUMP_SETS_MAX):
            sl = slice(q0, q0 + JUMP_SETS_MAX)
            p, e, stats, _ = self.engine.jump_sets_payoffs(forwards, strikes_ttms, codes, var[sl], g[sl], bool(recenter_forward),
                                                           a_ptrs=self.row_ptrs())
            prices += p
            stderrs += e
            extra += forwards_triples(stats)
        return (prices, stderrs, extra) if return_forwards else (prices, stderrs)

    def free(self) -> None:
        self.rows.free()


def hawkesjd_jump_rows(ttms: np.ndarray, lambda_p: float, lambda_m: float, mu: float, shift_p: float, mean_p: float, shift_m: float,
                       mean_m: float, theta_p: float, kappa_p: float, beta1_p: float, beta2_p: float, theta_m: float, kappa_m: float,
                       beta1_m: float, beta2_m: float, sigma: float = 0.0, risk_premia_gamma=None, nb_path: int = 100000,
                       nb_steps_per_year: int = NB_STEPS_PER_YEAR, seed: Optional[int] = None, comm=None, devices=None
                       ) -> HawkesJumpRows:
    """step the jump part of the Hawkes chain ONCE for every (sigma, gamma): in the conditional step the jump
    decisions, the jump sizes and both intensities depend on neither, and sigma enters a path's conditional mean only through the
    deterministic -sigma^2 dt / 2 of every step, so svmc_hawkesjd_chain_cond at sigma = 0 leaves rows a_j with
    x_T | jumps ~ N(a_j - v / 2, v), v = cv_i(sigma) one host number per expiry.  The jumps are those of
    hawkesjd_mc_chain_pricer_conditional(_with_risk_premia) at this seed (streams 9 and 10).  sigma and risk_premia_gamma are
    accepted and unused.  Returns a HawkesJumpRows; one GPU only (NotImplementedError).  Chains longer than 16 expiries step in
    launches of 16."""
    refuse_sharded_paths("hawkesjd_jump_rows", comm, devices)
    t = np.ascontiguousarray(np.asarray(ttms, dtype=np.float64)).ravel()
    if t.size < 1:
        raise ValueError("at least one expiry")
    nbs, dts = jump_step_grid(t, nb_steps_per_year)
    block = params_block_of(dict(locals(), sigma=0.0))
    eng = get_engine(int(nb_path))
    rng_seed, call_id = next_rng_call(seed)
    m, n = t.size, int(nb_path)
    eng.step_hawkesjd_jump_rows({"ttms": t, "m": m}, block, int(nb_steps_per_year), rng_seed, call_id)
    rows = DeviceBuffer(m * n)
    # the snapshot rows are shared with every other call on the engine: the handle keeps its own copy
    eng.copy_rows(rows.ptr, eng.snapshot_ptr(0), m * n)
    eng.synchronize()
    return HawkesJumpRows(eng, rows, t, nbs, dts, rng_seed, call_id)


def hawkesjd_mc_chain_pricer_conditional_sets(sigmas, risk_premia_gammas, ttms: np.ndarray, forwards: np.ndarray,
                                              discfactors: np.ndarray, strikes_ttms: Sequence[np.ndarray],
                                              optiontypes_ttms: Sequence[np.ndarray], lambda_p: float, lambda_m: float, mu: float,
                                              shift_p: float, mean_p: float, shift_m: float, mean_m: float, theta_p: float,
                                              kappa_p: float, beta1_p: float, beta2_p: float, theta_m: float, kappa_m: float,
                                              beta1_m: float, beta2_m: float, sigma=None, risk_premia_gamma=None,
                                              nb_path: int = 100000, variable_type: VariableType = VariableType.LOG_RETURN,
                                              nb_steps_per_year: int = NB_STEPS_PER_YEAR, seed: Optional[int] = None,
                                              recenter_forward: bool = False, return_forwards: bool = False, comm=None,
                                              devices=None):
    """hawkesjd_mc_chain_pricer_conditional_with_risk_premia at EVERY (sigma_q, gamma_q) of two sequences of one length from ONE
    stepping launch: one hawkesjd_jump_rows plus one HawkesJumpRows.price_sets.  At one seed a set's prices
    differ from that pricer's at (sigma_q, gamma_q) by the rounding of the paths' conditional means only: the jumps are the same.
    Returns as price_sets; prices are UNDISCOUNTED: discfactors are accepted and ignored.  sigma= and risk_premia_gamma= (the
    parameter set's own) are accepted and unused.  'C' / 'P' only (others: ValueError("not implemented")), LOG_RETURN only, one GPU
    only (NotImplementedError); a ValueError for sequences of unequal length, a negative or non-finite sigma, a non-finite gamma;
    each raised before any engine is asked for.  Not in the reference API."""
    check_conditional_request("hawkesjd_mc_chain_pricer_conditional_sets", variable_type, comm, devices, optiontypes_ttms)
    s, g = jump_sets_request(sigmas, risk_premia_gammas)
    strikes_ttms = [np.asarray(k, dtype=np.float64) for k in strikes_ttms]
    tilted_chain_arrays(forwards, strikes_ttms, [tilted_type_codes(t) for t in optiontypes_ttms], g[:1], ttms=ttms)    # the chain's checks
    rows = hawkesjd_jump_rows(ttms, lambda_p=lambda_p, lambda_m=lambda_m, mu=mu, shift_p=shift_p, mean_p=mean_p, shift_m=shift_m,
                              mean_m=mean_m, theta_p=theta_p, kappa_p=kappa_p, beta1_p=beta1_p, beta2_p=beta2_p, theta_m=theta_m,
                              kappa_m=kappa_m, beta1_m=beta1_m, beta2_m=beta2_m, nb_path=nb_path,
                              nb_steps_per_year=nb_steps_per_year, seed=seed)
    try:
        return rows.price_sets(s, g, forwards, strikes_ttms, optiontypes_ttms, recenter_forward, return_forwards)
    finally:
        rows.free()


def hawkesjd_mc_chain_pricer_conditional_with_risk_premia(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                                                          strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray],
                                                          risk_premia_gamma: float = None, nb_path: int = 100000,
                                                          nb_steps_per_year: int = NB_STEPS_PER_YEAR, seed: Optional[int] = None,
                                                          recenter_forward: bool = False, return_forwards: bool = False, **kwargs):
    """hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas at ONE gamma, so the two agree bit for bit: (prices, stderrs)
    per expiry, with return_forwards=True also (normalizers, gamma_forwards, stats).  kwargs: the model parameters (and
    variable_type=, comm=, devices=) of that function."""
    return tuple(o[0] for o in _at_one_gamma(hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas, locals()))


def hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                                                                 strikes_ttms: Sequence[np.ndarray],
                                                                 optiontypes_ttms: Sequence[np.ndarray], lambda_p: float,
                                                                 lambda_m: float, mu: float, sigma: float, shift_p: float,
                                                                 mean_p: float, shift_m: float, mean_m: float, theta_p: float,
                                                                 kappa_p: float, beta1_p: float, beta2_p: float, theta_m: float,
                                                                 kappa_m: float, beta1_m: float, beta2_m: float,
                                                                 risk_premia_gammas: Sequence[float] = (0.0,),
                                                                 nb_path: int = 100000,
                                                                 variable_type: VariableType = VariableType.LOG_RETURN,
                                                                 nb_steps_per_year: int = NB_STEPS_PER_YEAR,
                                                                 seed: Optional[int] = None, recenter_forward: bool = False,
                                                                 return_stats: bool = False, comm=None, devices=None,
                                                                 risk_premia_gamma=None, wrt: Optional[Sequence[str]] = ()) -> list:
    """hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas with the derivatives of its prices in the forward and the
    strike (include/svmc_est.h).  The weight exp(gamma mu + gamma^2 cv / 2) depends on neither, so each
    derivative is the weighted mean of a per-path Black-76 derivative at the shifted forward, with the ratio estimator's error: the
    EXACT derivatives of the price that pricer returns at the same seed.  The arguments are that pricer's, return_stats= in the
    place of return_forwards=.  Returns one dict per gamma of chain-shaped lists with the ten keys of engine.CMC_GREEKS_FIELDS:
    price, stderr (bit-equal to the conditional pricer under the kernel at the seed), delta, dual_delta, gamma, dual_gamma, each
    with its _stderr; with return_stats=True also "stats", per expiry the dict of engine.TILTED_COND_GREEKS_STATS_FIELDS (that
    pricer's block and n_zero_cv, the kept paths whose conditional variance is zero: they add no gamma).  All values are
    UNDISCOUNTED.  price = F delta + K dual_delta and F^2 gamma = K^2 dual_gamma hold to rounding; with recenter_forward the
    errors ignore the noise of the recentring mean, as the price's does.  ONE stepping call for all gammas, then the two tails
    (libsvmc_ext.so's for price and error, libsvmc_est.so's for the derivatives).  Refusals, each before any engine is asked for:
    that pricer's ('IC' / 'IP', variables other than the log-return, comm= / devices=) and any wrt= but the default () (parameter
    sensitivities under the kernel are not built: NotImplementedError).  wrt=None is refused too: in the sibling routes
    (logsv_mc_chain_greeks_conditional, hawkesjd_mc_chain_greeks_conditional) None and "all" ask for EVERY parameter, so it is a
    request, not its absence.  risk_premia_gamma= is accepted and unused, as in that pricer: it is there only so that
    **params.to_dict() can be passed; the gammas are risk_premia_gammas.  Not in the reference API."""
    who = "hawkesjd_mc_chain_greeks_conditional_with_risk_premia"
    codes = check_conditional_request(who, variable_type, comm, devices, optiontypes_ttms)
    if wrt is None or isinstance(wrt, str) or len(wrt) > 0:
        raise NotImplementedError(f"{who}: wrt=: parameter sensitivities under the risk-premia kernel are not covered")
    strikes_ttms = [np.asarray(k, dtype=np.float64) for k in strikes_ttms]
    ch = tilted_chain_arrays(forwards, strikes_ttms, codes, risk_premia_gammas, ttms=ttms)
    block = params_block_of(locals())
    eng = get_engine(int(nb_path))
    rng_seed, call_id = next_rng_call(seed)
    fields, stats = eng.price_hawkesjd_chain_tilted_cond_greeks(ch, block, int(nb_steps_per_year), rng_seed, call_id, ch["gammas"],
                                                                bool(recenter_forward))
    out = [dict(f) for f in fields]
    if return_stats:
        for d, st in zip(out, stats):
            d["stats"] = tilted_greeks_stats_dicts(st)
    return out


def hawkesjd_mc_chain_greeks_conditional_with_risk_premia(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                                                          strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray],
                                                          risk_premia_gamma: float = None, nb_path: int = 100000,
                                                          nb_steps_per_year: int = NB_STEPS_PER_YEAR, seed: Optional[int] = None,
                                                          recenter_forward: bool = False, return_stats: bool = False, **kwargs) -> dict:
    """hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas at ONE gamma, so the two agree bit for bit: its dict.  kwargs:
    the model parameters (and variable_type=, comm=, devices=, wrt=) of that function."""
    return _at_one_gamma(hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas, locals())[0]


def _model_kwargs(params: HawkesJDParams) -> Dict[str, Any]:
    """the keyword parameters of the single Monte Carlo pricers from a parameter set (risk_premia_gamma left out)"""
    kw = params.to_dict()
    kw.pop("risk_premia_gamma", None)
    return kw


def _refuse_sharded(name: str, comm, devices) -> None:
    """the tilted pricers and the many-job ones run on one device only"""
    if devices is not None or (comm.world if comm is not None else svdist.get_default_comm().world) > 1:
        raise NotImplementedError(f"{name}: not sharded over ranks or devices")


def hawkesjd_mc_chain_pricer_many(params_list: Sequence[HawkesJDParams], ttms: np.ndarray, forwards: np.ndarray,
                                  discfactors: np.ndarray, strikes_ttms: Sequence[np.ndarray],
                                  optiontypes_ttms: Sequence[np.ndarray], nb_path: int = 100000,
                                  variable_type: VariableType = VariableType.LOG_RETURN,
                                  nb_steps_per_year: int = NB_STEPS_PER_YEAR, seeds: Optional[Sequence[int]] = None, comm=None,
                                  devices=None) -> List[Tuple[List[np.ndarray], List[np.ndarray]]]:
    """hawkesjd_mc_chain_pricer for several independent jobs of ONE chain, as logsv_mc_chain_pricer_many: job j has the
    parameters params_list[j] (its start intensities lambda_p, lambda_m included) and its own random stream -- seeds[j] (call id
    0), or with seeds=None the process seed and the next call id, taken in list order.  Returns [(prices, stderrs)] per job, each
    BIT-EQUAL to hawkesjd_mc_chain_pricer(..., seed=seeds[j]) (or to the j-th of as many consecutive unseeded calls).  Up to
    MANY_MAX_JOBS jobs are stepped by ONE launch (svmc_hawkesjd_chain_price_many; longer lists in several calls, in order); more
    than 16 expiries is a loop of single calls -- the same numbers.  Sharded requests (devices=, a world above one) raise as the
    single pricer does; params' risk_premia_gamma is ignored, as there.  Not in the reference API."""
    params_list = check_many_args(params_list, seeds)
    if not params_list:
        return []
    _check_variable_type(variable_type)
    _refuse_sharded("hawkesjd_mc_chain_pricer_many", comm, devices)
    strikes_ttms = [np.asarray(k, dtype=np.float64) for k in strikes_ttms]
    optiontypes_ttms = [np.asarray(t) for t in optiontypes_ttms]
    if len(ttms) > 16:
        return [hawkesjd_mc_chain_pricer(ttms=ttms, forwards=forwards, discfactors=discfactors, strikes_ttms=strikes_ttms,
                                         optiontypes_ttms=optiontypes_ttms, nb_path=nb_path, variable_type=variable_type,
                                         nb_steps_per_year=nb_steps_per_year, seed=None if seeds is None else seeds[j],
                                         **_model_kwargs(p))
                for j, p in enumerate(params_list)]
    streams = many_job_streams(len(params_list), seeds)
    rows = np.stack([_model_block(p) for p in params_list])
    ch = marshalled_chain(np.asarray(ttms), np.asarray(forwards), np.asarray(discfactors), strikes_ttms,
                          [option_type_codes(t) for t in optiontypes_ttms])
    eng = get_engine(int(nb_path))
    out = []
    for _, part, job_seeds, ids in many_job_chunks(streams, rows):
        out += eng.price_chain_many_fused(ch, "hawkesjd", part, job_seeds, ids, 0, int(nb_steps_per_year), LOG_RETURN)
    return many_jobs_shaped(out, strikes_ttms)


def many_job_gammas(risk_premia_gammas, n_jobs: int) -> np.ndarray:
    """the gammas of a many-job tilted call as [n_jobs][n_gammas]: one flat sequence shared by all jobs, or one sequence per job,
    all of the same length (1 .. TILTED_MAX_GAMMAS finite values each); anything else raises ValueError"""
    g = list(risk_premia_gammas)
    per_job = len(g) > 0 and all(np.ndim(v) > 0 for v in g)
    if not per_job:
        if any(np.ndim(v) > 0 for v in g):
            raise ValueError("risk_premia_gammas: one flat sequence, or one sequence per job")
        return np.tile(tilted_gammas(g), (n_jobs, 1))
    if len(g) != n_jobs:
        raise ValueError(f"risk_premia_gammas has {len(g)} rows for {n_jobs} parameter sets")
    rows = [tilted_gammas(v) for v in g]
    if any(r.size != rows[0].size for r in rows):
        raise ValueError("risk_premia_gammas: every job needs the same number of gammas")
    return np.ascontiguousarray(np.stack(rows))


def hawkesjd_mc_chain_pricer_with_risk_premia_gammas_many(params_list: Sequence[HawkesJDParams], ttms: np.ndarray,
                                                          forwards: np.ndarray, discfactors: np.ndarray,
                                                          strikes_ttms: Sequence[np.ndarray],
                                                          optiontypes_ttms: Sequence[np.ndarray],
                                                          risk_premia_gammas: Sequence = (0.0,), nb_path: int = 100000,
                                                          variable_type: VariableType = VariableType.LOG_RETURN,
                                                          nb_steps_per_year: int = NB_STEPS_PER_YEAR,
                                                          recenter_forward: bool = False, return_forwards: bool = False,
                                                          seeds: Optional[Sequence[int]] = None, comm=None, devices=None) -> list:
    """hawkesjd_mc_chain_pricer_with_risk_premia_gammas for several independent jobs of ONE chain: ONE stepping launch for all
    jobs (svmc_hawkesjd_chain_price_tilted_many), then each job's weighted payoff reduction on its own snapshots.
    risk_premia_gammas: one flat sequence shared by all jobs, or one sequence per job, all of the same length.  Returns per job
    what the single function returns for (params_list[j], seeds[j], its gammas) -- (prices, stderrs), with return_forwards=True a
    third item [gamma] -> (normalizers, gamma_forwards, stats) -- bit for bit; streams as hawkesjd_mc_chain_pricer_many.  The
    single function's checks: 'C' / 'P' only (ValueError("not implemented")), LOG_RETURN only, not sharded; discfactors and the
    params' risk_premia_gamma are accepted and ignored.  More than 16 expiries is a loop of single calls."""
    params_list = check_many_args(params_list, seeds)
    if not params_list:
        return []
    _check_variable_type(variable_type)
    _refuse_sharded("hawkesjd_mc_chain_pricer_with_risk_premia_gammas_many", comm, devices)
    gammas = many_job_gammas(risk_premia_gammas, len(params_list))
    strikes_ttms = [np.asarray(k, dtype=np.float64) for k in strikes_ttms]
    codes = [tilted_type_codes(t) for t in optiontypes_ttms]                # ValueError("not implemented")
    ch = tilted_chain_arrays(forwards, strikes_ttms, codes, gammas[0], ttms=ttms)
    if ch["m"] > 16:
        return [hawkesjd_mc_chain_pricer_with_risk_premia_gammas(
            ttms=ttms, forwards=forwards, discfactors=discfactors, strikes_ttms=strikes_ttms, optiontypes_ttms=optiontypes_ttms,
            risk_premia_gammas=gammas[j], nb_path=nb_path, variable_type=variable_type, nb_steps_per_year=nb_steps_per_year,
            seed=None if seeds is None else seeds[j], recenter_forward=recenter_forward, return_forwards=return_forwards,
            **_model_kwargs(p)) for j, p in enumerate(params_list)]
    streams = many_job_streams(len(params_list), seeds)
    rows = np.stack([_model_block(p) for p in params_list])
    eng = get_engine(int(nb_path))
    out = []
    for q0, part, job_seeds, ids in many_job_chunks(streams, rows):
        out += eng.price_hawkesjd_chain_tilted_many_fused(ch, part, int(nb_steps_per_year), job_seeds, ids, gammas[q0:q0 + len(part)],
                                                          bool(recenter_forward))
    if not return_forwards:
        return [(prices, stderrs) for prices, stderrs, _ in out]
    return [(prices, stderrs, forwards_triples(stats)) for prices, stderrs, stats in out]


def _broadcast(v, nb_path: int, fill) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64)
    if v.shape[0] == 1:                   # initial value (reference :739-750)
        return v * fill(nb_path)
    assert v.shape[0] == nb_path
    return v


def simulate_hawkesjd_terminal(ttm: float, x0: np.ndarray, lambda_p0: np.ndarray, lambda_m0: np.ndarray, mu: float,
                               sigma: float, shift_p: float, mean_p: float, shift_m: float, mean_m: float, theta_p: float,
                               kappa_p: float, beta1_p: float, beta2_p: float, theta_m: float, kappa_m: float,
                               beta1_m: float, beta2_m: float, nb_path: int = 100000,
                               nb_steps_per_year: int = NB_STEPS_PER_YEAR, seed: Optional[int] = None
                               ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """terminal (x, lambda_p, lambda_m) after ttm from the given state (reference :715-776); a length-1 x0 becomes x0 * zeros,
    length-1 intensities lambda * ones, as there"""
    return hawkesjd_terminal_on_engine(ttm, x0, lambda_p0, lambda_m0, mu, sigma, shift_p, mean_p, shift_m, mean_m, theta_p,
                                       kappa_p, beta1_p, beta2_p, theta_m, kappa_m, beta1_m, beta2_m, nb_path,
                                       nb_steps_per_year, seed).get_state()


def hawkesjd_terminal_on_engine(ttm: float, x0: np.ndarray, lambda_p0: np.ndarray, lambda_m0: np.ndarray, mu: float,
                                sigma: float, shift_p: float, mean_p: float, shift_m: float, mean_m: float, theta_p: float,
                                kappa_p: float, beta1_p: float, beta2_p: float, theta_m: float, kappa_m: float,
                                beta1_m: float, beta2_m: float, nb_path: int = 100000,
                                nb_steps_per_year: int = NB_STEPS_PER_YEAR, seed: Optional[int] = None,
                                nb_steps: Optional[int] = None):
    """simulate_hawkesjd_terminal with the terminal state left on the engine it returns; nb_steps: a number of equal time steps
    in place of the grid of nb_steps_per_year"""
    x0 = _broadcast(x0, nb_path, np.zeros)
    lambda_p0 = _broadcast(lambda_p0, nb_path, np.ones)
    lambda_m0 = _broadcast(lambda_m0, nb_path, np.ones)
    block = params_block_of(dict(locals(), lambda_p=0.0, lambda_m=0.0))
    nb_steps, dt = (time_grid_steps(ttm=ttm, nb_steps_per_year=nb_steps_per_year) if nb_steps is None
                    else (int(nb_steps), float(ttm) / int(nb_steps)))
    rng_seed, call_id = next_rng_call(seed)
    eng = get_engine(int(nb_path))
    eng.set_state(x0, lambda_p0, lambda_m0)
    eng.hawkesjd_rng(nb_steps, dt, block, rng_seed, call_id, 0)
    return eng
