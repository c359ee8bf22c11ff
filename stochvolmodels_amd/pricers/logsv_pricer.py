"""
LogSV Monte Carlo on MI355X: drop-in for the MC part of the reference's pricers/logsv_pricer.py
(model_mc_price_chain :368-427, simulate_terminal_values :589-611, logsv_pdfs :613-635 / :742-803, logsv_mc_chain_pricer :806-867,
simulate_logsv_x_vol_terminal :950-1047, get_randoms_for_chain_valuation :1051-1074,
logsv_mc_chain_pricer_fixed_randoms :1100-1162).

Same names, keyword signatures, defaults and return structure; the arithmetic runs in libsvmc's HIP
kernels (one lane per path, fp64, state resident in HBM across expiries).  Two additions, both optional
keywords: `seed=` (the reference exposes none; default = process seed / set_seed + fresh call id) and
`comm=` (a stochvolmodels_amd.dist communicator to shard paths over GPUs; default = the process default).
"""
from __future__ import annotations

from enum import Enum
from typing import List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from .. import dist as svdist
from ..data.option_chain import OptionChain, black_ivols_native
from ..engine import (CMC_SETS_MAX, DeviceRandoms, chain_etas, cond_density_arrays, cond_density_stats_dicts, get_engine,
                      marshalled_chain, option_type_codes, payoff_finalize, tilted_type_codes)
from ..mc_chain import (chain_shaped, check_many_args, many_job_chunks, many_job_streams, many_jobs_shaped, price_chain_on_engine,
                        variable_type_code)
from ..mc_greeks import LOGSV_GREEK_PARAMS, check_greeks_request, greeks_bumps, greeks_job_table, greeks_shaped
from ..utils.calibration import ImpliedVolObjective, chain_calibration_weights, minimize_slsqp
from ..utils.config import VariableType
from ..utils.funcs import chain_step_grid, histogram_series, next_rng_call, set_time_grid, time_grid_steps, timer
from ..analytic import AnalyticGrid, chain_prices_from_sums, chain_sums, device_histograms, device_kdes, device_kdes_weighted, histogram_edges
from ..utils import mgf_pricer as mgfp
from .logsv.affine_expansion import ExpansionOrder, _order_code, get_init_conditions_a, note_integrator_flags
from .logsv.logsv_params import LogSvParams
from .logsv.vol_moments_ode import fit_model_vol_backbone_to_varswaps
from .model_pricer import ModelPricer

class LogsvModelCalibrationType(Enum):
    """which parameters the calibration solves for (reference :56-68)"""
    PARAMS4 = 1                     # sigma0, theta, beta, volvol; kappa1, kappa2 held at params0
    PARAMS5 = 2                     # sigma0, theta, kappa1, beta, volvol; kappa2 = kappa1 / theta
    PARAMS6 = 3
    PARAMS_WITH_VARSWAP_FIT = 4     # beta, volvol + a vol backbone fitted to variance swaps


class ConstraintsType(Enum):
    """martingale / moment constraints of Theorem 3.7 (reference :70-88)"""
    UNCONSTRAINT = 1
    MMA_MARTINGALE = 2              # kappa2 >= beta
    INVERSE_MARTINGALE = 3          # kappa2 >= 2 beta
    MMA_MARTINGALE_MOMENT4 = 4      # ... and kappa1 + kappa2 theta >= 1.5 (beta^2 + volvol^2)
    INVERSE_MARTINGALE_MOMENT4 = 5


class CalibrationEngine(Enum):
    """where the objective's model vols come from (reference :90-101)"""
    ANALYTIC = 1
    MC = 2
    ROUGH_MC = 3


_FREE_PARAMS = {LogsvModelCalibrationType.PARAMS4: ("sigma0", "theta", "beta", "volvol"),
                LogsvModelCalibrationType.PARAMS5: ("sigma0", "theta", "kappa1", "beta", "volvol"),
                LogsvModelCalibrationType.PARAMS_WITH_VARSWAP_FIT: ("beta", "volvol")}


def _calibration_parser(calibration_type: LogsvModelCalibrationType, params0: LogSvParams,
                        varswap_strikes: Optional[pd.Series] = None):
    """optimizer vector -> LogSvParams.  PARAMS4 keeps params0's kappas, PARAMS5 ties kappa2 = kappa1 / theta
    (LogSvParams(kappa2=None)); PARAMS_WITH_VARSWAP_FIT solves for (beta, volvol) only and, for every candidate,
    refits the vol backbone so that the model reproduces the term structure of `varswap_strikes`
    (vol_moments_ode.fit_model_vol_backbone_to_varswaps); H / nodes / weights always come from params0 (reference
    codec :106-160).  PARAMS6 raises as in the reference."""
    names = _FREE_PARAMS.get(calibration_type)
    if names is None:
        raise NotImplementedError(f"{calibration_type}")
    tied = calibration_type == LogsvModelCalibrationType.PARAMS5
    with_varswaps = calibration_type == LogsvModelCalibrationType.PARAMS_WITH_VARSWAP_FIT

    def parse(pars: np.ndarray) -> LogSvParams:
        fields = dict(sigma0=params0.sigma0, theta=params0.theta, kappa1=params0.kappa1,
                      kappa2=None if tied else params0.kappa2, H=params0.H, nodes=params0.nodes, weights=params0.weights)
        fields.update(zip(names, pars))
        params = LogSvParams(**fields)
        if with_varswaps:
            params.set_vol_backbone(fit_model_vol_backbone_to_varswaps(log_sv_params=params,
                                                                       varswap_strikes=varswap_strikes))
        return params
    return names, parse


def _calibration_constraints(parse, constraints_type: ConstraintsType):
    """SLSQP inequality constraints g(pars) >= 0 (reference :297-332)"""
    def mma(pars):
        p = parse(pars)
        return p.kappa2 - p.beta

    def inverse(pars):
        p = parse(pars)
        return p.kappa2 - 2.0 * p.beta

    def moment4(pars):
        p = parse(pars)
        return p.kappa1 + p.kappa2 * p.theta - 1.5 * (p.beta * p.beta + p.volvol * p.volvol)

    ineq = lambda f: {"type": "ineq", "fun": f}    # noqa: E731
    table = {ConstraintsType.UNCONSTRAINT: None,
             ConstraintsType.MMA_MARTINGALE: ineq(mma),
             ConstraintsType.INVERSE_MARTINGALE: ineq(inverse),
             ConstraintsType.MMA_MARTINGALE_MOMENT4: (ineq(mma), ineq(moment4)),
             ConstraintsType.INVERSE_MARTINGALE_MOMENT4: (ineq(inverse), ineq(moment4))}
    if constraints_type not in table:
        raise NotImplementedError(f"{constraints_type}")
    return table[constraints_type]


# logsv_mc_chain_pricer steps all expiries of a multi-expiry chain in one launch (svmc_logsv_chain_rng) when True,
# slice by slice otherwise (same bits)
WHOLE_CHAIN_STEPPING = True
# single-GPU chains on resident randoms go through svmc_logsv_chain_price_fixed (one C++ call per chain) when True
FUSED_FIXED_RANDOMS_DRIVER = True
# single-GPU chains with on-device randoms go through svmc_logsv_chain_price on the engine's own state (one C-ABI call per chain)
# when True; False (or WHOLE_CHAIN_STEPPING off, or several ranks): the phase-by-phase Python driver mc_chain.price_chain_on_engine
FUSED_MC_CHAIN_DRIVER = True
# rough LogSV chains: every expiry in one stepping launch (svmc_rough_logsv_chain); False = one launch per expiry (A/B, tests)
ROUGH_CHAIN_ONE_LAUNCH = True

LOGSV_BTC_PARAMS = LogSvParams(sigma0=0.8376, theta=1.0413, kappa1=3.1844, kappa2=3.058, beta=0.1514, volvol=1.8458)


# Grid points the coefficient-ODE integrator gave up on in the LAST analytic chain pricing of this process (step floor / try
# cap, csrc/svmc_analytic.hip): an int for logsv_chain_pricer, one count per parameter set for the batched pricer.  Zero for
# every sane parameter vector; non-zero means the inversion dropped those terms (as the reference's np.nansum drops NaN terms)
# and the prices are bounded but NOT the model's -- a RuntimeWarning says so, and a calibrator can test this to penalise the
# evaluation (the reference's solve_ivp returns whatever state it reached, without a signal).
LAST_ANALYTIC_GIVEN_UP = 0


def _note_given_up(count, n_grid: int) -> None:
    global LAST_ANALYTIC_GIVEN_UP
    LAST_ANALYTIC_GIVEN_UP = count
    if np.any(np.asarray(count) > 0):
        import warnings
        warnings.warn(f"analytic LogSV pricer: the coefficient ODEs were given up on {np.asarray(count).tolist()} of {n_grid} "
                      f"transform-grid points (stiff beyond the try cap, or blowing up before the expiry): those terms are dropped "
                      f"from the inversion and the prices are not the model's -- pricers.logsv_pricer.LAST_ANALYTIC_GIVEN_UP",
                      RuntimeWarning, stacklevel=3)


def _logsv_chain(params_list: Sequence[LogSvParams], ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms,
                 is_spot_measure: bool, expansion_order, variable_type, vol_scaler, kwargs):
    """the analytic chain pricing behind logsv_chain_pricer and logsv_chain_pricer_batch: the sets' grids side by side on one
    AnalyticGrid, the chain through chain_sums (the quadratic-variance inversion at one set only) -> the given-up counts
    [n_sets], the grid length and finish(), which turns the sums into prices [set][expiry] once the caller has noted the counts"""
    order = _order_code(expansion_order)
    inversion = "qvar" if int(getattr(variable_type, "value", variable_type)) == 2 else "vanilla"
    grids = [mgfp.get_transform_var_grid(variable_type=variable_type, is_spot_measure=is_spot_measure,
                                         vol_scaler=(set_vol_scaler(sigma0=p.sigma0, ttm=np.min(ttms))
                                                     if vol_scaler is None else vol_scaler)) for p in params_list]
    grid = AnalyticGrid.acquire([g[0] for g in grids], [g[1] for g in grids], 5 if order == 2 else 3)
    try:
        # [expiry][set][8]: the vol backbone's eta follows the expiry
        rows = np.array([[[p.sigma0, p.theta, p.kappa1, p.kappa2, p.beta, p.volvol, p.get_vol_backbone_eta(tau=ttm), 0.0]
                          for p in params_list] for ttm in ttms])

        def advance(i, dt):
            grid.logsv_advance(dt, rows[i], is_spot_measure, order, rtol=kwargs.get("ode_rtol"), atol=kwargs.get("ode_atol"))

        sums = chain_sums(grid, ttms, forwards, strikes_ttms, advance, inversion)
        return grid.last_given_up, grid.n, lambda: chain_prices_from_sums(sums, inversion, ttms, forwards, discfactors,
                                                                          strikes_ttms, optiontypes_ttms, is_spot_measure)
    finally:
        grid.release()


def logsv_chain_pricer_batch(params_list: Sequence[LogSvParams], ttms: np.ndarray, forwards: np.ndarray,
                             discfactors: np.ndarray, strikes_ttms: Sequence[np.ndarray],
                             optiontypes_ttms: Sequence[np.ndarray], is_spot_measure: bool = True,
                             expansion_order: ExpansionOrder = ExpansionOrder.SECOND, vol_scaler: float = None, **kwargs
                             ) -> List[List[np.ndarray]]:
    """logsv_chain_pricer (LOG_RETURN, numerical ODE route) for SEVERAL parameter sets on one chain, all sets advanced
    by one launch per expiry and inverted by one launch per expiry: [set][expiry] -> prices.  Each set keeps its own
    transform grid (set_vol_scaler follows its sigma0, reference :664-666); logsv_chain_pricer is this at one set.  A
    variable_type= keyword is swallowed by **kwargs and ignored.  Not in the reference API: the batched form of its per-set
    loop (config C5's five sets; the bumped vectors of a finite-difference gradient)."""
    given_up, n_grid, finish = _logsv_chain(params_list, ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms,
                                            is_spot_measure, expansion_order, VariableType.LOG_RETURN, vol_scaler, kwargs)
    _note_given_up(given_up, n_grid)
    return finish()


class LogSVPricer(ModelPricer):

    def price_chain_batch(self, option_chain: OptionChain, params_list: Sequence[LogSvParams], is_spot_measure: bool = True,
                          **kwargs) -> List[List[np.ndarray]]:
        """price_chain for several parameter sets in one batch of launches (logsv_chain_pricer_batch)"""
        return logsv_chain_pricer_batch(params_list=params_list, ttms=option_chain.ttms, forwards=option_chain.forwards,
                                        discfactors=option_chain.discfactors, strikes_ttms=option_chain.strikes_ttms,
                                        optiontypes_ttms=option_chain.optiontypes_ttms, is_spot_measure=is_spot_measure,
                                        **kwargs)

    def price_chain(self, option_chain: OptionChain, params: LogSvParams, is_spot_measure: bool = True, **kwargs
                    ) -> List[np.ndarray]:
        """analytic chain prices by Fourier inversion of the affine expansion (reference :345-366)"""
        return logsv_chain_pricer(params=params, ttms=option_chain.ttms, forwards=option_chain.forwards,
                                  discfactors=option_chain.discfactors, strikes_ttms=option_chain.strikes_ttms,
                                  optiontypes_ttms=option_chain.optiontypes_ttms, is_spot_measure=is_spot_measure,
                                  **kwargs)

    @timer
    def model_mc_price_chain(self, option_chain: OptionChain, params: LogSvParams, is_spot_measure: bool = True,
                             variable_type: VariableType = VariableType.LOG_RETURN, nb_path: int = 100000,
                             nb_steps: Optional[int] = None, **kwargs
                             ) -> Tuple[List[np.ndarray], List[np.ndarray]]:
        """price an option chain by Monte Carlo.  `nb_steps` is steps PER YEAR and defaults to
        int(360*max(ttms)) + 1, exactly the reference's rule (:427)."""
        if kwargs.get("use_rough_mc"):
            if "seed" not in kwargs:
                raise AssertionError("use_rough_mc requires seed=")          # reference :391
            if params.nodes is None or params.weights is None:
                raise ValueError("rough MC needs params.nodes / params.weights (LogSvParams.approximate_kernel)")
            common = dict(ttms=option_chain.ttms, forwards=option_chain.forwards, discfactors=option_chain.discfactors,
                          strikes_ttms=option_chain.strikes_ttms, optiontypes_ttms=option_chain.optiontypes_ttms,
                          sigma0=params.sigma0, theta=params.theta, kappa1=params.kappa1, kappa2=params.kappa2,
                          beta=params.beta, orthog_vol=params.volvol, weights=params.weights, nodes=params.nodes,
                          variable_type=variable_type, comm=kwargs.get("comm"),
                          normalize_stderr=bool(kwargs.get("normalize_stderr", False)))
            if kwargs.get("device_rng"):      # addition: no host randoms at all
                return rough_logsv_mc_chain_pricer(nb_path=nb_path, nb_steps_per_year=nb_steps or 360,
                                                   seed=kwargs["seed"], **common)
            Z0, Z1, grid_ttms = get_randoms_for_rough_vol_chain_valuation(ttms=option_chain.ttms, nb_path=nb_path,
                                                                          nb_steps_per_year=nb_steps or 360,
                                                                          seed=kwargs["seed"])
            return rough_logsv_mc_chain_pricer_fixed_randoms(Z0=Z0, Z1=Z1, timegrids=grid_ttms, **common)
        etas = params.get_vol_backbone_etas(ttms=option_chain.ttms)
        return logsv_mc_chain_pricer(v0=params.sigma0, theta=params.theta, kappa1=params.kappa1,
                                     kappa2=params.kappa2, beta=params.beta, volvol=params.volvol,
                                     vol_backbone_etas=etas, ttms=option_chain.ttms, forwards=option_chain.forwards,
                                     discfactors=option_chain.discfactors, strikes_ttms=option_chain.strikes_ttms,
                                     optiontypes_ttms=option_chain.optiontypes_ttms, is_spot_measure=is_spot_measure,
                                     variable_type=variable_type, nb_path=nb_path,
                                     nb_steps_per_year=nb_steps or int(360 * np.max(option_chain.ttms)) + 1,
                                     seed=kwargs.get("seed"), comm=kwargs.get("comm"), devices=kwargs.get("devices"),
                                     reduce=kwargs.get("reduce"))

    def model_mc_price_chain_conditional(self, option_chain: OptionChain, params: LogSvParams, is_spot_measure: bool = True,
                                         variable_type: VariableType = VariableType.LOG_RETURN, nb_path: int = 100000,
                                         nb_steps: Optional[int] = None, **kwargs):
        """model_mc_price_chain by conditional Monte Carlo (logsv_mc_chain_pricer_conditional) on the same step rule;
        recenter= and return_stats= are passed on"""
        etas = params.get_vol_backbone_etas(ttms=option_chain.ttms)
        return logsv_mc_chain_pricer_conditional(
            v0=params.sigma0, theta=params.theta, kappa1=params.kappa1, kappa2=params.kappa2, beta=params.beta, volvol=params.volvol,
            vol_backbone_etas=etas, ttms=option_chain.ttms, forwards=option_chain.forwards, discfactors=option_chain.discfactors,
            strikes_ttms=option_chain.strikes_ttms, optiontypes_ttms=option_chain.optiontypes_ttms, is_spot_measure=is_spot_measure,
            variable_type=variable_type, nb_path=nb_path, nb_steps_per_year=nb_steps or int(360 * np.max(option_chain.ttms)) + 1,
            seed=kwargs.get("seed"), comm=kwargs.get("comm"), devices=kwargs.get("devices"),
            recenter=kwargs.get("recenter", True), return_stats=kwargs.get("return_stats", False))

    def model_mc_chain_greeks_conditional(self, option_chain: OptionChain, params: LogSvParams, is_spot_measure: bool = True,
                                          variable_type: VariableType = VariableType.LOG_RETURN, nb_path: int = 100000,
                                          nb_steps: Optional[int] = None, **kwargs) -> dict:
        """model_mc_price_chain_conditional with delta, dual delta, gamma and dual gamma (logsv_mc_chain_greeks_conditional) on the
        same step rule; recenter=, return_stats=, wrt=, rel_bump= and bumps= are passed on"""
        etas = params.get_vol_backbone_etas(ttms=option_chain.ttms)
        return logsv_mc_chain_greeks_conditional(
            v0=params.sigma0, theta=params.theta, kappa1=params.kappa1, kappa2=params.kappa2, beta=params.beta, volvol=params.volvol,
            vol_backbone_etas=etas, ttms=option_chain.ttms, forwards=option_chain.forwards, discfactors=option_chain.discfactors,
            strikes_ttms=option_chain.strikes_ttms, optiontypes_ttms=option_chain.optiontypes_ttms, is_spot_measure=is_spot_measure,
            variable_type=variable_type, nb_path=nb_path, nb_steps_per_year=nb_steps or int(360 * np.max(option_chain.ttms)) + 1,
            seed=kwargs.get("seed"), comm=kwargs.get("comm"), devices=kwargs.get("devices"),
            recenter=kwargs.get("recenter", True), return_stats=kwargs.get("return_stats", False), wrt=kwargs.get("wrt", ()),
            rel_bump=kwargs.get("rel_bump", 1e-3), bumps=kwargs.get("bumps"))

    def model_mc_price_chain_conditional_many(self, option_chain: OptionChain, params_list: Sequence[LogSvParams],
                                              is_spot_measure: bool = True, variable_type: VariableType = VariableType.LOG_RETURN,
                                              nb_path: int = 100000, nb_steps: Optional[int] = None,
                                              seeds: Optional[Sequence[int]] = None, **kwargs) -> list:
        """model_mc_price_chain_conditional for several parameter sets, each with its own stream
        (logsv_mc_chain_pricer_conditional_many), on the same step rule; recenter= and return_stats= are passed on"""
        return logsv_mc_chain_pricer_conditional_many(
            params_list=params_list, ttms=option_chain.ttms, forwards=option_chain.forwards, discfactors=option_chain.discfactors,
            strikes_ttms=option_chain.strikes_ttms, optiontypes_ttms=option_chain.optiontypes_ttms, is_spot_measure=is_spot_measure,
            nb_path=nb_path, nb_steps_per_year=nb_steps or int(360 * np.max(option_chain.ttms)) + 1, variable_type=variable_type,
            seeds=seeds, comm=kwargs.get("comm"), devices=kwargs.get("devices"), recenter=kwargs.get("recenter", True),
            return_stats=kwargs.get("return_stats", False))

    def get_log_return_mc_pdf_conditional(self, params: LogSvParams, ttm: float, x_grid: np.ndarray, nb_path: int = 100000,
                                          seed: Optional[int] = None, recenter: bool = False, return_stderr: bool = False,
                                          nb_steps: Optional[int] = None):
        """the density of the simulated log-return at x_grid from the conditional estimator's dual gamma, without a bandwidth
        (conditional_log_return_pdf): UN-NORMALISED -- the KDE routes divide by their sum, this one integrates by itself to
        n_kept_nonzero_cv / n_kept, the share of the kept paths whose conditional variance is positive (a cv == 0 path is a point
        mass and adds nothing).  recenter=False: the density of the simulated x itself, as get_log_return_mc_pdf's.  With
        return_stderr=True (pdf, its standard error)."""
        def route(**chain):
            return logsv_mc_chain_greeks_conditional(
                v0=params.sigma0, theta=params.theta, kappa1=params.kappa1, kappa2=params.kappa2, beta=params.beta,
                volvol=params.volvol, vol_backbone_etas=params.get_vol_backbone_etas(ttms=np.array([ttm])), nb_path=nb_path,
                nb_steps_per_year=nb_steps or int(360 * ttm) + 1, seed=seed, recenter=recenter, **chain)
        return conditional_log_return_pdf(route, ttm, x_grid, return_stderr)

    def get_log_return_mc_pdf_mixture(self, params: LogSvParams, ttm: float, x_grid: np.ndarray, risk_premia_gammas=None,
                                      nb_path: int = 100000, seed: Optional[int] = None, return_stderr: bool = False,
                                      return_stats: bool = False, nb_steps: Optional[int] = None, is_spot_measure: bool = True,
                                      variable_type: VariableType = VariableType.LOG_RETURN, comm=None, devices=None):
        """the density of the simulated log-return at x_grid as the mixture of the paths' conditional Gaussians, without a bandwidth
        (mixture_log_return_pdf; include/svmc_est.h's svmc_cond_density_chain): the paths of
        model_mc_price_chain_conditional at this seed and step rule, one exponential per (path, point).  risk_premia_gammas=None:
        pdf in x_grid's shape -- get_log_return_mc_pdf_conditional(recenter=False)'s number, UN-NORMALISED in the same way: it
        integrates to the share of the kept paths whose conditional variance is positive.  A sequence of up to 16 gammas: the
        densities under the exponential kernel exp(gamma x), [gamma][x], each normalised by its weights, from the same stepping
        call (a gamma at which a path's squared weight overflows: NaN).  return_stderr=, return_stats= add the standard error and
        the dict(s) of engine.CD_STATS_FIELDS.  The log-return, the spot measure and one GPU only."""
        etas = params.get_vol_backbone_etas(ttms=np.array([ttm]))

        def step_rows(eng, rng_seed, call_id):
            nb, dt = one_expiry_grid(ttm, nb_steps or int(360 * ttm) + 1)
            eng.fill_state_cmc(0.0, params.sigma0, 0.0)
            eng.logsv_chain_cmc([nb], [dt], np.ravel(etas), params.theta, params.kappa1, params.kappa2, params.beta, params.volvol,
                                True, rng_seed, call_id, mu_row=0, cv_row=1)
        return mixture_log_return_pdf("LogSVPricer.get_log_return_mc_pdf_mixture", step_rows, x_grid, risk_premia_gammas, nb_path, seed,
                                      return_stderr, return_stats, variable_type, comm, devices, is_spot_measure)

    def model_mc_chain_greeks(self, option_chain: OptionChain, params: LogSvParams, is_spot_measure: bool = True,
                              variable_type: VariableType = VariableType.LOG_RETURN, nb_path: int = 100000,
                              nb_steps: Optional[int] = None, **kwargs) -> dict:
        """model_mc_price_chain with its Greeks (logsv_mc_chain_greeks) on the same step rule; wrt=, rel_bump=, bumps= and seed= are
        passed on"""
        return logsv_mc_chain_greeks(
            params=params, ttms=option_chain.ttms, forwards=option_chain.forwards, discfactors=option_chain.discfactors,
            strikes_ttms=option_chain.strikes_ttms, optiontypes_ttms=option_chain.optiontypes_ttms, wrt=kwargs.get("wrt"),
            rel_bump=kwargs.get("rel_bump", 1e-3), bumps=kwargs.get("bumps"), nb_path=nb_path,
            nb_steps_per_year=nb_steps or int(360 * np.max(option_chain.ttms)) + 1, seed=kwargs.get("seed"),
            is_spot_measure=is_spot_measure, variable_type=variable_type, comm=kwargs.get("comm"), devices=kwargs.get("devices"))

    def model_mc_price_chain_many(self, option_chain: OptionChain, params_list: Sequence[LogSvParams],
                                  is_spot_measure: bool = True, variable_type: VariableType = VariableType.LOG_RETURN,
                                  nb_path: int = 100000, nb_steps: Optional[int] = None,
                                  seeds: Optional[Sequence[int]] = None, **kwargs
                                  ) -> List[Tuple[List[np.ndarray], List[np.ndarray]]]:
        """model_mc_price_chain for several parameter sets, each with its own stream (logsv_mc_chain_pricer_many), on
        model_mc_price_chain's step rule: job j returns what model_mc_price_chain(option_chain, params_list[j],
        seed=seeds[j], ...) returns"""
        return logsv_mc_chain_pricer_many(params_list=params_list, ttms=option_chain.ttms, forwards=option_chain.forwards,
                                          discfactors=option_chain.discfactors, strikes_ttms=option_chain.strikes_ttms,
                                          optiontypes_ttms=option_chain.optiontypes_ttms, is_spot_measure=is_spot_measure,
                                          nb_path=nb_path,
                                          nb_steps_per_year=nb_steps or int(360 * np.max(option_chain.ttms)) + 1,
                                          variable_type=variable_type, seeds=seeds, comm=kwargs.get("comm"),
                                          devices=kwargs.get("devices"))

    def set_vol_scaler(self, option_chain: OptionChain) -> float:
        """transform-grid scaler from the chain's first ATM vol, held fixed over a calibration (reference :429-438)"""
        return set_vol_scaler(sigma0=option_chain.get_chain_atm_vols()[0], ttm=option_chain.ttms[0])

    @timer
    def calibrate_model_params_to_chain(self, option_chain: OptionChain, params0: LogSvParams,
                                        params_min: LogSvParams = LogSvParams(sigma0=0.1, theta=0.1, kappa1=0.25,
                                                                              kappa2=0.25, beta=-3.0, volvol=0.2),
                                        params_max: LogSvParams = LogSvParams(sigma0=1.5, theta=1.5, kappa1=10.0,
                                                                              kappa2=10.0, beta=3.0, volvol=3.0),
                                        is_vega_weighted: bool = True, is_unit_ttm_vega: bool = False,
                                        model_calibration_type: LogsvModelCalibrationType = LogsvModelCalibrationType.PARAMS5,
                                        constraints_type: ConstraintsType = ConstraintsType.UNCONSTRAINT,
                                        calibration_engine: CalibrationEngine = CalibrationEngine.ANALYTIC,
                                        nb_path: int = 100000, nb_steps: int = 360, seed: int = 10, **kwargs
                                        ) -> LogSvParams:
        """fit the model to the chain's mid implied vols: SLSQP on the vega-weighted squared vol error of Eq. (6.3)
        (reference :440-557).  The MC engines draw the reference's RandomState(seed) randoms once, upload this rank's
        columns to HBM once, and every objective evaluation re-prices the chain from those resident randoms -- the
        optimizer loop is kernel-bound, not PCIe-bound.  `kwargs`: comm=, disp= (SLSQP printing, default True as in
        the reference).  `self.last_calibration` keeps {"n_eval", "objective"} of the run.
        calibration_engine=CalibrationEngine.MC with estimator="conditional" (DESIGN.md row f15): the objective on the conditional
        Monte Carlo estimator (logsv_mc_chain_pricer_conditional_sets) on the frozen stream (seed, call 0) -- an order of magnitude
        less noise per path, a smooth function under the forward differences, nothing stored in HBM (device_randoms="hbm" raises
        ValueError, a sharded request NotImplementedError); recenter= is passed on (default True)."""
        vol_scaler = self.set_vol_scaler(option_chain=option_chain)
        _, market_vols_ttms = option_chain.get_chain_data_as_xy()
        market_vols = np.concatenate(market_vols_ttms).ravel()
        weights = chain_calibration_weights(option_chain, market_vols, is_vega_weighted, is_unit_ttm_vega)
        varswap_strikes = (option_chain.get_slice_varswap_strikes(floor_with_atm_vols=True)
                           if model_calibration_type == LogsvModelCalibrationType.PARAMS_WITH_VARSWAP_FIT else None)
        names, parse = _calibration_parser(model_calibration_type, params0, varswap_strikes)
        p0 = np.array([getattr(params0, n) for n in names], dtype=float)
        bounds = tuple((getattr(params_min, n), getattr(params_max, n)) for n in names)
        comm = kwargs.get("comm")
        chain_args = dict(ttms=option_chain.ttms, forwards=option_chain.forwards, discfactors=option_chain.discfactors,
                          strikes_ttms=option_chain.strikes_ttms, optiontypes_ttms=option_chain.optiontypes_ttms)
        resident = None
        model_vols_batch = None
        if calibration_engine == CalibrationEngine.ANALYTIC:
            # ode_rtol= / ode_atol=: the tolerances of the coefficient ODEs for this fit (default: the pricers' 1e-10 / 1e-12;
            # looser settings buy little since the 8th-order pair: stochvolmodels_amd/analytic.py)
            tol = {k: kwargs[k] for k in ("ode_rtol", "ode_atol") if k in kwargs}

            def model_vols(pars):
                return self.compute_model_ivols_for_chain(option_chain=option_chain, params=parse(pars),
                                                          vol_scaler=vol_scaler, **tol)

            def model_vols_batch(pars_list):
                # the n bumped vectors of SLSQP's forward-difference gradient through ONE batch of launches per expiry
                # (logsv_chain_pricer_batch: the sets advance together; bit-identical to one call per set)
                prices = self.price_chain_batch(option_chain=option_chain, params_list=[parse(p) for p in pars_list],
                                                vol_scaler=vol_scaler, **tol)
                return [option_chain.compute_model_ivols_from_chain_data(model_prices=pr) for pr in prices]
            if not kwargs.get("batched_gradient", True):
                model_vols_batch = None
        elif calibration_engine == CalibrationEngine.MC and kwargs.get("estimator") is not None:
            # estimator="conditional" (DESIGN.md row f15): the conditional estimator on the frozen stream (seed, call 0) -- an
            # evaluation is one replayed graph with the implied vols as its last kernel, the bumped vectors of a gradient ride one
            # stepping launch (logsv_mc_chain_pricer_conditional_sets).  Nothing is stored in HBM.
            if kwargs["estimator"] != "conditional":
                raise ValueError(f"estimator={kwargs['estimator']!r}: 'conditional', or no keyword for the plain estimator")
            if kwargs.get("device_randoms") == "hbm":
                raise ValueError('estimator="conditional" stores no randoms: device_randoms="hbm" does not apply')
            sets_args = dict(chain_args, nb_path=nb_path, nb_steps_per_year=nb_steps, seed=seed, recenter=kwargs.get("recenter", True),
                             return_ivols=True, comm=comm, devices=kwargs.get("devices"))
            check_conditional_request("calibrate_model_params_to_chain", VariableType.LOG_RETURN, comm, kwargs.get("devices"),
                                      option_chain.optiontypes_ttms)

            def model_vols(pars):
                return logsv_mc_chain_pricer_conditional_sets([parse(pars)], **sets_args)[0][2]

            def model_vols_batch(pars_list):
                return [res[2] for res in logsv_mc_chain_pricer_conditional_sets([parse(p) for p in pars_list], **sets_args)]
            if not kwargs.get("batched_gradient", True):
                model_vols_batch = None
        elif calibration_engine == CalibrationEngine.MC:
            if kwargs.get("device_randoms", False):
                # the fixed randoms are the counter-based stream of `seed` instead of NumPy's RandomState arrays (about a
                # second of host draws per 10^5 paths, 582 MB of upload at 10^5 x 364): same estimator, another sample.
                # device_randoms=True keeps NOTHING resident -- every objective evaluation regenerates the draws in
                # registers (svmc_logsv_chain_price_frozen_sets: no HBM term in the stepping, the draw shared by the
                # bumped parameter sets of a gradient); device_randoms="hbm" materialises them in HBM as round 4 did
                resident = draw_fixed_randoms_on_device(ttms=option_chain.ttms, nb_path=nb_path, nb_steps_per_year=nb_steps,
                                                        seed=seed, comm=comm, in_hbm=kwargs["device_randoms"] == "hbm")
            else:
                resident = upload_fixed_randoms(*get_randoms_for_chain_valuation(
                    ttms=option_chain.ttms, nb_path=nb_path, nb_steps_per_year=nb_steps, seed=seed), comm=comm)

            def model_vols(pars):
                # prices AND their implied vols in one call: on one GPU the inversion is the last kernel of the replayed
                # graph (svmc_logsv_chain_price_fixed_iv), so an objective evaluation is one launch and one wait
                p = parse(pars)
                _, _, ivols = logsv_mc_chain_pricer_fixed_randoms(
                    W0s=resident, W1s=None, dts=None, v0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2,
                    beta=p.beta, volvol=p.volvol, vol_backbone_etas=p.get_vol_backbone_etas(ttms=option_chain.ttms),
                    comm=comm, return_ivols=True, **chain_args)
                return ivols

            def model_vols_batch(pars_list):
                # the bumped vectors of SLSQP's forward-difference gradient in one replay: every lane steps all of them on
                # each pair of normals it reads (svmc_logsv_chain_price_fixed_sets) -- bit-identical to one call per vector
                out = logsv_mc_chain_pricer_fixed_randoms_batch(params_list=[parse(p) for p in pars_list], W0s=resident,
                                                                return_ivols=True, comm=comm, **chain_args)
                return [res[2] for res in out]
            if not kwargs.get("batched_gradient", True):
                model_vols_batch = None
        elif calibration_engine == CalibrationEngine.ROUGH_MC:
            if kwargs.get("device_randoms", False):
                # as for the MC engine: Z0 / Z1 drawn in HBM instead of by NumPy (same grids, another sample)
                grids = [set_time_grid(ttm=ttm, nb_steps_per_year=nb_steps)[2] for ttm in option_chain.ttms]
                comm_ = comm or svdist.get_default_comm()
                offset, n_local = svdist.shard_range(nb_path, comm_.rank, comm_.world)
                get_engine(n_local, path_offset=offset)
                resident = DeviceRandoms.drawn_on_device([grids[-1].size - 1], [0.0], nb_path, n_local, offset, seed)
            else:
                Z0, Z1, grids = get_randoms_for_rough_vol_chain_valuation(ttms=option_chain.ttms, nb_path=nb_path,
                                                                          nb_steps_per_year=nb_steps, seed=seed)
                resident = upload_rough_randoms(Z0, Z1, comm=comm)

            def model_vols(pars):
                p = parse(pars)
                prices, _ = rough_logsv_mc_chain_pricer_fixed_randoms(
                    Z0=resident, Z1=None, sigma0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2,
                    beta=p.beta, orthog_vol=p.volvol, weights=p.weights, nodes=p.nodes, timegrids=grids, comm=comm,
                    **chain_args)
                return option_chain.compute_model_ivols_from_chain_data(model_prices=prices)
        else:
            raise NotImplementedError(f"{calibration_engine}")
        objective = ImpliedVolObjective(model_vols, market_vols, weights, model_vols_batch=model_vols_batch, bounds=bounds)
        try:
            fit = minimize_slsqp(objective, p0, bounds, _calibration_constraints(parse, constraints_type),
                                 disp=bool(kwargs.get("disp", True)),
                                 jac=objective.gradient if model_vols_batch is not None else None)
            self.last_calibration = dict(n_eval=objective.n_eval, n_gradient_batches=objective.n_batches,
                                         objective=objective(fit))
        finally:
            if resident is not None:
                resident.free()
        return parse(fit)

    @timer
    def simulate_vol_paths(self, params: LogSvParams, brownians: np.ndarray = None, ttm: float = 1.0,
                           nb_path: int = 100000, is_spot_measure: bool = True, nb_steps: int = None,
                           year_days: int = 360, **kwargs) -> Tuple[np.ndarray, np.ndarray]:
        """volatility paths on the time grid (reference :560-587).  As in the reference, `nb_steps` (default
        ceil(year_days*ttm)) is handed on as steps PER YEAR."""
        nb_steps = nb_steps or int(np.ceil(year_days * ttm))
        return simulate_vol_paths(ttm=ttm, v0=params.sigma0, theta=params.theta, kappa1=params.kappa1,
                                  kappa2=params.kappa2, beta=params.beta, volvol=params.volvol, nb_path=nb_path,
                                  is_spot_measure=is_spot_measure, nb_steps_per_year=nb_steps, brownians=brownians,
                                  **kwargs)

    def vol_path_moments(self, params: LogSvParams, ttm: float = 1.0, nb_path: int = 100000, is_spot_measure: bool = True,
                         nb_steps: int = None, year_days: int = 360, n_terms: int = 4, **kwargs) -> dict:
        """per-time-step Monte Carlo moments of the volatility paths, computed on the device (module-level vol_path_moments):
        the reduction the reference's scripts apply to simulate_vol_paths' array, without the 8 bytes per path-step of PCIe"""
        nb_steps = nb_steps or int(np.ceil(year_days * ttm))
        return vol_path_moments(ttm=ttm, v0=params.sigma0, theta=params.theta, kappa1=params.kappa1, kappa2=params.kappa2,
                                beta=params.beta, volvol=params.volvol, is_spot_measure=is_spot_measure, nb_path=nb_path,
                                nb_steps_per_year=nb_steps, n_terms=n_terms, **kwargs)

    @timer
    def simulate_terminal_values(self, params: LogSvParams, ttm: float = 1.0, nb_path: int = 100000,
                                 is_spot_measure: bool = True, **kwargs
                                 ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        # same as simulate_logsv_x_vol_terminal(x0=zeros, sigma0=sigma0*ones, qvar0=zeros, ...) (reference :600-610),
        # with the constant initial state written on the device instead of uploaded
        return self._simulate_on_engine(params, ttm, nb_path, is_spot_measure, kwargs.get("seed")).get_state()

    @staticmethod
    def _simulate_on_engine(params: LogSvParams, ttm: float, nb_path: int, is_spot_measure: bool, seed, nb_steps: Optional[int] = None):
        """the terminal state of simulate_terminal_values left on the engine it returns (the state stays on the device);
        nb_steps: a number of equal time steps in place of the daily grid's"""
        nb_steps, dt = time_grid_steps(ttm=ttm, nb_steps_per_year=360) if nb_steps is None else (int(nb_steps), float(ttm) / int(nb_steps))
        rng_seed, call_id = next_rng_call(seed)
        eng = get_engine(nb_path)
        eng.fill_state(0.0, params.sigma0, 0.0)
        eng.logsv_rng(nb_steps, dt, params.theta, params.kappa1, params.kappa2, params.beta, params.volvol, 1.0,
                      is_spot_measure, rng_seed, call_id, 0)
        return eng

    def model_mc_il_payoff(self, params: LogSvParams, ttm: float, p1, p0, pa, pb, nb_path: int = 100000, nb_steps: Optional[int] = None,
                           seed: Optional[int] = None, notional=1000000, return_pieces: bool = False, **kwargs):
        """the Monte Carlo impermanent loss of the range [pa, pb] opened at p0, at the forward p1, under this model: the terminal
        log-returns of simulate_terminal_values stay on the device and svmc_il_payoff reduces them (include/svmc.h: recentred
        spots, value = -(notional0 notional) mean(pay), its standard error).  p1, p0, pa, pb, notional broadcast together and
        share one path set.  nb_steps: the number of time steps (default: the model's daily grid).  Returns (value, stderr), and
        with return_pieces=True a dict of the six piece means, n_kept and n_dropped.  A sharded request (comm=, devices=) raises
        NotImplementedError.  Not in the reference, which has no Monte Carlo side for this payoff."""
        from .il_pricer import il_cases, refuse_sharded_il
        refuse_sharded_il("model_mc_il_payoff", kwargs)
        il_cases(p1, p0, pa, pb, notional)                       # ValueError before any device work
        eng = self._simulate_on_engine(params, ttm, nb_path, True, seed, nb_steps)
        return eng.il_payoffs(p1, p0, pa, pb, notional, return_pieces=return_pieces)

    @timer
    def logsv_pdfs(self, params: LogSvParams, ttm: float, space_grid: np.ndarray, is_stiff_solver: bool = False,
                   is_analytic: bool = False, is_spot_measure: bool = True,
                   expansion_order: ExpansionOrder = ExpansionOrder.SECOND,
                   variable_type: VariableType = VariableType.LOG_RETURN, vol_scaler: float = None) -> np.ndarray:
        """the model density of the log-return, the annualised quadratic variance or the volatility on `space_grid`, as bin
        masses (reference :613-635; module-level logsv_pdfs)"""
        return logsv_pdfs(params=params, ttm=ttm, space_grid=space_grid, is_stiff_solver=is_stiff_solver,
                          is_analytic=is_analytic, is_spot_measure=is_spot_measure, expansion_order=expansion_order,
                          variable_type=variable_type, vol_scaler=vol_scaler)

    def terminal_value_histograms(self, params: LogSvParams, ttm: float = 1.0, nb_path: int = 100000,
                                  is_spot_measure: bool = True, space_grids: Optional[dict] = None, n: int = 200,
                                  n_stdevs: float = 3.0, **kwargs) -> dict:
        """simulate_terminal_values followed by compute_histogram_data of x, qvar / ttm and sigma on their space grids, with
        the counting done on the device: {VariableType: pd.Series}, each Series what utils.funcs.compute_histogram_data
        returns for that variable (its first entry is x_grid[0] / nb_path, the reference's quirk) -- 3 x n_bins counts come
        back instead of 3 x nb_path doubles.  space_grids: {VariableType: grid}; default params.get_variable_space_grid(
        ttm=ttm, n=n, n_stdevs=n_stdevs) of the three variables.  seed= as simulate_terminal_values.  Not in the reference API."""
        if space_grids is None:
            space_grids = {vt: params.get_variable_space_grid(variable_type=vt, ttm=ttm, n=n, n_stdevs=n_stdevs)
                           for vt in (VariableType.LOG_RETURN, VariableType.Q_VAR, VariableType.SIGMA)}
        eng = self._simulate_on_engine(params, ttm, nb_path, is_spot_measure, kwargs.get("seed"))
        return engine_state_histograms(eng, space_grids, ttm)

    def terminal_value_kdes(self, params: LogSvParams, ttm: float = 1.0, nb_path: int = 100000,
                            is_spot_measure: bool = True, space_grids: Optional[dict] = None, n: int = 200,
                            n_stdevs: float = 3.0, **kwargs):
        """simulate_terminal_values followed by scipy.stats.gaussian_kde of x, qvar / ttm and sigma on their space grids, with the
        n_path x n_grid exponentials summed on the device: {VariableType: density per unit of the variable}.  space_grids, n,
        n_stdevs and seed= as terminal_value_histograms; bandwidth_factor= a positive factor in place of Scott's;
        return_stats=True also returns {VariableType: {n_kept, n_nan, n_low, n_high, mean, var, h, factor}}.
        risk_premia_gamma= a float or up to 16 gammas: every variable weighted by exp(gamma x) (engine_state_kdes), the densities
        [n_gammas][n_grid] and the stats a list per gamma.  Not in the reference API."""
        refuse_sharded_kde("terminal_value_kdes", kwargs)
        if space_grids is None:
            space_grids = {vt: params.get_variable_space_grid(variable_type=vt, ttm=ttm, n=n, n_stdevs=n_stdevs)
                           for vt in (VariableType.LOG_RETURN, VariableType.Q_VAR, VariableType.SIGMA)}
        eng = self._simulate_on_engine(params, ttm, nb_path, is_spot_measure, kwargs.get("seed"))
        return split_kde_results(engine_state_kdes(eng, space_grids, ttm, **kde_keywords(kwargs)), kwargs.get("return_stats", False))

    def get_log_return_mc_pdf_device(self, ttm: float, params: LogSvParams, x_grid: np.ndarray, nb_path: int = 100000,
                                     **kwargs) -> np.ndarray:
        """get_log_return_mc_pdf with the state left on the device and the kernel estimate summed there (seed= and
        is_spot_measure= as simulate_terminal_values; risk_premia_gamma= and return_stats= as engine_log_return_mc_pdf)"""
        refuse_sharded_kde("get_log_return_mc_pdf_device", kwargs)
        eng = self._simulate_on_engine(params, ttm, nb_path, kwargs.get("is_spot_measure", True), kwargs.get("seed"))
        return engine_log_return_mc_pdf(eng, x_grid, kwargs.get("risk_premia_gamma"), kwargs.get("return_stats", False))


def engine_state_histograms(eng, space_grids: dict, ttm: float) -> dict:
    """compute_histogram_data of the engine's resident state on the given grids, counted on the device (svmc_histogram_uniform):
    LOG_RETURN -> x, Q_VAR -> qvar / ttm, SIGMA -> the second state vector (the volatility; Heston's variance)"""
    src = {1: (eng.x.ptr, 1.0), 2: (eng.qvar.ptr, float(ttm)), 3: (eng.vol.ptr, 1.0)}
    keys = list(space_grids)
    grids = [np.asarray(space_grids[k], dtype=np.float64) for k in keys]
    codes = [int(getattr(k, "value", k)) for k in keys]
    if any(c not in src for c in codes):
        raise NotImplementedError
    edges = [histogram_edges(g[0], g[-1], len(g) - 1) for g in grids]
    counts = device_histograms([src[c][0] for c in codes], eng.n_path, edges, [src[c][1] for c in codes], eng.stream)
    return {k: histogram_series(cnt, e, g[0], eng.n_path) for k, g, e, cnt in zip(keys, grids, edges, counts)}


MAX_KDE_GAMMAS = 16


def engine_state_kdes(eng, space_grids: dict, ttm: float, limit: float = 1e16, bandwidth_factor: Optional[float] = None,
                      risk_premia_gamma=None) -> dict:
    """scipy.stats.gaussian_kde of the engine's resident state on the given grids, summed on the device (svmc_kde_gaussian), with
    engine_state_histograms' sources: LOG_RETURN -> x, Q_VAR -> qvar / ttm, SIGMA -> the second state vector.
    {key: (density per unit of the variable, stats)}.  risk_premia_gamma: None, or a float or a sequence of up to 16 gammas;
    then every variable is weighted by exp(gamma x) of the resident (undivided) x (svmc_kde_gaussian_weighted, one call per
    variable and gamma on the engine's stream, one upload and one download) and the result gains a leading gamma axis, also for
    a float: {key: (density [n_gammas][n_grid], [stats per gamma])}"""
    src = {1: (eng.x.ptr, 1.0), 2: (eng.qvar.ptr, float(ttm)), 3: (eng.vol.ptr, 1.0)}
    keys = list(space_grids)
    codes = [int(getattr(k, "value", k)) for k in keys]
    if any(c not in src for c in codes):
        raise NotImplementedError
    if risk_premia_gamma is None:
        out = device_kdes([src[c][0] for c in codes], eng.n_path, [space_grids[k] for k in keys], [src[c][1] for c in codes],
                          limit=limit, bandwidth_factor=bandwidth_factor, stream=eng.stream)
        return dict(zip(keys, out))
    gammas = [float(g) for g in np.atleast_1d(np.asarray(risk_premia_gamma, dtype=np.float64)).ravel()]
    if not 1 <= len(gammas) <= MAX_KDE_GAMMAS:
        raise ValueError(f"risk_premia_gamma: between 1 and {MAX_KDE_GAMMAS} gammas, got {len(gammas)}")
    n_g, n_k = len(gammas), len(keys)
    out = device_kdes_weighted([src[c][0] for c in codes] * n_g, eng.n_path, [space_grids[k] for k in keys] * n_g,
                               [src[c][1] for c in codes] * n_g, tilt_ptrs=[eng.x.ptr] * (n_g * n_k),
                               gammas=[g for g in gammas for _ in keys], limit=limit, bandwidth_factor=bandwidth_factor,
                               stream=eng.stream)
    return {k: (np.stack([out[g * n_k + i][0] for g in range(n_g)]), [out[g * n_k + i][1] for g in range(n_g)])
            for i, k in enumerate(keys)}


def kde_keywords(kwargs: dict) -> dict:
    """the keywords a pricer's terminal_value_kdes hands on to engine_state_kdes; risk_premia_gamma only where it is given, so
    that a call without it is the call it was"""
    kw = {"bandwidth_factor": kwargs.get("bandwidth_factor")}
    if kwargs.get("risk_premia_gamma") is not None:
        kw["risk_premia_gamma"] = kwargs["risk_premia_gamma"]
    return kw


def split_kde_results(out: dict, return_stats: bool):
    """engine_state_kdes' {key: (density, stats)} as {key: density}, or with return_stats ({key: density}, {key: stats})"""
    densities = {k: d for k, (d, _) in out.items()}
    return (densities, {k: s for k, (_, s) in out.items()}) if return_stats else densities


def refuse_sharded_kde(who: str, kwargs: dict) -> None:
    """the kernel density estimate runs on one engine: a sharded request (comm= of world > 1, devices=, or a default
    communicator of world > 1) raises rather than estimate from one rank's paths"""
    comm = kwargs.get("comm")
    if kwargs.get("devices") is not None or (comm.world if comm is not None else svdist.get_default_comm().world) > 1:
        raise NotImplementedError(f"{who}: the kernel density estimate is not sharded over ranks or devices")


def engine_log_return_mc_pdf(eng, x_grid: np.ndarray, risk_premia_gamma=None, return_stats: bool = False):
    """ModelPricer.get_log_return_mc_pdf's arithmetic on the engine's resident x: the reference's line about the dropped paths
    from the device counts, then density / nansum(density).  risk_premia_gamma: None, or a float or up to 16 gammas; then the
    estimate is weighted by exp(gamma x) (engine_state_kdes), the line is printed once (the counts of x do not depend on gamma)
    and every gamma's row is normalised on its own: [n_gammas][n_grid].  return_stats=True -> (pdf, stats), the stats a dict, or
    a list of dicts per gamma"""
    grids = {1: np.asarray(x_grid, dtype=np.float64)}
    if risk_premia_gamma is None:
        density, stats = engine_state_kdes(eng, grids, 1.0)[1]
        first, total = stats, np.nansum(density)
    else:
        density, stats = engine_state_kdes(eng, grids, 1.0, risk_premia_gamma=risk_premia_gamma)[1]
        first, total = stats[0], np.nansum(density, axis=1, keepdims=True)
    print(f"in mc: num -inf = {first['n_low']}, num +inf = {first['n_high']}, num nans = {first['n_nan']}")
    return (density / total, stats) if return_stats else density / total


def set_vol_scaler(sigma0: float, ttm: float) -> float:
    """transform-grid scaler from the ATM vol and the shortest maturity, floored at two weeks (reference :664-666)"""
    return sigma0 * np.sqrt(np.minimum(np.min(ttm), 0.5 / 12.0))


def logsv_chain_pricer(params: LogSvParams, ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                       strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray],
                       is_stiff_solver: bool = False, is_analytic: bool = False, is_spot_measure: bool = True,
                       expansion_order: ExpansionOrder = ExpansionOrder.SECOND,
                       variable_type: VariableType = VariableType.LOG_RETURN, vol_scaler: float = None, **kwargs
                       ) -> List[np.ndarray]:
    """analytic LogSV chain prices (reference :669-739): per expiry one launch integrating the coefficient ODEs of every
    transform-grid point from the previous expiry's A, then one launch of per-strike Simpson sums.  LOG_RETURN uses
    the 1000-point phi grid; Q_VAR (calls on the annualised quadratic variance) the 40 000-point psi grid."""
    if int(getattr(variable_type, "value", variable_type)) not in (1, 2):
        raise NotImplementedError
    note_integrator_flags(is_stiff_solver, is_analytic)       # both accepted: one device integrator answers them (warned once)
    given_up, n_grid, finish = _logsv_chain([params], ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms,
                                            is_spot_measure, expansion_order, variable_type, vol_scaler, kwargs)
    _note_given_up(int(given_up[0]), n_grid)
    return finish()[0]


def _pdf_setup(params: LogSvParams, ttm: float, is_spot_measure: bool, order: int, variable_type, vol_scaler):
    """the grids, A(0) and the inversion's (transform grid, which resident buffer it is, shift, scale) of one logsv_pdfs case
    (reference :756-795)"""
    if variable_type not in (VariableType.LOG_RETURN, VariableType.Q_VAR, VariableType.SIGMA):
        raise NotImplementedError
    if vol_scaler is None:
        vol_scaler = set_vol_scaler(sigma0=params.sigma0, ttm=ttm)
    phi_grid, psi_grid, theta_grid = mgfp.get_transform_var_grid(variable_type=variable_type, is_spot_measure=is_spot_measure,
                                                                 vol_scaler=vol_scaler)
    a_t0 = get_init_conditions_a(phi_grid=phi_grid, psi_grid=psi_grid, theta_grid=theta_grid, n_terms=5 if order == 2 else 3,
                                 variable_type=variable_type)
    if variable_type == VariableType.LOG_RETURN:
        var_grid, resident, shift, scale = phi_grid, "phi", 0.0, 1.0
    elif variable_type == VariableType.Q_VAR:                 # scaled by ttm
        var_grid, resident, shift, scale = psi_grid, "psi", 0.0, 1.0 / ttm
    else:                                                     # SIGMA: the theta grid is not one of the ODE's two, it is uploaded
        var_grid, resident, shift, scale = theta_grid, None, params.theta, 1.0
    return phi_grid, psi_grid, a_t0, var_grid, resident, shift, scale


def _logsv_pdfs(params_list: Sequence[LogSvParams], ttm: float, space_grids, orders: Sequence[int], is_spot_measure: bool,
                variable_type, vol_scaler, kwargs) -> Tuple[List[np.ndarray], np.ndarray, int]:
    """the density route behind logsv_pdfs and logsv_pdfs_batch: the cases of one expansion order share one AnalyticGrid, one
    ODE launch and one inversion launch -> (bin masses per case, given-up counts per case, grid length)"""
    out: List[Optional[np.ndarray]] = [None] * len(params_list)
    given_up = np.zeros(len(params_list), dtype=int)
    n_grid = 0
    for order in sorted(set(orders)):
        idx = [i for i, o in enumerate(orders) if o == order]
        setups = [_pdf_setup(params_list[i], ttm, is_spot_measure, order, variable_type, vol_scaler) for i in idx]
        grid = AnalyticGrid.acquire([s[0] for s in setups], [s[1] for s in setups], 5 if order == 2 else 3)
        try:
            if any(np.any(s[2]) for s in setups):
                grid.set_a(np.stack([s[2] for s in setups]))
            rows = np.array([[p.sigma0, p.theta, p.kappa1, p.kappa2, p.beta, p.volvol, 1.0, 0.0]
                             for p in (params_list[i] for i in idx)])
            grid.logsv_advance(ttm, rows, is_spot_measure, order, rtol=kwargs.get("ode_rtol"), atol=kwargs.get("ode_atol"))
            spaces = [np.asarray(space_grids[i], dtype=np.float64) for i in idx]
            scales = [s[6] for s in setups]
            pdf = grid.pdf_sums([s[3] for s in setups], spaces, [s[5] for s in setups], scales, resident=setups[0][4])
            n_grid = grid.n
            for k, i in enumerate(idx):
                out[i] = (pdf[k] / scales[k]).reshape(spaces[k].shape)
                given_up[i] = grid.last_given_up[k]
        finally:
            grid.release()
    return out, given_up, n_grid


def logsv_pdfs(params: LogSvParams, ttm: float, space_grid: np.ndarray, is_stiff_solver: bool = False,
               is_analytic: bool = False, is_spot_measure: bool = True, expansion_order: ExpansionOrder = ExpansionOrder.SECOND,
               variable_type: VariableType = VariableType.LOG_RETURN, vol_scaler: float = None, **kwargs) -> np.ndarray:
    """model density of the log-return (1000-point phi grid), the annualised quadratic variance (40 000-point psi grid) or the
    volatility (5000-point theta grid) at `space_grid`, as the bin masses dx * density (reference :742-803): one launch
    integrating the coefficient ODEs from A(0) = get_init_conditions_a over ttm, one launch inverting over the space grid; the
    log-MGF stays on the device between them.  is_stiff_solver / is_analytic are accepted and answered by the one device
    integrator (warned once); grid points it gives up on are counted and warned about (LAST_ANALYTIC_GIVEN_UP).
    ode_rtol= / ode_atol= as logsv_chain_pricer.  This is logsv_pdfs_batch at one case."""
    note_integrator_flags(is_stiff_solver, is_analytic)
    out, given_up, n_grid = _logsv_pdfs([params], ttm, [space_grid], [_order_code(expansion_order)], is_spot_measure,
                                        variable_type, vol_scaler, kwargs)
    _note_given_up(int(given_up[0]), n_grid)
    return out[0]


def logsv_pdfs_batch(params_list: Sequence[LogSvParams], ttm: float, space_grids: Sequence[np.ndarray],
                     is_spot_measure: bool = True, expansion_orders=ExpansionOrder.SECOND,
                     variable_type: VariableType = VariableType.LOG_RETURN, vol_scaler: float = None, **kwargs
                     ) -> List[np.ndarray]:
    """logsv_pdfs for several cases of ONE variable, maturity and measure: case i has the parameters params_list[i], the space
    grid space_grids[i] (all of one length) and the expansion order expansion_orders[i] (one order for all when not a
    sequence).  The cases of one expansion order share one ODE launch and one inversion launch (the coefficient arrays of the
    two orders differ in width, so a list holding both orders takes two launches of each).  Not in the reference API: the
    batched form of the six calls behind one panel of its density figure."""
    params_list = list(params_list)
    if not isinstance(expansion_orders, (list, tuple)):
        expansion_orders = [expansion_orders] * len(params_list)
    if not (len(params_list) == len(space_grids) == len(expansion_orders)):
        raise ValueError("logsv_pdfs_batch: params_list, space_grids and expansion_orders must have one length")
    orders = [_order_code(o) for o in expansion_orders]
    spaces = [np.asarray(g, dtype=np.float64) for g in space_grids]
    if len({g.size for g in spaces}) > 1:
        raise ValueError("logsv_pdfs_batch: the space grids must have one length")
    out, given_up, n_grid = _logsv_pdfs(params_list, ttm, spaces, orders, is_spot_measure, variable_type, vol_scaler, kwargs)
    _note_given_up(given_up, n_grid)
    return out


def _broadcast_state(x0, vol0, qvar0, nb_path):
    """length-1 inputs are initial values (x0 -> x0*zeros, qvar0 -> zeros, vol0 -> vol0*ones); otherwise the
    vectors must have nb_path entries (reference :1007-1020, AssertionError)."""
    x0, vol0, qvar0 = np.asarray(x0, dtype=np.float64), np.asarray(vol0, dtype=np.float64), \
        np.asarray(qvar0, dtype=np.float64)
    if x0.shape[0] == 1:
        x0 = x0 * np.zeros(nb_path)
    else:
        assert x0.shape[0] == nb_path
    if qvar0.shape[0] == 1:
        qvar0 = np.zeros(nb_path)
    else:
        assert qvar0.shape[0] == nb_path
    if vol0.shape[0] == 1:
        vol0 = vol0 * np.ones(nb_path)
    else:
        assert vol0.shape[0] == nb_path
    return x0, vol0, qvar0


def simulate_logsv_x_vol_terminal(ttm: float, x0: np.ndarray, sigma0: np.ndarray, qvar0: np.ndarray, theta: float,
                                  kappa1: float, kappa2: float, beta: float, volvol: float,
                                  vol_backbone_eta: float = 1.0, is_spot_measure: bool = True, nb_path: int = 100000,
                                  nb_steps_per_year: int = 360, W0: Optional[np.ndarray] = None,
                                  W1: Optional[np.ndarray] = None, dt: Optional[float] = None,
                                  seed: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """terminal (x, sigma, qvar) after one slice of Eq. (3.59) (reference :950-1047).  W0/W1 are UNSCALED
    N(0,1) of shape [nb_steps, nb_path] with their `dt`; when omitted the increments are drawn on device."""
    x0, sigma0, qvar0 = _broadcast_state(x0, sigma0, qvar0, nb_path)
    eng = get_engine(nb_path)
    eng.set_state(x0, sigma0, qvar0)
    if W0 is None and W1 is None:
        nb_steps, dt = time_grid_steps(ttm=ttm, nb_steps_per_year=nb_steps_per_year)
        rng_seed, call_id = next_rng_call(seed)
        eng.logsv_rng(nb_steps, dt, theta, kappa1, kappa2, beta, volvol, vol_backbone_eta, is_spot_measure,
                      rng_seed, call_id, 0)
    else:
        W0, W1 = np.asarray(W0), np.asarray(W1)
        if W0.shape != W1.shape or W0.ndim != 2 or W0.shape[1] != nb_path:
            raise ValueError("W0 and W1 must both have shape [nb_steps, nb_path]")
        if dt is None:
            raise ValueError("dt must be supplied with W0 and W1")
        w0, w1 = eng.upload_randoms((W0, W1))
        eng.logsv_w(W0.shape[0], dt, theta, kappa1, kappa2, beta, volvol, vol_backbone_eta, is_spot_measure, w0, w1)
    return eng.get_state()


def simulate_vol_paths(ttm: float, v0: float, theta: float, kappa1: float, kappa2: float, beta: float, volvol: float,
                       is_spot_measure: bool = True, nb_path: int = 100000, nb_steps_per_year: int = 360,
                       brownians: np.ndarray = None, seed: Optional[int] = None, return_device: bool = False,
                       out: Optional[np.ndarray] = None, **kwargs) -> Tuple[np.ndarray, np.ndarray]:
    """sigma_t of shape (nb_steps + 1, nb_path), first row = v0, and the time grid (reference :870-947).
    `brownians` are the reference's SCALED increments sqrt(dt)*N(0,1), shape (nb_steps, nb_path).
    The array is 8 bytes per path-step -- 8.6 GB at 2^20 x 1024, two milliseconds to compute: by default it comes back as
    the reference's NumPy array through a pinned, pipelined download (into `out` when given); return_device=True leaves it in
    HBM as an engine.DeviceArray (zero-copy into torch / cupy, `.row_moments()`, `.numpy()`) -- see vol_path_moments()."""
    nb_steps, dt, grid_t = set_time_grid(ttm=ttm, nb_steps_per_year=nb_steps_per_year)
    if brownians is not None:
        brownians = np.asarray(brownians)
        if brownians.shape != (nb_steps, nb_path):
            raise ValueError("brownians must have shape (nb_steps, nb_path)")
    rng_seed, call_id = next_rng_call(seed)
    eng = get_engine(nb_path)
    sigma_t = eng.logsv_vol_paths(nb_steps, dt, v0, theta, kappa1, kappa2, beta, volvol, is_spot_measure, rng_seed,
                                  call_id, brownians=brownians, return_device=return_device, out_host=out)
    return sigma_t, grid_t


def vol_path_moments(ttm: float, v0: float, theta: float, kappa1: float, kappa2: float, beta: float, volvol: float,
                     is_spot_measure: bool = True, nb_path: int = 100000, nb_steps_per_year: int = 360, n_terms: int = 4,
                     center: Optional[float] = None, with_qvar: bool = False, seed: Optional[int] = None) -> dict:
    """What the reference's users of simulate_vol_paths compute from the array (papers/logsv_model_with_quadratic_drift/
    moments_vol_qvar.py:48, :98-104), without the array ever leaving the GPU: per time step the Monte Carlo mean and
    population standard deviation over the paths of (sigma_t - center)^k, k = 1 .. n_terms (center = theta by default, as in
    plot_vol_moments_vs_mc), and with with_qvar those of the expanding time average of sigma_t^2.  -> {"grid_t", "mean"
    [nb_steps + 1][n_terms], "std" (same shape; divide by sqrt(nb_path) for the standard error), "qvar_mean", "qvar_std"}."""
    sigma_t, grid_t = simulate_vol_paths(ttm=ttm, v0=v0, theta=theta, kappa1=kappa1, kappa2=kappa2, beta=beta, volvol=volvol,
                                         is_spot_measure=is_spot_measure, nb_path=nb_path, nb_steps_per_year=nb_steps_per_year,
                                         seed=seed, return_device="view")      # the engine's cached buffer: no 8.6 GB allocation per call
    try:
        mean, std = sigma_t.row_moments(center=theta if center is None else center, n_moments=n_terms)
        out = {"grid_t": grid_t, "mean": mean, "std": std}
        if with_qvar:
            q = sigma_t.expanding_mean_of_squares()
            try:
                qm, qs = q.row_moments(center=0.0, n_moments=1)
            finally:
                q.free()
            out["qvar_mean"], out["qvar_std"] = qm[:, 0], qs[:, 0]
        return out
    finally:
        sigma_t.free()
        get_engine(nb_path).trim_bulk()        # the views are done: cached path arrays beyond an eighth of the device's memory go back


def logsv_mc_chain_pricer(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                          strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray], v0: float,
                          theta: float, kappa1: float, kappa2: float, beta: float, volvol: float,
                          vol_backbone_etas: np.ndarray, is_spot_measure: bool = True, nb_path: int = 100000,
                          nb_steps_per_year: int = 360, variable_type: VariableType = VariableType.LOG_RETURN,
                          seed: Optional[int] = None, comm=None, devices=None, reduce: Optional[str] = None
                          ) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """chain MC with on-device randoms (reference :806-867): per slice nb_steps_i = int((T_i - T_{i-1})*spy) + 1.
    devices=N | [ids]: shard the paths over that many GPUs of THIS process (stochvolmodels_amd.multi: one session and one
    host thread per device inside libsvmc; reduce='auto' | 'host' | 'rccl' picks the all-reduce transport) -- the same
    numbers as one device up to the order of the final additions."""
    vt_code = variable_type_code(variable_type)
    if devices is not None:
        if comm is not None:
            raise ValueError("devices= (one process, several GPUs) and comm= (one process per GPU) are exclusive")
        from ..multi import get_multi_session
        rng_seed, call_id = next_rng_call(seed)
        ms = get_multi_session(devices, nb_path, len(ttms), sum(int(np.asarray(k).size) for k in strikes_ttms), reduce=reduce)
        return ms.price_logsv_chain(ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms, v0, theta, kappa1, kappa2,
                                    beta, volvol, vol_backbone_etas, is_spot_measure, nb_steps_per_year, vt_code, rng_seed,
                                    call_id)
    comm = comm or svdist.get_default_comm()
    rng_seed, call_id = next_rng_call(seed)
    if FUSED_MC_CHAIN_DRIVER and WHOLE_CHAIN_STEPPING and comm.world == 1:
        eng = get_engine(nb_path)
        if hasattr(eng, "price_logsv_chain_fused"):
            # one GPU: the whole chain is ONE call of the fused C driver on the engine's own state (the kernels of the route
            # below in the same order: the same bits; -21 us of interpreter and ctypes per call)
            ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, [option_type_codes(t) for t in optiontypes_ttms])
            prices, stderrs = eng.price_logsv_chain_fused(ch, v0, theta, kappa1, kappa2, beta, volvol, vol_backbone_etas,
                                                          is_spot_measure, nb_steps_per_year, vt_code, rng_seed, call_id)
            return chain_shaped(prices, strikes_ttms), chain_shaped(stderrs, strikes_ttms)
    grids = list(zip(*chain_step_grid(ttms, nb_steps_per_year)))
    return _logsv_mc_chain_on_grids(grids, rng_seed, call_id, comm, ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms,
                                    v0, theta, kappa1, kappa2, beta, volvol, vol_backbone_etas, is_spot_measure, nb_path,
                                    variable_type)


def check_conditional_request(who: str, variable_type, comm, devices, optiontypes_ttms, is_spot_measure: bool = True) -> list:
    """the requests the conditional Monte Carlo pricers refuse, before any device work (each a separate step):
    'IC' / 'IP' (ValueError("not implemented")), another variable than LOG_RETURN, the inverse measure, sharded paths.  Returns
    the per-expiry type codes."""
    codes = [tilted_type_codes(t) for t in optiontypes_ttms]                # ValueError("not implemented")
    if variable_type_code(variable_type) != 1:
        raise NotImplementedError(f"{who}: variable_type={variable_type}: the conditional estimator prices the log-return only")
    if not is_spot_measure:
        raise NotImplementedError(f"{who}: is_spot_measure=False: the conditional estimator covers the spot measure")
    refuse_sharded_paths(who, comm, devices)
    return codes


def refuse_sharded_paths(who: str, comm, devices) -> None:
    """the conditional routes step every path on one GPU"""
    if devices is not None or (comm or svdist.get_default_comm()).world > 1:
        raise NotImplementedError(f"{who}: sharded paths (comm.world > 1, devices=) are not covered")


def logsv_mc_chain_pricer_conditional(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                                      strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray], v0: float,
                                      theta: float, kappa1: float, kappa2: float, beta: float, volvol: float,
                                      vol_backbone_etas: np.ndarray, is_spot_measure: bool = True, nb_path: int = 100000,
                                      nb_steps_per_year: int = 360, variable_type: VariableType = VariableType.LOG_RETURN,
                                      seed: Optional[int] = None, comm=None, devices=None, reduce: Optional[str] = None,
                                      recenter: bool = True, return_stats: bool = False):
    """logsv_mc_chain_pricer by CONDITIONAL Monte Carlo (include/svmc.h): given the path of the volatility's
    driver the discretised log-return is Gaussian, so each path contributes a Black-76 price instead of a payoff -- the same
    expectation for the same discretised model, a smaller variance, one normal per step (random stream 8, not the plain pricer's:
    the two are independent estimates at equal seeds).  Same signature and (prices, stderrs) lists; return_stats=True adds per
    expiry the dict of engine.CMC_STATS_FIELDS (forward_mc = mean F_c, its standard error, corr, n_kept, n_dropped).
    recenter=False prices against the unrecentred strikes.  'C' / 'P', LOG_RETURN, the spot measure and one GPU only
    (check_conditional_request).  Not in the reference API."""
    codes = check_conditional_request("logsv_mc_chain_pricer_conditional", variable_type, comm, devices, optiontypes_ttms,
                                      is_spot_measure)
    rng_seed, call_id = next_rng_call(seed)
    ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, codes)
    prices, stderrs, stats = get_engine(nb_path).price_logsv_chain_cmc_fused(
        ch, v0, theta, kappa1, kappa2, beta, volvol, vol_backbone_etas, is_spot_measure, nb_steps_per_year, recenter, rng_seed, call_id)
    out = (chain_shaped(prices, strikes_ttms), chain_shaped(stderrs, strikes_ttms))
    return out + (stats,) if return_stats else out


def conditional_greeks_shaped(fields: dict, stats: list, strikes_ttms: Sequence[np.ndarray], return_stats: bool) -> dict:
    """an engine's (fields, stats) of the conditional Greeks as the function routes return them: chain-shaped lists per field of
    engine.CMC_GREEKS_FIELDS, and "stats" (per expiry the dict of engine.CMC_GREEKS_STATS_FIELDS) when asked"""
    out = {name: chain_shaped(rows, strikes_ttms) for name, rows in fields.items()}
    if return_stats:
        out["stats"] = stats
    return out


def logsv_mc_chain_greeks_conditional(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                                      strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray], v0: float,
                                      theta: float, kappa1: float, kappa2: float, beta: float, volvol: float,
                                      vol_backbone_etas: np.ndarray, is_spot_measure: bool = True, nb_path: int = 100000,
                                      nb_steps_per_year: int = 360, variable_type: VariableType = VariableType.LOG_RETURN,
                                      seed: Optional[int] = None, comm=None, devices=None, reduce: Optional[str] = None,
                                      recenter: bool = True, return_stats: bool = False, wrt: Optional[Sequence[str]] = (),
                                      rel_bump: float = 1e-3, bumps: Optional[dict] = None) -> dict:
    """logsv_mc_chain_pricer_conditional with the derivatives of its prices in the forward and the strike (include/svmc.h, DESIGN.md
    row f13): per path the Black-76 delta, dual delta and dual gamma in closed form, each with a standard error -- the exact
    derivatives of the number the conditional pricer returns at the same seed.  Same signature; returns a dict of chain-shaped
    lists: price, stderr (bit-equal to logsv_mc_chain_pricer_conditional), delta, delta_stderr, dual_delta, dual_delta_stderr,
    gamma, gamma_stderr, dual_gamma, dual_gamma_stderr; return_stats=True adds "stats", per expiry the dict of
    engine.CMC_GREEKS_STATS_FIELDS (the conditional pricer's and n_zero_cv, the kept paths whose conditional variance is zero: they
    add no gamma).  price = F delta + K dual_delta and F^2 gamma = K^2 dual_gamma hold to rounding.  With recenter=True the errors
    ignore the noise of the recentring mean, as the price's does.  Refusals: check_conditional_request's.  Not in the reference
    API.

    wrt (row f14; default (): nothing above changes): a sequence of parameter names, or None / "all" for sigma0 theta kappa1 kappa2
    beta volvol -- the parameter sensitivities of this estimator on common random numbers.  The base job and per name the pair at
    +- h (h = rel_bump |value| or bumps[name]; names, bump rules and ValueErrors are mc_greeks.greeks_bumps's) are stepped by ONE
    launch on one stream; the dict gains sens[name], sens_stderr[name] and n_pairs[name], chain-shaped: the central difference of
    the two bumped conditional prices and the error of that DIFFERENCE, with the delta-method term of the two recentring means.
    The ten fields above stay bit-equal to the call with wrt=().  At most 16 expiries."""
    who = "logsv_mc_chain_greeks_conditional"
    codes = check_conditional_request(who, variable_type, comm, devices, optiontypes_ttms, is_spot_measure)
    if not (wrt is None or isinstance(wrt, str) or len(wrt) > 0):
        rng_seed, call_id = next_rng_call(seed)
        ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, codes)
        fields, stats = get_engine(nb_path).price_logsv_chain_cmc_greeks_fused(
            ch, v0, theta, kappa1, kappa2, beta, volvol, vol_backbone_etas, is_spot_measure, nb_steps_per_year, recenter, rng_seed,
            call_id)
        return conditional_greeks_shaped(fields, stats, strikes_ttms, return_stats)
    values = dict(sigma0=v0, theta=theta, kappa1=kappa1, kappa2=kappa2, beta=beta, volvol=volvol)
    names, h = greeks_bumps("logsv", values, None if isinstance(wrt, str) and wrt == "all" else wrt, rel_bump, bumps)
    check_conditional_sens_expiries(who, ttms)
    etas = chain_etas(vol_backbone_etas, len(ttms))
    rows = greeks_job_table("logsv", np.concatenate([[values[k] for k in LOGSV_GREEK_PARAMS], etas]), names, h)
    rng_seed, call_id = next_rng_call(seed)
    ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, codes)
    fields, stats, sens = get_engine(nb_path).price_chain_cmc_sens_fused(ch, "logsv", rows, h, int(bool(is_spot_measure)),
                                                                         nb_steps_per_year, recenter, rng_seed, call_id)
    return conditional_sens_shaped(conditional_greeks_shaped(fields, stats, strikes_ttms, return_stats), sens, names, ch["slices"],
                                   strikes_ttms)


def check_conditional_sens_expiries(who: str, ttms) -> None:
    """the sensitivities ride on the many-job stepping launch: at most 16 expiries (refused before any device work)"""
    if len(ttms) > 16:
        raise NotImplementedError(f"{who}: wrt= takes at most 16 expiries, got {len(ttms)}")


def conditional_sens_shaped(out: dict, sens: np.ndarray, names: Sequence[str], slices, strikes_ttms) -> dict:
    """adds sens[name], sens_stderr[name] and n_pairs[name] (chain-shaped; the counts as integer arrays) from sens [P][3][K]"""
    cut = lambda row: chain_shaped([row[sl] for sl in slices], strikes_ttms)         # noqa: E731
    out["sens"] = {name: cut(sens[j, 0]) for j, name in enumerate(names)}
    out["sens_stderr"] = {name: cut(sens[j, 1]) for j, name in enumerate(names)}
    out["n_pairs"] = {name: [p.astype(np.int64) for p in cut(sens[j, 2])] for j, name in enumerate(names)}
    return out


def logsv_mc_chain_pricer_conditional_many(params_list: Sequence[LogSvParams], ttms: np.ndarray, forwards: np.ndarray,
                                           discfactors: np.ndarray, strikes_ttms: Sequence[np.ndarray],
                                           optiontypes_ttms: Sequence[np.ndarray], is_spot_measure: bool = True,
                                           nb_path: int = 100000, nb_steps_per_year: int = 360,
                                           variable_type: VariableType = VariableType.LOG_RETURN,
                                           seeds: Optional[Sequence[int]] = None, comm=None, devices=None, recenter: bool = True,
                                           return_stats: bool = False) -> list:
    """logsv_mc_chain_pricer_conditional for several independent jobs of ONE chain: job j has the parameters
    params_list[j] (with their vol-backbone etas) and its own random stream -- seeds[j] (call id 0), or with seeds=None the process
    seed and the next call id, taken in list order.  Returns per job what logsv_mc_chain_pricer_conditional(..., seed=seeds[j])
    returns, BIT FOR BIT: (prices, stderrs), with return_stats=True also the statistics.  Up to MANY_MAX_JOBS jobs are stepped by ONE
    launch (svmc_logsv_chain_price_cmc_many; longer lists in several calls, in order); more than 16 expiries run as a loop of single
    calls.  Refusals: check_conditional_request's.  Not in the reference API."""
    codes = check_conditional_request("logsv_mc_chain_pricer_conditional_many", variable_type, comm, devices, optiontypes_ttms,
                                      is_spot_measure)
    params_list = check_many_args(params_list, seeds)
    if not params_list:
        return []
    m = len(ttms)
    etas = [p.get_vol_backbone_etas(ttms=np.asarray(ttms, dtype=float)) for p in params_list]
    if m > 16:
        return [logsv_mc_chain_pricer_conditional(
            ttms=ttms, forwards=forwards, discfactors=discfactors, strikes_ttms=strikes_ttms, optiontypes_ttms=optiontypes_ttms,
            v0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2, beta=p.beta, volvol=p.volvol, vol_backbone_etas=e,
            is_spot_measure=is_spot_measure, nb_path=nb_path, nb_steps_per_year=nb_steps_per_year, variable_type=variable_type,
            seed=None if seeds is None else seeds[j], recenter=recenter, return_stats=return_stats)
            for j, (p, e) in enumerate(zip(params_list, etas))]
    streams = many_job_streams(len(params_list), seeds)
    rows = np.ones((len(params_list), 6 + m))
    for row, p in zip(rows, params_list):
        row[:6] = (p.sigma0, p.theta, p.kappa1, p.kappa2, p.beta, p.volvol)
    rows[:, 6:] = np.reshape(etas, (len(params_list), m))
    ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, codes)
    eng = get_engine(nb_path)
    out = []
    for _, part, job_seeds, ids in many_job_chunks(streams, rows):
        out += eng.price_chain_cmc_many_fused(ch, "logsv", part, job_seeds, ids, int(bool(is_spot_measure)), nb_steps_per_year, recenter)
    return conditional_many_shaped(out, strikes_ttms, return_stats)


def conditional_many_shaped(out: list, strikes_ttms: Sequence[np.ndarray], return_stats: bool) -> list:
    """every job's (prices, stderrs, stats) of the engine's many-job conditional call as the single function returns them"""
    shaped = [(chain_shaped(pr, strikes_ttms), chain_shaped(se, strikes_ttms), st) for pr, se, st in out]
    return shaped if return_stats else [(pr, se) for pr, se, _ in shaped]


def conditional_sets_on_engine(model: str, rows: np.ndarray, single, chain: tuple, codes, is_spot_measure: bool, nb_path: int,
                               nb_steps_per_year: int, seed: Optional[int], recenter: bool, return_ivols: bool,
                               return_stats: bool) -> list:
    """the body of the two *_mc_chain_pricer_conditional_sets functions: the sets `rows` ([P][6 + m] | [P][5]) of one chain on ONE
    (seed, call id) -- seed None: the process seed and ONE next call id -- in engine calls of up to CMC_SETS_MAX sets, in order.
    More than 16 expiries: single(q, seed, call_id) -> (prices, stderrs, stats), one conditional call per set on that stream, and
    the host routine's vols.  chain: (ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms).  Per set (prices, stderrs[,
    ivols][, stats]), chain-shaped."""
    if len(rows) == 0:
        return []
    rng_seed, call_id = next_rng_call(seed)
    ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms = chain
    if len(ttms) > 16:
        out = []
        for q in range(len(rows)):
            prices, stderrs, stats = single(q, rng_seed, call_id)
            ivols = [black_ivols_native(p, float(t), float(f), np.ravel(k), np.ravel(ty), float(d))
                     for p, t, f, k, ty, d in zip(prices, ttms, forwards, strikes_ttms, optiontypes_ttms, discfactors)] if return_ivols else None
            out.append((prices, stderrs, ivols, stats))
    else:
        ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, codes)
        eng = get_engine(nb_path)
        out = []
        for q0 in range(0, len(rows), CMC_SETS_MAX):
            out += eng.price_chain_cmc_sets_fused(ch, model, rows[q0:q0 + CMC_SETS_MAX], int(bool(is_spot_measure)), nb_steps_per_year,
                                                  recenter, rng_seed, call_id, want_ivols=return_ivols)
    shapes = [k.shape if isinstance(k, np.ndarray) else np.shape(k) for k in strikes_ttms]
    shaped = []
    for prices, stderrs, ivols, stats in out:
        one = (chain_shaped(prices, strikes_ttms, shapes), chain_shaped(stderrs, strikes_ttms, shapes))
        if return_ivols:
            one += (chain_shaped(ivols, strikes_ttms, shapes),)
        shaped.append(one + (stats,) if return_stats else one)
    return shaped


def logsv_mc_chain_pricer_conditional_sets(params_list: Sequence[LogSvParams], ttms: np.ndarray, forwards: np.ndarray,
                                           discfactors: np.ndarray, strikes_ttms: Sequence[np.ndarray],
                                           optiontypes_ttms: Sequence[np.ndarray], is_spot_measure: bool = True,
                                           nb_path: int = 100000, nb_steps_per_year: int = 360,
                                           variable_type: VariableType = VariableType.LOG_RETURN, seed: Optional[int] = None,
                                           recenter: bool = True, return_ivols: bool = False, return_stats: bool = False, comm=None,
                                           devices=None) -> list:
    """logsv_mc_chain_pricer_conditional for several parameter sets of ONE chain on ONE random stream: the
    evaluation of a calibration objective on a frozen stream.  Every set is priced on (seed, call 0) -- with seed=None on the process
    seed and ONE next call id -- and returns what logsv_mc_chain_pricer_conditional returns on that stream, BIT FOR BIT: (prices,
    stderrs), with return_ivols=True also the Black-76 implied vols of the prices (NaN outside [1e-6, 10]; computed by the graph's
    last kernel), with return_stats=True also the statistics.  Up to CMC_SETS_MAX sets are ONE replayed graph
    (svmc_logsv_chain_price_cmc_sets: the job table's upload, one stepping launch, one tail for all sets); longer lists go in
    several calls, in order, on the same stream; more than 16 expiries run as single conditional calls with the host routine's
    vols.  Refusals: check_conditional_request's.  Not in the reference API."""
    who = "logsv_mc_chain_pricer_conditional_sets"
    codes = check_conditional_request(who, variable_type, comm, devices, optiontypes_ttms, is_spot_measure)
    params_list = list(params_list)
    ttms = np.asarray(ttms, dtype=float)
    m = len(ttms)
    etas = [p.get_vol_backbone_etas(ttms=ttms) for p in params_list]
    rows = np.ones((len(params_list), 6 + m))
    for row, p, e in zip(rows, params_list, etas):
        row[:6] = (p.sigma0, p.theta, p.kappa1, p.kappa2, p.beta, p.volvol)
        row[6:] = np.ravel(e)
    chain = (ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms)

    def single(q: int, rng_seed: int, call_id: int):
        p = params_list[q]
        ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, codes)
        return get_engine(nb_path).price_logsv_chain_cmc_fused(ch, p.sigma0, p.theta, p.kappa1, p.kappa2, p.beta, p.volvol, etas[q],
                                                               is_spot_measure, nb_steps_per_year, recenter, rng_seed, call_id)
    return conditional_sets_on_engine("logsv", rows, single, chain, codes, is_spot_measure, nb_path, nb_steps_per_year, seed, recenter,
                                      return_ivols, return_stats)


def conditional_log_return_pdf(route, ttm: float, x_grid: np.ndarray, return_stderr: bool = False):
    """the density of the simulated log-return on x_grid from a conditional Greeks route (route(ttms=, forwards=, discfactors=,
    strikes_ttms=, optiontypes_ttms=) -> its dict): one expiry at forward 1 and discount factor 1 with calls at K_j = exp(x_j), and
    pdf(x_j) = K_j dual_gamma_j -- the density of the terminal spot at K_j times dK / dx.  Not normalised."""
    x = np.asarray(x_grid, dtype=np.float64)
    strikes = np.exp(x.ravel())
    out = route(ttms=np.array([float(ttm)]), forwards=np.array([1.0]), discfactors=np.array([1.0]), strikes_ttms=[strikes],
                optiontypes_ttms=[np.full(strikes.size, "C")])
    pdf = (strikes * out["dual_gamma"][0]).reshape(x.shape)
    if return_stderr:
        return pdf, (strikes * out["dual_gamma_stderr"][0]).reshape(x.shape)
    return pdf


def mixture_log_return_pdf(who: str, step_rows, x_grid: np.ndarray, risk_premia_gammas, nb_path: int, seed: Optional[int],
                           return_stderr: bool, return_stats: bool, variable_type=VariableType.LOG_RETURN, comm=None, devices=None,
                           is_spot_measure: bool = True):
    """the body of the three pricers' get_log_return_mc_pdf_mixture: the refusals of the conditional routes
    (check_conditional_request: variables other than the log-return, the inverse measure, comm= / devices=) and the checks of the
    points and gammas, each before any engine is asked for; the next (seed, call id) exactly as the conditional pricer takes it;
    step_rows(engine, seed, call_id) leaves the expiry's mu in snapshot row 0 and its cv in row 1 -- the rows the conditional pricer
    steps on that stream --; then ONE svmc_cond_density_chain for all gammas (engine.conditional_densities).  Without gammas: pdf
    in x_grid's shape (gamma 0); with: [gamma][x].  Then the standard error and the statistics (engine.CD_STATS_FIELDS; one dict,
    or one per gamma) when asked."""
    check_conditional_request(who, variable_type, comm, devices, [], is_spot_measure)
    single = risk_premia_gammas is None
    x = np.asarray(x_grid, dtype=np.float64)
    ch = cond_density_arrays([x], [0.0] if single else risk_premia_gammas)         # ValueError
    rng_seed, call_id = next_rng_call(seed)
    eng = get_engine(int(nb_path))
    step_rows(eng, rng_seed, call_id)
    pdf, err, stats = eng.conditional_densities([x], ch["gammas"], mu_rows=[0], cv_rows=[1])
    p, e = np.array([g[0] for g in pdf]), np.array([g[0] for g in err])
    st = [cond_density_stats_dicts(s)[0] for s in stats]
    out = (p[0] if single else p,)
    if return_stderr:
        out += (e[0] if single else e,)
    if return_stats:
        out += (st[0] if single else st,)
    return out[0] if len(out) == 1 else out


def one_expiry_grid(ttm: float, nb_steps_per_year: int) -> Tuple[int, float]:
    """(steps, dt) of one expiry from the origin as the fused chain drivers cut it (svmc_chain.hip expiry_grids)"""
    nbs, dts = chain_step_grid([ttm], nb_steps_per_year)
    return nbs[0], dts[0]


def logsv_mc_chain_greeks(params: LogSvParams, ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                          strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray],
                          wrt: Optional[Sequence[str]] = None, rel_bump: float = 1e-3, bumps: Optional[dict] = None,
                          nb_path: int = 100000, nb_steps_per_year: int = 360, seed: Optional[int] = None,
                          is_spot_measure: bool = True, variable_type: VariableType = VariableType.LOG_RETURN, comm=None,
                          devices=None) -> dict:
    """logsv_mc_chain_pricer with its Greeks (include/svmc.h), on common random numbers: the base parameters and,
    per name in wrt (default: sigma0 theta kappa1 kappa2 beta volvol), the pair at +- h (h = rel_bump |value|, or bumps[name]) are
    stepped by ONE launch on one random stream.  Returns a dict of chain-shaped lists: price, stderr (bit-equal to
    logsv_mc_chain_pricer at the same seed), delta, delta_stderr (the pathwise forward delta), dual_delta, dual_delta_stderr, n_itm,
    and per name sens[name], sens_stderr[name], n_pairs[name] -- the central difference of the two bumped prices and the error of
    that DIFFERENCE, from the per-path paired differences.  No gamma; 'C' / 'P', LOG_RETURN, the spot measure and one GPU only; a
    zero parameter needs an explicit bump and no bump may leave the parameter's domain (ValueError naming the parameter; mc_greeks.
    greeks_bumps).  The vol-backbone etas are held fixed.  Not in the reference API."""
    codes = check_greeks_request("logsv_mc_chain_greeks", variable_type, comm, devices, optiontypes_ttms, is_spot_measure)
    names, h = greeks_bumps("logsv", {k: getattr(params, k) for k in LOGSV_GREEK_PARAMS}, wrt, rel_bump, bumps)
    etas = np.asarray(params.get_vol_backbone_etas(ttms=np.asarray(ttms, dtype=float)), dtype=np.float64)
    rows = greeks_job_table("logsv", np.concatenate([[getattr(params, k) for k in LOGSV_GREEK_PARAMS], etas]), names, h)
    rng_seed, call_id = next_rng_call(seed)
    ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, codes)
    prices, stderrs, base, sens = get_engine(nb_path).price_chain_greeks_fused(ch, "logsv", rows, h, int(bool(is_spot_measure)),
                                                                               nb_steps_per_year, rng_seed, call_id)
    return greeks_shaped(prices, stderrs, base, sens, names, ch["slices"], strikes_ttms)


def logsv_mc_chain_pricer_many(params_list: Sequence[LogSvParams], ttms: np.ndarray, forwards: np.ndarray,
                               discfactors: np.ndarray, strikes_ttms: Sequence[np.ndarray],
                               optiontypes_ttms: Sequence[np.ndarray], is_spot_measure: bool = True, nb_path: int = 100000,
                               nb_steps_per_year: int = 360, variable_type: VariableType = VariableType.LOG_RETURN,
                               seeds: Optional[Sequence[int]] = None, comm=None, devices=None
                               ) -> List[Tuple[List[np.ndarray], List[np.ndarray]]]:
    """logsv_mc_chain_pricer for several independent jobs of ONE chain: job j has the parameters params_list[j] (with their
    vol-backbone etas) and its own random stream -- seeds[j] (call id 0), or with seeds=None the process seed and the next call
    id, taken in list order.  Returns [(prices, stderrs)] per job, each BIT-EQUAL to logsv_mc_chain_pricer(..., seed=seeds[j])
    (or to the j-th of as many consecutive unseeded calls).  On one GPU up to MANY_MAX_JOBS jobs are stepped by ONE launch
    (svmc_logsv_chain_price_many; longer lists in several calls, in order); with comm.world > 1, devices=, or more than 16
    expiries it is a loop of single calls -- the same numbers.  Not in the reference API."""
    params_list = check_many_args(params_list, seeds)
    if not params_list:
        return []
    comm = comm or svdist.get_default_comm()
    m = len(ttms)
    etas = [p.get_vol_backbone_etas(ttms=np.asarray(ttms, dtype=float)) for p in params_list]
    if devices is not None or comm.world > 1 or m > 16 or not (FUSED_MC_CHAIN_DRIVER and WHOLE_CHAIN_STEPPING):
        # a loop of single calls (a sharded batch is out of scope): each takes its own stream, unseeded ones in list order
        return [logsv_mc_chain_pricer(ttms=ttms, forwards=forwards, discfactors=discfactors, strikes_ttms=strikes_ttms,
                                      optiontypes_ttms=optiontypes_ttms, v0=p.sigma0, theta=p.theta, kappa1=p.kappa1,
                                      kappa2=p.kappa2, beta=p.beta, volvol=p.volvol, vol_backbone_etas=e,
                                      is_spot_measure=is_spot_measure, nb_path=nb_path, nb_steps_per_year=nb_steps_per_year,
                                      variable_type=variable_type, seed=None if seeds is None else seeds[j], comm=comm,
                                      devices=devices)
                for j, (p, e) in enumerate(zip(params_list, etas))]
    streams = many_job_streams(len(params_list), seeds)
    rows = np.ones((len(params_list), 6 + m))
    for row, p in zip(rows, params_list):
        row[:6] = (p.sigma0, p.theta, p.kappa1, p.kappa2, p.beta, p.volvol)
    rows[:, 6:] = np.reshape(etas, (len(params_list), m))
    ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, [option_type_codes(t) for t in optiontypes_ttms])
    eng = get_engine(nb_path)
    out = []
    for _, part, job_seeds, ids in many_job_chunks(streams, rows):
        out += eng.price_chain_many_fused(ch, "logsv", part, job_seeds, ids, int(bool(is_spot_measure)), nb_steps_per_year,
                                          variable_type_code(variable_type))
    return many_jobs_shaped(out, strikes_ttms)


def _logsv_mc_chain_on_grids(grids, rng_seed: int, call_id: int, comm, ttms, forwards, discfactors, strikes_ttms,
                             optiontypes_ttms, v0, theta, kappa1, kappa2, beta, volvol, vol_backbone_etas, is_spot_measure,
                             nb_path, variable_type) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """the on-device-RNG chain on explicit per-expiry grids [(nb_steps_i, dt_i)] and an explicit stream (seed, call id):
    logsv_mc_chain_pricer after its bookkeeping, and what a chain on FROZEN randoms (DeviceRandoms.frozen) runs when it is
    sharded over ranks"""
    offset, n_local = svdist.shard_range(nb_path, comm.rank, comm.world)
    eng = get_engine(n_local, path_offset=offset)
    step0 = [0]
    for g in grids:
        step0.append(step0[-1] + g[0])
    start = (0.0, v0, 0.0)     # every path's start state (reference :823-826) goes to the first stepping launch as constants

    def advance(i: int, forward: float, snap_row: int, qvar_row, spot_ptr: int) -> None:
        nb, dt = grids[i]
        eng.logsv_slice_rng(nb, dt, theta, kappa1, kappa2, beta, volvol, float(vol_backbone_etas[i]), is_spot_measure,
                            rng_seed, call_id, int(step0[i]), forward, snap_row, qvar_row, spot_ptr,
                            start=start if i == 0 else None)

    def advance_chain(need_qvar: bool, spot_ptr: int) -> None:
        eng.logsv_chain_rng([g[0] for g in grids], [g[1] for g in grids], vol_backbone_etas, forwards, theta, kappa1,
                            kappa2, beta, volvol, is_spot_measure, rng_seed, call_id, 0, need_qvar, spot_ptr, start=start)

    return price_chain_on_engine(eng, comm, nb_path, ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms,
                                 variable_type, advance,
                                 advance_chain=advance_chain if (WHOLE_CHAIN_STEPPING and len(grids) > 1) else None)


def get_randoms_for_chain_valuation(ttms: np.ndarray, nb_path: int = 100000, nb_steps_per_year: int = 360,
                                    seed: int = 10) -> Tuple[List[np.ndarray], List[np.ndarray], List[float]]:
    """host-side fixed randoms, identical to the reference (:1051-1074): a local RandomState(seed) draws, per
    slice, W0 then W1 of shape [nb_steps_i, nb_path]; the global NumPy RNG is untouched."""
    rng = np.random.RandomState(seed)
    W0s, W1s = [], []
    nbs, dts = chain_step_grid(ttms, nb_steps_per_year)
    for nb in nbs:
        W0s.append(rng.normal(0, 1, size=(nb, nb_path)))
        W1s.append(rng.normal(0, 1, size=(nb, nb_path)))
    return W0s, W1s, dts


def upload_fixed_randoms(W0s: Sequence[np.ndarray], W1s: Sequence[np.ndarray], dts: Sequence[float], comm=None
                         ) -> DeviceRandoms:
    """copy the chain's fixed randoms to HBM once (this rank's path columns); pass the result as `W0s` to
    logsv_mc_chain_pricer_fixed_randoms.  This is what makes an MC calibration loop kernel-bound instead of
    PCIe-bound (reference logsv_pricer.py:520-527 draws the randoms once and re-prices per optimizer iterate)."""
    comm = comm or svdist.get_default_comm()
    offset, n_local = svdist.shard_range(np.asarray(W0s[0]).shape[1], comm.rank, comm.world)
    return DeviceRandoms(W0s, W1s, dts, n_local, offset)


def draw_fixed_randoms_on_device(ttms: np.ndarray, nb_path: int = 100000, nb_steps_per_year: int = 360, seed: int = 10,
                                 comm=None, in_hbm: bool = False) -> DeviceRandoms:
    """the device-side twin of get_randoms_for_chain_valuation + upload_fixed_randoms (no reference counterpart): the
    same per-expiry grids, the N(0,1) draws of the counter-based generator -- the draws logsv_mc_chain_pricer(seed=seed)
    consumes at its call 0 -- frozen.  By default NOTHING is stored: the object is the stream's definition (seed, call 0)
    and every pricing on it regenerates the same normals in registers (DeviceRandoms.frozen), bit-identical to
    logsv_mc_chain_pricer on that stream.  in_hbm=True materialises them in HBM instead (16 bytes per path-step, priced
    by the streamed-randoms kernels in the reference's evaluation order: the same draws, rounding-level different prices).
    Either way statistically equivalent to, not bit-identical with, the RandomState(seed) arrays of the reference."""
    comm = comm or svdist.get_default_comm()
    offset, n_local = svdist.shard_range(nb_path, comm.rank, comm.world)
    grids = list(zip(*chain_step_grid(ttms, nb_steps_per_year)))
    get_engine(n_local, path_offset=offset)               # the library and the device are up before the first launch
    make = DeviceRandoms.drawn_on_device if in_hbm else DeviceRandoms.frozen
    return make([g[0] for g in grids], [g[1] for g in grids], nb_path, n_local, offset, seed)


def logsv_mc_chain_pricer_fixed_randoms(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                                        strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray],
                                        W0s: Sequence[np.ndarray], W1s: Sequence[np.ndarray], dts: Sequence[float],
                                        v0: float, theta: float, kappa1: float, kappa2: float, beta: float,
                                        volvol: float, vol_backbone_etas: np.ndarray, is_spot_measure: bool = True,
                                        variable_type: VariableType = VariableType.LOG_RETURN, comm=None,
                                        return_ivols: bool = False) -> Tuple[List[np.ndarray], ...]:
    """chain MC on supplied randoms (reference :1100-1162): nb_path = W0s[0].shape[1]; each rank uploads only
    its own column range of the host arrays.  W0s may instead be a DeviceRandoms (upload_fixed_randoms): the
    randoms then stay in HBM across calls and W1s / dts are taken from it."""
    variable_type_code(variable_type)
    comm = comm or svdist.get_default_comm()
    resident = W0s if isinstance(W0s, DeviceRandoms) else None
    nb_path = resident.nb_path if resident else np.asarray(W0s[0]).shape[1]
    offset, n_local = svdist.shard_range(nb_path, comm.rank, comm.world)
    if resident and (resident.n_local, resident.col0) != (n_local, offset):
        raise ValueError("DeviceRandoms were uploaded for a different path shard")
    if FUSED_FIXED_RANDOMS_DRIVER and resident and comm.world == 1 and len(resident) == len(ttms):
        # single GPU, randoms resident: the whole chain in one call of the fused C++ driver
        strikes = [np.ascontiguousarray(np.asarray(k, dtype=np.float64)) for k in strikes_ttms]
        codes = [option_type_codes(t) for t in optiontypes_ttms]
        out = resident.price_logsv_chain(ttms, forwards, discfactors, [k.ravel() for k in strikes],
                                         [c.ravel() for c in codes], v0, theta, kappa1, kappa2, beta, volvol,
                                         vol_backbone_etas, is_spot_measure, variable_type_code(variable_type),
                                         want_ivols=return_ivols)
        return tuple(chain_shaped(part, strikes_ttms) for part in out)
    if resident and resident.is_frozen:
        # frozen randoms, sharded over ranks (or the fused driver switched off): the on-device-RNG chain on the stream the
        # object names -- the same numbers the fused route gives on one GPU
        fr_seed, fr_call = resident.frozen_stream
        prices, stderrs = _logsv_mc_chain_on_grids(list(zip(resident.nb_steps, resident.dts)), fr_seed, fr_call, comm, ttms,
                                                   forwards, discfactors, strikes_ttms, optiontypes_ttms, v0, theta, kappa1,
                                                   kappa2, beta, volvol, vol_backbone_etas, is_spot_measure, nb_path,
                                                   variable_type)
        if not return_ivols:
            return prices, stderrs
        return prices, stderrs, _host_ivols(prices, ttms, forwards, strikes_ttms, optiontypes_ttms, discfactors)
    eng = get_engine(n_local, path_offset=offset)
    eng.fill_state(0.0, v0, 0.0)

    def advance(i: int, forward: float, snap_row: int, qvar_row, spot_ptr: int) -> None:
        if resident:
            eng.logsv_slice_w(resident.nb_steps[i], resident.dts[i], theta, kappa1, kappa2, beta, volvol,
                              float(vol_backbone_etas[i]), is_spot_measure, resident.w0[i].ptr, resident.w1[i].ptr,
                              forward, snap_row, qvar_row, spot_ptr)
            return
        W0, W1 = np.asarray(W0s[i]), np.asarray(W1s[i])
        if W0.shape != W1.shape or W0.shape[1] != nb_path:
            raise ValueError("every W0/W1 must have shape [nb_steps_i, nb_path]")
        w0, w1 = eng.upload_randoms((W0, W1), col0=offset)
        eng.logsv_slice_w(W0.shape[0], float(dts[i]), theta, kappa1, kappa2, beta, volvol,
                          float(vol_backbone_etas[i]), is_spot_measure, w0, w1, forward, snap_row, qvar_row, spot_ptr)

    prices, stderrs = price_chain_on_engine(eng, comm, nb_path, ttms, forwards, discfactors, strikes_ttms,
                                            optiontypes_ttms, variable_type, advance)
    if not return_ivols:
        return prices, stderrs
    return prices, stderrs, _host_ivols(prices, ttms, forwards, strikes_ttms, optiontypes_ttms, discfactors)


def _host_ivols(prices, ttms, forwards, strikes_ttms, optiontypes_ttms, discfactors) -> List[np.ndarray]:
    from ..data.option_chain import black_ivols_native           # the host twin of the graph's implied-vol kernel
    return [black_ivols_native(np.asarray(p, dtype=float).ravel(), float(t), float(f), np.asarray(k, dtype=float).ravel(),
                               np.asarray(ty).ravel(), float(d)).reshape(np.shape(k))
            for p, t, f, k, ty, d in zip(prices, ttms, forwards, strikes_ttms, optiontypes_ttms, discfactors)]


def logsv_mc_chain_pricer_fixed_randoms_batch(params_list: Sequence[LogSvParams], ttms: np.ndarray, forwards: np.ndarray,
                                              discfactors: np.ndarray, strikes_ttms: Sequence[np.ndarray],
                                              optiontypes_ttms: Sequence[np.ndarray], W0s: DeviceRandoms,
                                              is_spot_measure: bool = True,
                                              variable_type: VariableType = VariableType.LOG_RETURN,
                                              return_ivols: bool = False, comm=None) -> List[Tuple[List[np.ndarray], ...]]:
    """logsv_mc_chain_pricer_fixed_randoms for SEVERAL parameter sets on the same resident randoms (W0s: the result of
    upload_fixed_randoms / draw_fixed_randoms_on_device): per set the (prices, stderrs[, ivols]) of a single call, the
    same bits.  On one GPU, 2..8 sets go through ONE replayed graph whose stepping launch reads the randoms once for all
    sets (svmc_logsv_chain_price_fixed_sets) -- the base point of an SLSQP iterate and its finite-difference neighbours;
    otherwise the sets are priced one after the other.  Not in the reference API."""
    vt = variable_type_code(variable_type)
    comm = comm or svdist.get_default_comm()
    if not isinstance(W0s, DeviceRandoms):
        raise TypeError("the batched pricer works on resident randoms (upload_fixed_randoms / draw_fixed_randoms_on_device)")
    codes = [option_type_codes(t) for t in optiontypes_ttms]
    if comm.world == 1 and FUSED_FIXED_RANDOMS_DRIVER and len(W0s) == len(ttms):
        strikes = [np.ascontiguousarray(np.asarray(k, dtype=np.float64)) for k in strikes_ttms]
        rows = np.ones((len(params_list), 6 + len(ttms)))
        for row, p in zip(rows, params_list):
            row[:6] = (p.sigma0, p.theta, p.kappa1, p.kappa2, p.beta, p.volvol)
            if p.vol_backbone is not None:
                row[6:] = p.get_vol_backbone_etas(ttms=ttms)
        out = []
        for q0 in range(0, len(params_list), 8):                      # a launch takes up to 8 sets
            out += W0s.price_logsv_chain_sets(ttms, forwards, discfactors, [k.ravel() for k in strikes],
                                              [c.ravel() for c in codes], rows[q0:q0 + 8], is_spot_measure, vt,
                                              want_ivols=return_ivols)
        if all(np.ndim(k) == 1 for k in strikes_ttms):
            return out
        return [tuple(chain_shaped(part, strikes_ttms) for part in res) for res in out]
    return [logsv_mc_chain_pricer_fixed_randoms(ttms=ttms, forwards=forwards, discfactors=discfactors,
                                                strikes_ttms=strikes_ttms, optiontypes_ttms=optiontypes_ttms, W0s=W0s,
                                                W1s=None, dts=None, v0=p.sigma0, theta=p.theta, kappa1=p.kappa1,
                                                kappa2=p.kappa2, beta=p.beta, volvol=p.volvol,
                                                vol_backbone_etas=p.get_vol_backbone_etas(ttms=ttms),
                                                is_spot_measure=is_spot_measure, variable_type=variable_type, comm=comm,
                                                return_ivols=return_ivols) for p in params_list]


# ---------------------------------------------------------------------------------------------------
# rough LogSV (Markovian lift of the fractional kernel), reference :1075-1232
# ---------------------------------------------------------------------------------------------------
def get_randoms_for_rough_vol_chain_valuation(ttms: np.ndarray, nb_path: int = 100000, nb_steps_per_year: int = 360,
                                              seed: int = 10) -> Tuple[np.ndarray, np.ndarray, List[np.ndarray]]:
    """host randoms and per-expiry time grids, identical to the reference (:1075-1097): every expiry has its own
    grid from 0 to T_i with int(T_i*spy)+1 steps; Z0 then Z1 of shape [nb_steps_last, nb_path] from a local
    RandomState(seed)."""
    rng = np.random.RandomState(seed)
    grids = [set_time_grid(ttm=ttm, nb_steps_per_year=nb_steps_per_year)[2] for ttm in ttms]
    nb_last = grids[-1].size - 1
    Z0 = rng.normal(0, 1, size=(nb_last, nb_path))
    Z1 = rng.normal(0, 1, size=(nb_last, nb_path))
    return Z0, Z1, grids


def upload_rough_randoms(Z0: np.ndarray, Z1: np.ndarray, comm=None) -> DeviceRandoms:
    """copy the rough chain's Z0 / Z1 to HBM once (this rank's path columns); pass the result as `Z0` to
    rough_logsv_mc_chain_pricer_fixed_randoms"""
    comm = comm or svdist.get_default_comm()
    offset, n_local = svdist.shard_range(np.asarray(Z0).shape[1], comm.rank, comm.world)
    return DeviceRandoms([Z0], [Z1], [0.0], n_local, offset)


def _rough_finalize(normalize_stderr: bool):
    """The reference passes a [1, nb_path] log-spot to compute_mc_vars_payoff, whose "/ sqrt(x0.shape[0])"
    (utils/mc_payoffs.py:88) then divides by 1: its second return is the payoff's standard deviation.  Reproduced
    by default; normalize_stderr=True returns the standard error instead."""
    if normalize_stderr:
        return payoff_finalize

    def finalize(sums, shifts, discfactor, n_path_total):
        p, e = payoff_finalize(sums, shifts, discfactor, n_path_total)
        return p, e * np.sqrt(n_path_total)
    return finalize


def _rough_coefficients(sigma0, beta, orthog_vol, weights, nodes):
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    nodes = np.ascontiguousarray(nodes, dtype=np.float64)
    if not (weights.ndim == 1 and weights.shape == nodes.shape):
        raise AssertionError("weights and nodes must be 1-d arrays of one shape")      # reference :1188
    if not 1 <= nodes.size <= 3:
        raise NotImplementedError("the Markovian lift is built for 1 to 3 factors (LogSvParams.approximate_kernel)")
    v0 = np.full(nodes.size, sigma0 / np.sum(weights))
    volvol = float(np.sqrt(beta ** 2 + orthog_vol ** 2))
    return weights, nodes, v0, float(beta / volvol), volvol


def rough_logsv_mc_chain_pricer_fixed_randoms(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                                              strikes_ttms: Sequence[np.ndarray],
                                              optiontypes_ttms: Sequence[np.ndarray], Z0: np.ndarray, Z1: np.ndarray,
                                              sigma0: float, theta: float, kappa1: float, kappa2: float, beta: float,
                                              orthog_vol: float, weights: np.ndarray, nodes: np.ndarray,
                                              timegrids: Sequence[np.ndarray],
                                              variable_type: VariableType = VariableType.LOG_RETURN,
                                              debug: bool = False, comm=None, normalize_stderr: bool = False
                                              ) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """rough-LogSV chain on supplied N(0,1) draws (reference :1164-1232).  Z0 may be the result of
    upload_rough_randoms (Z1 is then ignored); otherwise Z0/Z1 go to HBM once per call (this rank's path columns); every expiry is then one kernel that re-simulates from time 0 over the first len(timegrid_i)-1 rows
    with step timegrid_i[1]-timegrid_i[0], exactly as the reference does."""
    variable_type_code(variable_type)
    weights, nodes, v0, rho, volvol = _rough_coefficients(sigma0, beta, orthog_vol, weights, nodes)
    comm = comm or svdist.get_default_comm()
    resident = Z0 if isinstance(Z0, DeviceRandoms) else None
    if resident is None:
        Z0, Z1 = np.asarray(Z0), np.asarray(Z1)
        if Z0.ndim != 2 or Z0.shape != Z1.shape:
            raise ValueError("Z0 and Z1 must both have shape [nb_steps, nb_path]")
    nb_path = resident.nb_path if resident else Z0.shape[1]
    nb_rows = resident.nb_steps[0] if resident else Z0.shape[0]
    nbs = [int(np.asarray(g).size) - 1 for g in timegrids]
    if len(nbs) != len(ttms) or max(nbs) > nb_rows or min(nbs) < 1:
        raise ValueError("one time grid per maturity, each with at most Z0.shape[0] steps")
    offset, n_local = svdist.shard_range(nb_path, comm.rank, comm.world)
    if resident and (resident.n_local, resident.col0) != (n_local, offset):
        raise ValueError("DeviceRandoms were uploaded for a different path shard")
    eng = get_engine(n_local, path_offset=offset)
    if resident:
        z0, z1 = resident.w0[0].ptr, resident.w1[0].ptr
    else:
        z0, z1 = eng.upload_randoms((Z0[:max(nbs)], Z1[:max(nbs)]), col0=offset)

    def advance(i: int, forward: float, snap_row: int, qvar_row, spot_ptr: int) -> None:
        h = float(timegrids[i][1] - timegrids[i][0])
        eng.rough_logsv(nbs[i], h, nodes, weights, v0, theta, kappa1, kappa2, rho, volvol, z0, z1,
                        slice_out=(forward, snap_row, qvar_row, spot_ptr))
        if debug:
            x, _, _ = eng.get_state()
            vw = weights @ eng.get_factors(nodes.size)
            print(f"Number of paths with negative vol: {np.sum(vw < 0.0)}, nan vol: {np.count_nonzero(np.isnan(vw))}")
            print(f"Mean spot Strand: {np.mean(np.exp(x))}, nan spots: {np.count_nonzero(np.isnan(x))}")

    def advance_chain(need_q: bool, spot_ptr: int) -> None:
        # the expiries are independent simulations from time 0 (:1206-1216): all of them in one launch, side by side
        eng.rough_logsv_chain(nbs, [float(g[1] - g[0]) for g in timegrids], forwards, nodes, weights, v0, theta, kappa1, kappa2,
                              rho, volvol, need_q, spot_ptr, z0_ptr=z0, z1_ptr=z1)

    one_launch = ROUGH_CHAIN_ONE_LAUNCH and not debug and len(nbs) <= 16 and hasattr(eng, "rough_logsv_chain")
    return price_chain_on_engine(eng, comm, nb_path, ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms,
                                 variable_type, advance, finalize=_rough_finalize(normalize_stderr),
                                 advance_chain=advance_chain if one_launch else None)


def rough_logsv_mc_chain_pricer(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                                strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray],
                                sigma0: float, theta: float, kappa1: float, kappa2: float, beta: float,
                                orthog_vol: float, weights: np.ndarray, nodes: np.ndarray, nb_path: int = 100000,
                                nb_steps_per_year: int = 360, variable_type: VariableType = VariableType.LOG_RETURN,
                                seed: Optional[int] = None, comm=None, normalize_stderr: bool = False
                                ) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """addition (no reference counterpart): the same chain with the N(0,1) draws generated in the kernel (stream 3 of
    the counter-based generator), so nothing but the chain itself crosses PCIe.  Expiry i uses the draws of steps
    0..nb_steps_i-1, i.e. the same nesting of randoms over expiries as the fixed-randoms pricer."""
    variable_type_code(variable_type)
    weights, nodes, v0, rho, volvol = _rough_coefficients(sigma0, beta, orthog_vol, weights, nodes)
    comm = comm or svdist.get_default_comm()
    offset, n_local = svdist.shard_range(nb_path, comm.rank, comm.world)
    eng = get_engine(n_local, path_offset=offset)
    rng_seed, call_id = next_rng_call(seed)
    grids = [set_time_grid(ttm=ttm, nb_steps_per_year=nb_steps_per_year)[:2] for ttm in ttms]

    def advance(i: int, forward: float, snap_row: int, qvar_row, spot_ptr: int) -> None:
        nb, h = grids[i]
        eng.rough_logsv(nb, h, nodes, weights, v0, theta, kappa1, kappa2, rho, volvol, seed=rng_seed, call_id=call_id,
                        slice_out=(forward, snap_row, qvar_row, spot_ptr))

    def advance_chain(need_q: bool, spot_ptr: int) -> None:
        eng.rough_logsv_chain([g[0] for g in grids], [g[1] for g in grids], forwards, nodes, weights, v0, theta, kappa1, kappa2,
                              rho, volvol, need_q, spot_ptr, seed=rng_seed, call_id=call_id)

    one_launch = ROUGH_CHAIN_ONE_LAUNCH and len(grids) <= 16 and hasattr(eng, "rough_logsv_chain")
    return price_chain_on_engine(eng, comm, nb_path, ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms,
                                 variable_type, advance, finalize=_rough_finalize(normalize_stderr),
                                 advance_chain=advance_chain if one_launch else None)
