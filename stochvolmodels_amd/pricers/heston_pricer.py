"""
Heston Monte Carlo on MI355X: drop-in for the MC part of the reference's pricers/heston_pricer.py
(HestonParams :27-41, model_mc_price_chain :68-87, simulate_terminal_values :89-108,
heston_mc_chain_pricer :285-331, simulate_heston_x_vol_terminal :334-381).

The reference's only scheme is an Euler step with the variance floored at 1e-4; it is the default here
(scheme="euler").  scheme="qe" selects Andersen's QE-M (new capability; validated against the reference's
analytic Heston prices).  `nb_steps_per_year` is exposed on the chain driver with the reference's fixed
value 360 as default; `seed=` and `comm=` as in logsv_pricer.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .. import dist as svdist
from ..data.option_chain import OptionChain
from ..engine import HESTON_EULER_FLOOR, HESTON_QE, get_engine, marshalled_chain, option_type_codes
from ..mc_chain import (chain_shaped, check_many_args, many_job_chunks, many_job_streams, many_jobs_shaped, price_chain_on_engine,
                        variable_type_code)
from ..mc_greeks import HESTON_GREEK_PARAMS, check_greeks_request, greeks_bumps, greeks_job_table, greeks_shaped
from ..utils.calibration import ImpliedVolObjective, chain_calibration_weights, minimize_slsqp
from ..utils.config import VariableType
from ..utils.funcs import chain_step_grid, next_rng_call, set_time_grid, time_grid_steps, timer
from ..analytic import AnalyticGrid, chain_prices_from_sums, chain_sums
from ..utils import mgf_pricer as mgfp
from .logsv_pricer import (_broadcast_state, check_conditional_request, check_conditional_sens_expiries, conditional_greeks_shaped,
                           conditional_log_return_pdf, conditional_many_shaped, conditional_sens_shaped, conditional_sets_on_engine,
                           mixture_log_return_pdf, one_expiry_grid)
from .model_pricer import ModelParams, ModelPricer


@dataclass
class HestonParams(ModelParams):
    """dv = kappa (theta - v) dt + volvol sqrt(v) dW, rho = corr(dS, dv)."""
    v0: float = 0.04
    theta: float = 0.04
    kappa: float = 4.0
    rho: float = -0.5
    volvol: float = 0.4


BTC_HESTON_PARAMS = HestonParams(v0=0.8, theta=1.0, kappa=2.0, rho=0.0, volvol=2.0)


def _scheme_code(scheme) -> int:
    if scheme in (HESTON_EULER_FLOOR, "euler", "euler_floor", None):
        return HESTON_EULER_FLOOR
    if scheme in (HESTON_QE, "qe", "QE"):
        return HESTON_QE
    raise ValueError(f"unknown Heston scheme {scheme!r} (use 'euler' or 'qe')")


# heston_mc_chain_pricer steps all expiries of a multi-expiry chain in one launch (svmc_heston_chain_rng) when True
WHOLE_CHAIN_STEPPING = True
# single-GPU chains go through svmc_heston_chain_price on the engine's own state (one C-ABI call per chain) when True
FUSED_MC_CHAIN_DRIVER = True


class HestonPricer(ModelPricer):

    def price_chain(self, option_chain: OptionChain, params: HestonParams, **kwargs) -> List[np.ndarray]:
        """analytic chain prices by Fourier inversion of the closed-form MGF (reference :52-66)"""
        return heston_chain_pricer(v0=params.v0, theta=params.theta, kappa=params.kappa, volvol=params.volvol,
                                   rho=params.rho, ttms=option_chain.ttms, forwards=option_chain.forwards,
                                   discfactors=option_chain.discfactors, strikes_ttms=option_chain.strikes_ttms,
                                   optiontypes_ttms=option_chain.optiontypes_ttms,
                                   variable_type=kwargs.get("variable_type", VariableType.LOG_RETURN))

    def model_mc_price_chain(self, option_chain: OptionChain, params: HestonParams, nb_path: int = 100000,
                             variable_type: VariableType = VariableType.LOG_RETURN, **kwargs
                             ) -> Tuple[List[np.ndarray], List[np.ndarray]]:
        return heston_mc_chain_pricer(v0=params.v0, theta=params.theta, kappa=params.kappa, rho=params.rho,
                                      volvol=params.volvol, ttms=option_chain.ttms, forwards=option_chain.forwards,
                                      discfactors=option_chain.discfactors, strikes_ttms=option_chain.strikes_ttms,
                                      optiontypes_ttms=option_chain.optiontypes_ttms, nb_path=nb_path,
                                      variable_type=variable_type, scheme=kwargs.get("scheme", "euler"),
                                      nb_steps_per_year=kwargs.get("nb_steps_per_year", 360),
                                      seed=kwargs.get("seed"), comm=kwargs.get("comm"), devices=kwargs.get("devices"),
                                      reduce=kwargs.get("reduce"))

    def model_mc_price_chain_conditional(self, option_chain: OptionChain, params: HestonParams, nb_path: int = 100000,
                                         variable_type: VariableType = VariableType.LOG_RETURN, **kwargs):
        """model_mc_price_chain by conditional Monte Carlo (heston_mc_chain_pricer_conditional); recenter= and return_stats= are
        passed on"""
        return heston_mc_chain_pricer_conditional(
            v0=params.v0, theta=params.theta, kappa=params.kappa, rho=params.rho, volvol=params.volvol, ttms=option_chain.ttms,
            forwards=option_chain.forwards, discfactors=option_chain.discfactors, strikes_ttms=option_chain.strikes_ttms,
            optiontypes_ttms=option_chain.optiontypes_ttms, nb_path=nb_path, variable_type=variable_type,
            scheme=kwargs.get("scheme", "euler"), nb_steps_per_year=kwargs.get("nb_steps_per_year", 360), seed=kwargs.get("seed"),
            comm=kwargs.get("comm"), devices=kwargs.get("devices"), recenter=kwargs.get("recenter", True),
            return_stats=kwargs.get("return_stats", False))

    def model_mc_chain_greeks_conditional(self, option_chain: OptionChain, params: HestonParams, nb_path: int = 100000,
                                          variable_type: VariableType = VariableType.LOG_RETURN, **kwargs) -> dict:
        """model_mc_price_chain_conditional with delta, dual delta, gamma and dual gamma (heston_mc_chain_greeks_conditional);
        recenter=, return_stats=, wrt=, rel_bump= and bumps= are passed on"""
        return heston_mc_chain_greeks_conditional(
            v0=params.v0, theta=params.theta, kappa=params.kappa, rho=params.rho, volvol=params.volvol, ttms=option_chain.ttms,
            forwards=option_chain.forwards, discfactors=option_chain.discfactors, strikes_ttms=option_chain.strikes_ttms,
            optiontypes_ttms=option_chain.optiontypes_ttms, nb_path=nb_path, variable_type=variable_type,
            scheme=kwargs.get("scheme", "euler"), nb_steps_per_year=kwargs.get("nb_steps_per_year", 360), seed=kwargs.get("seed"),
            comm=kwargs.get("comm"), devices=kwargs.get("devices"), recenter=kwargs.get("recenter", True),
            return_stats=kwargs.get("return_stats", False), wrt=kwargs.get("wrt", ()), rel_bump=kwargs.get("rel_bump", 1e-3),
            bumps=kwargs.get("bumps"))

    def model_mc_price_chain_conditional_many(self, option_chain: OptionChain, params_list: Sequence[HestonParams],
                                              nb_path: int = 100000, variable_type: VariableType = VariableType.LOG_RETURN,
                                              seeds: Optional[Sequence[int]] = None, **kwargs) -> list:
        """model_mc_price_chain_conditional for several parameter sets, each with its own stream
        (heston_mc_chain_pricer_conditional_many); recenter= and return_stats= are passed on"""
        return heston_mc_chain_pricer_conditional_many(
            params_list=params_list, ttms=option_chain.ttms, forwards=option_chain.forwards, discfactors=option_chain.discfactors,
            strikes_ttms=option_chain.strikes_ttms, optiontypes_ttms=option_chain.optiontypes_ttms, nb_path=nb_path,
            variable_type=variable_type, scheme=kwargs.get("scheme", "euler"), nb_steps_per_year=kwargs.get("nb_steps_per_year", 360),
            seeds=seeds, comm=kwargs.get("comm"), devices=kwargs.get("devices"), recenter=kwargs.get("recenter", True),
            return_stats=kwargs.get("return_stats", False))

    def get_log_return_mc_pdf_conditional(self, params: HestonParams, ttm: float, x_grid: np.ndarray, nb_path: int = 100000,
                                          seed: Optional[int] = None, recenter: bool = False, return_stderr: bool = False,
                                          nb_steps_per_year: int = 360):
        """the density of the simulated log-return at x_grid from the conditional estimator's dual gamma, without a bandwidth
        (logsv_pricer.conditional_log_return_pdf): UN-NORMALISED -- the KDE routes divide by their sum, this one integrates by
        itself to n_kept_nonzero_cv / n_kept.  recenter=False: the density of the simulated x itself.  With return_stderr=True
        (pdf, its standard error).  Euler scheme."""
        def route(**chain):
            return heston_mc_chain_greeks_conditional(v0=params.v0, theta=params.theta, kappa=params.kappa, rho=params.rho,
                                                      volvol=params.volvol, nb_path=nb_path, nb_steps_per_year=nb_steps_per_year,
                                                      seed=seed, recenter=recenter, **chain)
        return conditional_log_return_pdf(route, ttm, x_grid, return_stderr)

    def get_log_return_mc_pdf_mixture(self, params: HestonParams, ttm: float, x_grid: np.ndarray, risk_premia_gammas=None,
                                      nb_path: int = 100000, seed: Optional[int] = None, return_stderr: bool = False,
                                      return_stats: bool = False, nb_steps: Optional[int] = None, scheme="euler",
                                      variable_type: VariableType = VariableType.LOG_RETURN, comm=None, devices=None):
        """the density of the simulated log-return at x_grid as the mixture of the paths' conditional Gaussians, without a bandwidth
        (logsv_pricer.mixture_log_return_pdf; LogSVPricer.get_log_return_mc_pdf_mixture states the returns): the paths of
        model_mc_price_chain_conditional at this seed, nb_steps steps per year (default 360).  risk_premia_gammas: the densities
        under exp(gamma x), [gamma][x].  Euler scheme (scheme="qe": NotImplementedError), the log-return and one GPU only."""
        who = "HestonPricer.get_log_return_mc_pdf_mixture"
        if _scheme_code(scheme) != HESTON_EULER_FLOOR:
            raise NotImplementedError(f"{who}: scheme='qe' is not covered (Euler only)")

        def step_rows(eng, rng_seed, call_id):
            nb, dt = one_expiry_grid(ttm, nb_steps or 360)
            eng.fill_state_cmc(0.0, params.v0, 0.0)
            eng.heston_chain_cmc([nb], [dt], params.theta, params.kappa, params.rho, params.volvol, rng_seed, call_id, mu_row=0,
                                 cv_row=1)
        return mixture_log_return_pdf(who, step_rows, x_grid, risk_premia_gammas, nb_path, seed, return_stderr, return_stats,
                                      variable_type, comm, devices)

    def model_mc_chain_greeks(self, option_chain: OptionChain, params: HestonParams, nb_path: int = 100000,
                              variable_type: VariableType = VariableType.LOG_RETURN, **kwargs) -> dict:
        """model_mc_price_chain with its Greeks (heston_mc_chain_greeks); wrt=, rel_bump=, bumps=, scheme= and seed= are passed on"""
        return heston_mc_chain_greeks(
            params=params, ttms=option_chain.ttms, forwards=option_chain.forwards, discfactors=option_chain.discfactors,
            strikes_ttms=option_chain.strikes_ttms, optiontypes_ttms=option_chain.optiontypes_ttms, wrt=kwargs.get("wrt"),
            rel_bump=kwargs.get("rel_bump", 1e-3), bumps=kwargs.get("bumps"), nb_path=nb_path,
            nb_steps_per_year=kwargs.get("nb_steps_per_year", 360), seed=kwargs.get("seed"), scheme=kwargs.get("scheme", "euler"),
            variable_type=variable_type, comm=kwargs.get("comm"), devices=kwargs.get("devices"))

    def model_mc_price_chain_many(self, option_chain: OptionChain, params_list: Sequence[HestonParams], nb_path: int = 100000,
                                  variable_type: VariableType = VariableType.LOG_RETURN, seeds: Optional[Sequence[int]] = None,
                                  **kwargs) -> List[Tuple[List[np.ndarray], List[np.ndarray]]]:
        """model_mc_price_chain for several parameter sets, each with its own stream (heston_mc_chain_pricer_many): job j
        returns what model_mc_price_chain(option_chain, params_list[j], seed=seeds[j], ...) returns"""
        return heston_mc_chain_pricer_many(params_list=params_list, ttms=option_chain.ttms, forwards=option_chain.forwards,
                                           discfactors=option_chain.discfactors, strikes_ttms=option_chain.strikes_ttms,
                                           optiontypes_ttms=option_chain.optiontypes_ttms, nb_path=nb_path,
                                           variable_type=variable_type, scheme=kwargs.get("scheme", "euler"),
                                           nb_steps_per_year=kwargs.get("nb_steps_per_year", 360), seeds=seeds,
                                           comm=kwargs.get("comm"), devices=kwargs.get("devices"))

    @timer
    def calibrate_model_params_to_chain(self, option_chain: OptionChain, params0: HestonParams = None,
                                        is_vega_weighted: bool = True, is_unit_ttm_vega: bool = False, **kwargs
                                        ) -> HestonParams:
        """fit (v0, theta, kappa, rho, volvol) to the chain's mid vols with the analytic pricer under the Feller
        constraint 2 kappa theta >= volvol^2 (reference :110-181; same start point, bounds and SLSQP options).
        estimator="conditional" (not in the reference): the same fit on the implied vols of the conditional
        Monte Carlo estimator on one frozen stream (heston_mc_chain_pricer_conditional_sets; nb_path=100000, nb_steps_per_year=360,
        seed=10, recenter=True), the gradient from ImpliedVolObjective.gradient in one batch per iterate."""
        p0 = np.array([0.1, 0.1, 2.0, -0.2, 1.0]) if params0 is None else \
            np.array([params0.v0, params0.theta, params0.kappa, params0.rho, params0.volvol])
        bounds = ((0.01, 2.0), (0.01, 2.0), (0.1, 30.0), (-0.99, 0.99), (0.1, 5.0))
        _, market_vols_ttms = option_chain.get_chain_data_as_xy()
        market_vols = np.concatenate(market_vols_ttms).ravel()
        weights = chain_calibration_weights(option_chain, market_vols, is_vega_weighted, is_unit_ttm_vega)

        def parse(pars: np.ndarray) -> HestonParams:
            return HestonParams(v0=pars[0], theta=pars[1], kappa=pars[2], rho=pars[3], volvol=pars[4])

        feller = {"type": "ineq", "fun": lambda pars: 2.0 * pars[2] * pars[1] - pars[4] * pars[4]}
        if kwargs.get("estimator") is not None:
            # estimator="conditional" (DESIGN.md row f15): the same fit on the conditional Monte Carlo estimator's implied vols on
            # the frozen stream (seed, call 0), an evaluation one replayed graph, the gradient's bumped vectors one batch
            if kwargs["estimator"] != "conditional":
                raise ValueError(f"estimator={kwargs['estimator']!r}: 'conditional', or no keyword for the analytic pricer")
            sets_args = dict(ttms=option_chain.ttms, forwards=option_chain.forwards, discfactors=option_chain.discfactors,
                             strikes_ttms=option_chain.strikes_ttms, optiontypes_ttms=option_chain.optiontypes_ttms,
                             nb_path=kwargs.get("nb_path", 100000), nb_steps_per_year=kwargs.get("nb_steps_per_year", 360),
                             seed=kwargs.get("seed", 10), recenter=kwargs.get("recenter", True), return_ivols=True,
                             comm=kwargs.get("comm"), devices=kwargs.get("devices"), scheme=kwargs.get("scheme", "euler"))
            check_conditional_request("calibrate_model_params_to_chain", VariableType.LOG_RETURN, sets_args["comm"], sets_args["devices"],
                                      option_chain.optiontypes_ttms)
            objective = ImpliedVolObjective(
                lambda pars: heston_mc_chain_pricer_conditional_sets([parse(pars)], **sets_args)[0][2], market_vols, weights,
                model_vols_batch=lambda pars_list: [res[2] for res in heston_mc_chain_pricer_conditional_sets(
                    [parse(p) for p in pars_list], **sets_args)], bounds=bounds)
            fit = minimize_slsqp(objective, p0, bounds, feller, disp=bool(kwargs.get("disp", True)), jac=objective.gradient)
            self.last_calibration = dict(n_eval=objective.n_eval, n_gradient_batches=objective.n_batches, objective=objective(fit))
            return parse(fit)
        objective = ImpliedVolObjective(
            lambda pars: self.compute_model_ivols_for_chain(option_chain=option_chain, params=parse(pars)),
            market_vols, weights)
        fit = minimize_slsqp(objective, p0, bounds, feller, disp=bool(kwargs.get("disp", True)))
        self.last_calibration = dict(n_eval=objective.n_eval, objective=objective(fit))
        return parse(fit)

    @timer
    def simulate_terminal_values(self, params: HestonParams, ttm: float = 1.0, nb_path: int = 100000,
                                 x0: float = 0.0, **kwargs) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """returns (x, VARIANCE, qvar) like the reference (:89-108); the x0 argument is ignored there too."""
        return self._simulate_on_engine(params, ttm, nb_path, kwargs.get("scheme", "euler"), kwargs.get("seed")).get_state()

    @staticmethod
    def _simulate_on_engine(params: HestonParams, ttm: float, nb_path: int, scheme, seed, nb_steps: Optional[int] = None):
        """the terminal state of simulate_terminal_values left on the engine it returns (the state stays on the device);
        nb_steps: a number of equal time steps in place of the daily grid's"""
        nb_steps, dt = time_grid_steps(ttm=ttm, nb_steps_per_year=360) if nb_steps is None else (int(nb_steps), float(ttm) / int(nb_steps))
        rng_seed, call_id = next_rng_call(seed)
        eng = get_engine(nb_path)
        eng.fill_state(0.0, params.v0, 0.0)           # constant initial state written on the device (reference :98-107)
        eng.heston_rng(nb_steps, dt, params.theta, params.kappa, params.rho, params.volvol, _scheme_code(scheme), rng_seed,
                       call_id, 0)
        return eng

    def model_mc_il_payoff(self, params: HestonParams, ttm: float, p1, p0, pa, pb, nb_path: int = 100000, nb_steps: Optional[int] = None,
                           seed: Optional[int] = None, notional=1000000, return_pieces: bool = False, **kwargs):
        """the Monte Carlo impermanent loss of the range [pa, pb] opened at p0, at the forward p1, under this model: the terminal
        log-returns of simulate_terminal_values stay on the device and svmc_il_payoff reduces them (include/svmc.h: recentred
        spots, value = -(notional0 notional) mean(pay), its standard error).  p1, p0, pa, pb, notional broadcast together and
        share one path set.  nb_steps: the number of time steps (default: the model's daily grid).  Returns (value, stderr), and
        with return_pieces=True a dict of the six piece means, n_kept and n_dropped.  scheme= as simulate_terminal_values.  A sharded request (comm=, devices=) raises
        NotImplementedError.  Not in the reference, which has no Monte Carlo side for this payoff."""
        from .il_pricer import il_cases, refuse_sharded_il
        refuse_sharded_il("model_mc_il_payoff", kwargs)
        il_cases(p1, p0, pa, pb, notional)                       # ValueError before any device work
        eng = self._simulate_on_engine(params, ttm, nb_path, kwargs.get("scheme", "euler"), seed, nb_steps)
        return eng.il_payoffs(p1, p0, pa, pb, notional, return_pieces=return_pieces)

    def terminal_value_histograms(self, params: HestonParams, space_grids: dict, ttm: float = 1.0, nb_path: int = 100000,
                                  **kwargs) -> dict:
        """simulate_terminal_values followed by compute_histogram_data of x, qvar / ttm and the VARIANCE (keyed
        VariableType.SIGMA: the second state vector) on the given space grids {VariableType: grid}, counted on the device --
        LogSVPricer.terminal_value_histograms for this model.  seed= / scheme= as simulate_terminal_values."""
        from .logsv_pricer import engine_state_histograms
        eng = self._simulate_on_engine(params, ttm, nb_path, kwargs.get("scheme", "euler"), kwargs.get("seed"))
        return engine_state_histograms(eng, space_grids, ttm)

    def terminal_value_kdes(self, params: HestonParams, space_grids: dict, ttm: float = 1.0, nb_path: int = 100000, **kwargs):
        """simulate_terminal_values followed by scipy.stats.gaussian_kde of x, qvar / ttm and the VARIANCE (keyed
        VariableType.SIGMA) on the given space grids, summed on the device -- LogSVPricer.terminal_value_kdes for this model.
        seed= / scheme= as simulate_terminal_values; bandwidth_factor=, return_stats= and risk_premia_gamma= as there."""
        from .logsv_pricer import engine_state_kdes, kde_keywords, refuse_sharded_kde, split_kde_results
        refuse_sharded_kde("terminal_value_kdes", kwargs)
        eng = self._simulate_on_engine(params, ttm, nb_path, kwargs.get("scheme", "euler"), kwargs.get("seed"))
        return split_kde_results(engine_state_kdes(eng, space_grids, ttm, **kde_keywords(kwargs)), kwargs.get("return_stats", False))

    def get_log_return_mc_pdf_device(self, ttm: float, params: HestonParams, x_grid: np.ndarray, nb_path: int = 100000,
                                     **kwargs) -> np.ndarray:
        """get_log_return_mc_pdf with the state left on the device and the kernel estimate summed there (seed= / scheme= as
        simulate_terminal_values; risk_premia_gamma= and return_stats= as engine_log_return_mc_pdf)"""
        from .logsv_pricer import engine_log_return_mc_pdf, refuse_sharded_kde
        refuse_sharded_kde("get_log_return_mc_pdf_device", kwargs)
        eng = self._simulate_on_engine(params, ttm, nb_path, kwargs.get("scheme", "euler"), kwargs.get("seed"))
        return engine_log_return_mc_pdf(eng, x_grid, kwargs.get("risk_premia_gamma"), kwargs.get("return_stats", False))


def compute_heston_mgf_grid(v0: float, theta: float, kappa: float, volvol: float, rho: float, ttm: float,
                            phi_grid: np.ndarray, psi_grid: np.ndarray, a_t0: np.ndarray = None, b_t0: np.ndarray = None
                            ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """closed-form Heston log-MGF over the grid, (log_mgf, a_t1, b_t1) (reference :183-214).  A missing a_t0 / b_t0
    is the zero vector: the reference's `None` branches are exactly the formulas at a_t0 = b_t0 = 0."""
    from .. import _lib
    grid = AnalyticGrid(np.asarray(phi_grid), np.asarray(psi_grid), 1)
    try:
        if a_t0 is not None:
            grid.set_a(np.asarray(a_t0, dtype=np.complex128).reshape(1, -1, 1))
        if b_t0 is not None:
            b0 = np.ascontiguousarray(b_t0, dtype=np.complex128)
            _lib.check(grid.lib.svmc_memcpy_h2d(grid.b.ptr, b0.ctypes.data, b0.nbytes, None))
            _lib.check(grid.lib.svmc_stream_synchronize(None))
        grid.heston_advance(ttm, v0, theta, kappa, volvol, rho, True)
        return grid.get_log_mgf()[0], grid.get_a().ravel(), grid._down(grid.b, (grid.n,))
    finally:
        grid.close()


def heston_chain_pricer(v0: float, theta: float, kappa: float, volvol: float, rho: float, ttms: np.ndarray,
                        forwards: np.ndarray, strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray],
                        discfactors: np.ndarray, variable_type: VariableType = VariableType.LOG_RETURN,
                        vol_scaler: float = None) -> List[np.ndarray]:
    """analytic Heston chain prices (reference :217-282): LOG_RETURN on the 1000-point phi grid, Q_VAR (calls on the
    annualised quadratic variance) on the 40 000-point psi grid"""
    vt = int(getattr(variable_type, "value", variable_type))
    if vt not in (1, 2):
        raise NotImplementedError(f"variable_type={variable_type}")
    if vol_scaler is None:
        vol_scaler = np.minimum(0.3, np.sqrt(v0 * ttms[0]))
    phi_grid, psi_grid, _ = mgfp.get_transform_var_grid(variable_type=variable_type, vol_scaler=vol_scaler)
    grid = AnalyticGrid.acquire(phi_grid, psi_grid, 1)
    try:
        inversion = "vanilla" if vt == 1 else "qvar"
        sums = chain_sums(grid, ttms, forwards, strikes_ttms,      # have_t0 on zeroed a, b == the reference's None branch
                          lambda i, dt: grid.heston_advance(dt, v0, theta, kappa, volvol, rho, True), inversion)
        return chain_prices_from_sums(sums, inversion, ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms)[0]
    finally:
        grid.release()


def heston_mc_chain_pricer_many(params_list: Sequence[HestonParams], ttms: np.ndarray, forwards: np.ndarray,
                                discfactors: np.ndarray, strikes_ttms: Sequence[np.ndarray],
                                optiontypes_ttms: Sequence[np.ndarray], nb_path: int = 100000,
                                variable_type: VariableType = VariableType.LOG_RETURN, scheme="euler",
                                nb_steps_per_year: int = 360, seeds: Optional[Sequence[int]] = None, comm=None, devices=None
                                ) -> List[Tuple[List[np.ndarray], List[np.ndarray]]]:
    """heston_mc_chain_pricer for several independent jobs of ONE chain, as logsv_mc_chain_pricer_many: job j has the
    parameters params_list[j] and the stream seeds[j] (or the next call id, in list order, with seeds=None), and returns
    what heston_mc_chain_pricer(..., seed=seeds[j]) returns, bit for bit.  On one GPU up to MANY_MAX_JOBS jobs per
    svmc_heston_chain_price_many call; with comm.world > 1, devices= or more than 16 expiries a loop of single calls."""
    params_list = check_many_args(params_list, seeds)
    code = _scheme_code(scheme)
    if not params_list:
        return []
    comm = comm or svdist.get_default_comm()
    if devices is not None or comm.world > 1 or len(ttms) > 16 or not (FUSED_MC_CHAIN_DRIVER and WHOLE_CHAIN_STEPPING):
        # a loop of single calls (a sharded batch is out of scope): each takes its own stream, unseeded ones in list order
        return [heston_mc_chain_pricer(ttms=ttms, forwards=forwards, discfactors=discfactors, strikes_ttms=strikes_ttms,
                                       optiontypes_ttms=optiontypes_ttms, v0=p.v0, theta=p.theta, kappa=p.kappa, rho=p.rho,
                                       volvol=p.volvol, nb_path=nb_path, variable_type=variable_type, scheme=scheme,
                                       nb_steps_per_year=nb_steps_per_year, seed=None if seeds is None else seeds[j],
                                       comm=comm, devices=devices)
                for j, p in enumerate(params_list)]
    streams = many_job_streams(len(params_list), seeds)
    rows = np.array([(p.v0, p.theta, p.kappa, p.rho, p.volvol) for p in params_list], dtype=np.float64)
    ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, [option_type_codes(t) for t in optiontypes_ttms])
    eng = get_engine(nb_path)
    out = []
    for _, part, job_seeds, ids in many_job_chunks(streams, rows):
        out += eng.price_chain_many_fused(ch, "heston", part, job_seeds, ids, code, nb_steps_per_year, variable_type_code(variable_type))
    return many_jobs_shaped(out, strikes_ttms)


def heston_mc_chain_greeks(params: HestonParams, ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                           strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray],
                           wrt: Optional[Sequence[str]] = None, rel_bump: float = 1e-3, bumps: Optional[dict] = None,
                           nb_path: int = 100000, nb_steps_per_year: int = 360, seed: Optional[int] = None, scheme="euler",
                           variable_type: VariableType = VariableType.LOG_RETURN, comm=None, devices=None) -> dict:
    """heston_mc_chain_pricer with its Greeks (include/svmc.h; see logsv_mc_chain_greeks): wrt defaults to v0 theta
    kappa rho volvol, either scheme.  Returns the same dict of chain-shaped lists; price / stderr are bit-equal to
    heston_mc_chain_pricer at the same seed and scheme.  A bump that takes |rho| to 1 or beyond, or a variance or the vol-of-vol
    below zero, raises ValueError naming the parameter.  Not in the reference API."""
    codes = check_greeks_request("heston_mc_chain_greeks", variable_type, comm, devices, optiontypes_ttms)
    code = _scheme_code(scheme)
    names, h = greeks_bumps("heston", {k: getattr(params, k) for k in HESTON_GREEK_PARAMS}, wrt, rel_bump, bumps)
    rows = greeks_job_table("heston", [getattr(params, k) for k in HESTON_GREEK_PARAMS], names, h)
    rng_seed, call_id = next_rng_call(seed)
    ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, codes)
    prices, stderrs, base, sens = get_engine(nb_path).price_chain_greeks_fused(ch, "heston", rows, h, code, nb_steps_per_year, rng_seed,
                                                                               call_id)
    return greeks_shaped(prices, stderrs, base, sens, names, ch["slices"], strikes_ttms)


def simulate_heston_x_vol_terminal(ttm: float, x0: np.ndarray, var0: np.ndarray, qvar0: np.ndarray, theta: float,
                                   kappa: float, rho: float, volvol: float, nb_path: int = 100000,
                                   nb_steps_per_year: int = 360, scheme="euler", seed: Optional[int] = None,
                                   W0: Optional[np.ndarray] = None, W1: Optional[np.ndarray] = None,
                                   dt: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """terminal (x, variance, qvar) (reference :334-381).  W0/W1/dt are an extension: supplied UNSCALED normals
    for the Euler scheme, the fixed-randoms route the reference offers only for LogSV."""
    x0, var0, qvar0 = _broadcast_state(x0, var0, qvar0, nb_path)
    code = _scheme_code(scheme)
    eng = get_engine(nb_path)
    eng.set_state(x0, var0, qvar0)
    if W0 is None and W1 is None:
        nb_steps, dt = time_grid_steps(ttm=ttm, nb_steps_per_year=nb_steps_per_year)
        rng_seed, call_id = next_rng_call(seed)
        eng.heston_rng(nb_steps, dt, theta, kappa, rho, volvol, code, rng_seed, call_id, 0)
    else:
        if code != HESTON_EULER_FLOOR:
            raise ValueError("supplied W0/W1 drive the Euler scheme only")
        W0, W1 = np.asarray(W0), np.asarray(W1)
        if W0.shape != W1.shape or W0.ndim != 2 or W0.shape[1] != nb_path or dt is None:
            raise ValueError("W0 and W1 must both have shape [nb_steps, nb_path] and come with dt")
        w0, w1 = eng.upload_randoms((W0, W1))
        eng.heston_w(W0.shape[0], dt, theta, kappa, rho, volvol, w0, w1)
    return eng.get_state()


def heston_mc_chain_pricer_conditional(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                                       strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray], v0: float,
                                       theta: float, kappa: float, rho: float, volvol: float, nb_path: int = 100000,
                                       variable_type: VariableType = VariableType.LOG_RETURN, scheme="euler",
                                       nb_steps_per_year: int = 360, seed: Optional[int] = None, comm=None, devices=None,
                                       reduce: Optional[str] = None, recenter: bool = True, return_stats: bool = False):
    """heston_mc_chain_pricer by CONDITIONAL Monte Carlo (include/svmc.h; see
    logsv_mc_chain_pricer_conditional): the reference's Euler step with its floor, the variance driven by one normal per step, a
    Black-76 price per path.  Same signature and (prices, stderrs) lists; return_stats=True adds the per-expiry dicts of
    engine.CMC_STATS_FIELDS.  scheme="qe" raises NotImplementedError (the QE step's return is not Gaussian given the variance
    path's driver as written here: a separate step); 'C' / 'P', LOG_RETURN and one GPU only.  Not in the reference API."""
    codes = check_conditional_request("heston_mc_chain_pricer_conditional", variable_type, comm, devices, optiontypes_ttms)
    if _scheme_code(scheme) != HESTON_EULER_FLOOR:
        raise NotImplementedError("heston_mc_chain_pricer_conditional: scheme='qe' is not covered (Euler only)")
    rng_seed, call_id = next_rng_call(seed)
    ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, codes)
    prices, stderrs, stats = get_engine(nb_path).price_heston_chain_cmc_fused(ch, v0, theta, kappa, rho, volvol, nb_steps_per_year,
                                                                               recenter, rng_seed, call_id)
    out = (chain_shaped(prices, strikes_ttms), chain_shaped(stderrs, strikes_ttms))
    return out + (stats,) if return_stats else out


def heston_mc_chain_greeks_conditional(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                                       strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray], v0: float,
                                       theta: float, kappa: float, rho: float, volvol: float, nb_path: int = 100000,
                                       variable_type: VariableType = VariableType.LOG_RETURN, scheme="euler",
                                       nb_steps_per_year: int = 360, seed: Optional[int] = None, comm=None, devices=None,
                                       reduce: Optional[str] = None, recenter: bool = True, return_stats: bool = False,
                                       wrt: Optional[Sequence[str]] = (), rel_bump: float = 1e-3, bumps: Optional[dict] = None) -> dict:
    """heston_mc_chain_pricer_conditional with delta, dual delta, gamma and dual gamma and their standard errors (include/svmc.h,
    DESIGN.md row f13; see logsv_mc_chain_greeks_conditional for the returned dict).  Same signature and refusals, scheme="qe"
    among them.  wrt (row f14; default (): nothing changes): names among v0 theta kappa rho volvol, or None / "all" -- the
    dict gains sens[name], sens_stderr[name], n_pairs[name] as logsv_mc_chain_greeks_conditional's does.  Not in the reference
    API."""
    who = "heston_mc_chain_greeks_conditional"
    codes = check_conditional_request(who, variable_type, comm, devices, optiontypes_ttms)
    if _scheme_code(scheme) != HESTON_EULER_FLOOR:
        raise NotImplementedError("heston_mc_chain_greeks_conditional: scheme='qe' is not covered (Euler only)")
    if not (wrt is None or isinstance(wrt, str) or len(wrt) > 0):
        rng_seed, call_id = next_rng_call(seed)
        ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, codes)
        fields, stats = get_engine(nb_path).price_heston_chain_cmc_greeks_fused(ch, v0, theta, kappa, rho, volvol, nb_steps_per_year,
                                                                                recenter, rng_seed, call_id)
        return conditional_greeks_shaped(fields, stats, strikes_ttms, return_stats)
    values = dict(v0=v0, theta=theta, kappa=kappa, rho=rho, volvol=volvol)
    names, h = greeks_bumps("heston", values, None if isinstance(wrt, str) and wrt == "all" else wrt, rel_bump, bumps)
    check_conditional_sens_expiries(who, ttms)
    rows = greeks_job_table("heston", [values[k] for k in HESTON_GREEK_PARAMS], names, h)
    rng_seed, call_id = next_rng_call(seed)
    ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, codes)
    fields, stats, sens = get_engine(nb_path).price_chain_cmc_sens_fused(ch, "heston", rows, h, 0, nb_steps_per_year, recenter, rng_seed,
                                                                         call_id)
    return conditional_sens_shaped(conditional_greeks_shaped(fields, stats, strikes_ttms, return_stats), sens, names, ch["slices"],
                                   strikes_ttms)


def heston_mc_chain_pricer_conditional_many(params_list: Sequence[HestonParams], ttms: np.ndarray, forwards: np.ndarray,
                                            discfactors: np.ndarray, strikes_ttms: Sequence[np.ndarray],
                                            optiontypes_ttms: Sequence[np.ndarray], nb_path: int = 100000,
                                            variable_type: VariableType = VariableType.LOG_RETURN, scheme="euler",
                                            nb_steps_per_year: int = 360, seeds: Optional[Sequence[int]] = None, comm=None,
                                            devices=None, recenter: bool = True, return_stats: bool = False) -> list:
    """heston_mc_chain_pricer_conditional for several independent jobs of ONE chain (see
    logsv_mc_chain_pricer_conditional_many): job j is bit-equal to heston_mc_chain_pricer_conditional with (params_list[j],
    seeds[j]); up to MANY_MAX_JOBS jobs per stepping launch, more than 16 expiries as a loop of single calls.  Not in the reference
    API."""
    codes = check_conditional_request("heston_mc_chain_pricer_conditional_many", variable_type, comm, devices, optiontypes_ttms)
    if _scheme_code(scheme) != HESTON_EULER_FLOOR:
        raise NotImplementedError("heston_mc_chain_pricer_conditional_many: scheme='qe' is not covered (Euler only)")
    params_list = check_many_args(params_list, seeds)
    if not params_list:
        return []
    if len(ttms) > 16:
        return [heston_mc_chain_pricer_conditional(
            ttms=ttms, forwards=forwards, discfactors=discfactors, strikes_ttms=strikes_ttms, optiontypes_ttms=optiontypes_ttms,
            v0=p.v0, theta=p.theta, kappa=p.kappa, rho=p.rho, volvol=p.volvol, nb_path=nb_path, variable_type=variable_type,
            nb_steps_per_year=nb_steps_per_year, seed=None if seeds is None else seeds[j], recenter=recenter, return_stats=return_stats)
            for j, p in enumerate(params_list)]
    streams = many_job_streams(len(params_list), seeds)
    rows = np.array([[p.v0, p.theta, p.kappa, p.rho, p.volvol] for p in params_list], dtype=np.float64)
    ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, codes)
    eng = get_engine(nb_path)
    out = []
    for _, part, job_seeds, ids in many_job_chunks(streams, rows):
        out += eng.price_chain_cmc_many_fused(ch, "heston", part, job_seeds, ids, 0, nb_steps_per_year, recenter)
    return conditional_many_shaped(out, strikes_ttms, return_stats)


def heston_mc_chain_pricer_conditional_sets(params_list: Sequence[HestonParams], ttms: np.ndarray, forwards: np.ndarray,
                                            discfactors: np.ndarray, strikes_ttms: Sequence[np.ndarray],
                                            optiontypes_ttms: Sequence[np.ndarray], nb_path: int = 100000,
                                            nb_steps_per_year: int = 360, variable_type: VariableType = VariableType.LOG_RETURN,
                                            seed: Optional[int] = None, recenter: bool = True, return_ivols: bool = False,
                                            return_stats: bool = False, comm=None, devices=None, scheme="euler") -> list:
    """heston_mc_chain_pricer_conditional for several parameter sets of ONE chain on ONE random stream (see
    logsv_mc_chain_pricer_conditional_sets): set q is bit-equal to heston_mc_chain_pricer_conditional(params_list[q]) on (seed, call
    0) -- seed=None: the process seed and ONE next call id --, return_ivols=True adds the Black-76 implied vols of its prices; up to
    CMC_SETS_MAX sets are one replayed graph (svmc_heston_chain_price_cmc_sets).  Not in the reference API."""
    who = "heston_mc_chain_pricer_conditional_sets"
    codes = check_conditional_request(who, variable_type, comm, devices, optiontypes_ttms)
    if _scheme_code(scheme) != HESTON_EULER_FLOOR:
        raise NotImplementedError(f"{who}: scheme='qe' is not covered (Euler only)")
    params_list = list(params_list)
    rows = np.array([[p.v0, p.theta, p.kappa, p.rho, p.volvol] for p in params_list], dtype=np.float64).reshape(len(params_list), 5)
    chain = (ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms)

    def single(q: int, rng_seed: int, call_id: int):
        p = params_list[q]
        ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, codes)
        return get_engine(nb_path).price_heston_chain_cmc_fused(ch, p.v0, p.theta, p.kappa, p.rho, p.volvol, nb_steps_per_year, recenter,
                                                                rng_seed, call_id)
    return conditional_sets_on_engine("heston", rows, single, chain, codes, True, nb_path, nb_steps_per_year, seed, recenter,
                                      return_ivols, return_stats)


def heston_mc_chain_pricer(ttms: np.ndarray, forwards: np.ndarray, discfactors: np.ndarray,
                           strikes_ttms: Sequence[np.ndarray], optiontypes_ttms: Sequence[np.ndarray], v0: float,
                           theta: float, kappa: float, rho: float, volvol: float, nb_path: int = 100000,
                           variable_type: VariableType = VariableType.LOG_RETURN, scheme="euler",
                           nb_steps_per_year: int = 360, seed: Optional[int] = None, comm=None, devices=None,
                           reduce: Optional[str] = None) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """chain MC (reference :285-331): state carried slice to slice, 360 steps/yr unless overridden.
    devices=N | [ids]: the paths sharded over that many GPUs of this process (stochvolmodels_amd.multi), as for
    logsv_mc_chain_pricer."""
    vt_code = variable_type_code(variable_type)
    code = _scheme_code(scheme)
    if devices is not None:
        if comm is not None:
            raise ValueError("devices= (one process, several GPUs) and comm= (one process per GPU) are exclusive")
        from ..multi import get_multi_session
        rng_seed, call_id = next_rng_call(seed)
        ms = get_multi_session(devices, nb_path, len(ttms), sum(int(np.asarray(k).size) for k in strikes_ttms), reduce=reduce)
        return ms.price_heston_chain(ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms, v0, theta, kappa, rho, volvol,
                                     code, nb_steps_per_year, vt_code, rng_seed, call_id)
    comm = comm or svdist.get_default_comm()
    offset, n_local = svdist.shard_range(nb_path, comm.rank, comm.world)
    eng = get_engine(n_local, path_offset=offset)
    rng_seed, call_id = next_rng_call(seed)
    if FUSED_MC_CHAIN_DRIVER and WHOLE_CHAIN_STEPPING and comm.world == 1 and hasattr(eng, "price_heston_chain_fused"):
        # one GPU: ONE call of the fused C driver on the engine's own state (see logsv_mc_chain_pricer)
        ch = marshalled_chain(ttms, forwards, discfactors, strikes_ttms, [option_type_codes(t) for t in optiontypes_ttms])
        prices, stderrs = eng.price_heston_chain_fused(ch, v0, theta, kappa, rho, volvol, code, nb_steps_per_year, vt_code,
                                                       rng_seed, call_id)
        return chain_shaped(prices, strikes_ttms), chain_shaped(stderrs, strikes_ttms)
    grids = list(zip(*chain_step_grid(ttms, nb_steps_per_year)))
    step0 = np.concatenate([[0], np.cumsum([g[0] for g in grids])])
    start = (0.0, v0, 0.0)     # every path's start state (reference :303-305) goes to the first stepping launch as constants

    def advance(i: int, forward: float, snap_row: int, qvar_row, spot_ptr: int) -> None:
        nb, dt = grids[i]
        eng.heston_slice_rng(nb, dt, theta, kappa, rho, volvol, code, rng_seed, call_id, int(step0[i]), forward,
                             snap_row, qvar_row, spot_ptr, start=start if i == 0 else None)

    def advance_chain(need_qvar: bool, spot_ptr: int) -> None:
        eng.heston_chain_rng([g[0] for g in grids], [g[1] for g in grids], forwards, theta, kappa, rho, volvol, code,
                             rng_seed, call_id, 0, need_qvar, spot_ptr, start=start)

    return price_chain_on_engine(eng, comm, nb_path, ttms, forwards, discfactors, strikes_ttms, optiontypes_ttms,
                                 variable_type, advance,
                                 advance_chain=advance_chain if (WHOLE_CHAIN_STEPPING and len(grids) > 1) else None)
