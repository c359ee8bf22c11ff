"""
Transform grids, quadrature weights and the Fourier slice pricer (mirror of the reference's utils/mgf_pricer.py:
get_phi_grid :11-34, get_psi_grid :37-47, get_theta_grid :50-58, get_transform_var_grid :61-94,
compute_integration_weights :97-155, vanilla_slice_pricer_with_mgf_grid :174-221, digital_slice_pricer_with_mgf_grid :224-269,
slice_pricer_with_mgf_grid_with_gamma :273-321, pdf_with_mgf_grid :361-384).  Grid construction is host NumPy; the sums of the
slice pricers run in libsvmc's mgf_vanilla_slice_kernel, mgf_gamma_slice_kernel, mgf_digital_slice_kernel and
mgf_pdf_slice_kernel.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from ..analytic import (AnalyticGrid, digital_prices_from_sums, digital_slice_sums, gamma_slice_prices, pdf_slices,
                        vanilla_prices_from_capped)
from .config import VariableType


def get_phi_grid(is_spot_measure: bool = True, max_phi: int = 1000, vol_scaler: float = 0.28,
                 real_phi: float = None) -> np.ndarray:
    p = np.linspace(0, 5.6 / vol_scaler, max_phi)
    real_p = (-0.5 if is_spot_measure else 0.5) if real_phi is None else real_phi
    return real_p + 1j * p


def get_psi_grid() -> np.ndarray:
    return -0.5 + 1j * np.linspace(0, 4000, 40000)


def get_theta_grid() -> np.ndarray:
    return 0.0 + 1j * np.linspace(0, 600, 5000)


def get_transform_var_grid(variable_type: VariableType = VariableType.LOG_RETURN, is_spot_measure: bool = True,
                           max_phi: int = 1000, vol_scaler: float = 0.28, real_phi: float = None
                           ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    code = int(getattr(variable_type, "value", variable_type))
    if code == 1:
        phi_grid = get_phi_grid(is_spot_measure=is_spot_measure, max_phi=max_phi, vol_scaler=vol_scaler, real_phi=real_phi)
        psi_grid = np.zeros_like(phi_grid, dtype=np.complex128)
        theta_grid = np.zeros_like(phi_grid, dtype=np.complex128)
    elif code == 2:
        psi_grid = get_psi_grid()
        phi_grid = (np.zeros_like if is_spot_measure else np.ones_like)(psi_grid, dtype=np.complex128)
        theta_grid = np.zeros_like(phi_grid, dtype=np.complex128)
    elif code == 3:
        theta_grid = get_theta_grid()
        phi_grid = np.zeros_like(theta_grid, dtype=np.complex128)
        psi_grid = np.zeros_like(theta_grid, dtype=np.complex128)
    else:
        raise NotImplementedError
    return phi_grid, psi_grid, theta_grid


def compute_integration_weights(var_grid: np.ndarray, is_simpson: bool = True) -> np.ndarray:
    """validated composite Simpson / trapezoid weights on Im(var_grid) (reference :97-155)"""
    p = np.imag(var_grid)
    if len(p) < (3 if is_simpson else 2):
        raise ValueError("integration grid is too short for the selected rule")
    if not np.all(np.isfinite(p)):
        raise ValueError("integration grid must contain only finite values")
    steps = p[1:] - p[:-1]
    if np.any(steps <= 0.0):
        raise ValueError("integration grid must be strictly increasing")
    if np.any(np.abs(steps - steps[0]) > 1.0e-12 * max(1.0, np.abs(steps[0]))):
        raise ValueError("integration grid must be uniformly spaced")
    if is_simpson:
        if len(p) % 2 == 0:
            raise ValueError("Simpson integration requires an odd number of grid points")
        dp = 2.0 * np.ones(len(p))
        dp[0] = dp[-1] = 1.0
        dp[1::2] = 4.0
        return ((p[1] - p[0]) / 3.0) * dp
    dp = steps[0] * np.ones(len(p))
    dp[0] = dp[-1] = 0.5 * steps[0]
    return dp


def vanilla_slice_pricer_with_mgf_grid(log_mgf_grid: np.ndarray, phi_grid: np.ndarray, forward: float,
                                       strikes: np.ndarray, optiontypes: np.ndarray, discfactor: float = 1.0,
                                       is_spot_measure: bool = True, is_simpson: bool = True) -> np.ndarray:
    """vanilla prices of one slice from log E on the phi grid (reference :174-221), grids with |Re phi| = 1/2."""
    if not is_simpson or not np.all(np.abs(np.real(phi_grid)) == 0.5):
        raise NotImplementedError("the GPU slice pricer covers the Simpson rule on phi = +/-0.5 + i p grids")
    grid = AnalyticGrid(phi_grid, np.zeros_like(phi_grid), 1)
    try:
        lm = grid._up(np.ascontiguousarray(log_mgf_grid, dtype=np.complex128))
        capped = grid.capped_sums(forward, np.asarray(strikes, dtype=np.float64), log_mgf_ptr=lm.ptr)[0]
        lm.free()
    finally:
        grid.close()
    return vanilla_prices_from_capped(capped, forward, strikes, optiontypes, discfactor, is_spot_measure)


def gamma_shortcut(phi_grid: np.ndarray, risk_premia_gamma: float) -> bool:
    """the reference's branch of the risk-premia payoff weight (:296): the real shortcut where every
    |Re phi - (0.5 + gamma)| < 1e-10 -- on the risk grid Re phi = -0.5 - gamma, i.e. only at gamma = -0.5"""
    return bool(np.all(np.abs(np.real(phi_grid) - (0.5 + risk_premia_gamma)) < 1e-10))


def gamma_type_codes(optiontypes) -> np.ndarray:
    """'C' -> 0, 'P' -> 1; any other type raises as the reference does (:318-319)"""
    codes = np.empty(len(optiontypes), dtype=np.int32)
    for i, t in enumerate(optiontypes):
        t = str(t)
        if t not in ("C", "P"):
            raise ValueError("not implemented")
        codes[i] = 0 if t == "C" else 1
    return codes


def slice_pricer_with_mgf_grid_with_gamma(log_mgf_grid: np.ndarray, phi_grid: np.ndarray, risk_premia_gamma: float, ttm: float,
                                          forward: float, normalizer: float, gamma_forward: float, strikes: np.ndarray,
                                          optiontypes: np.ndarray, discfactor: float = 1.0, is_spot_measure: bool = True,
                                          is_simpson: bool = True) -> np.ndarray:
    """vanilla prices of one slice under the risk-premia kernel from log E on the phi grid (reference :273-321): legacy Simpson
    weights, the payoff weight (dp / pi) / (p^2 + 1/4) where gamma_shortcut holds and -(dp / pi) / ((phi + gamma + 1)(phi +
    gamma)) otherwise, cap = nansum Re[w exp(-x phi + log E)]; 'C' -> gamma_forward - normalizer K^(1+gamma) cap, 'P' -> K -
    normalizer K^(1+gamma) cap.  As in the reference, the prices are undiscounted (discfactor and ttm are unused), and
    is_spot_measure=False or a type other than 'C' / 'P' raises ValueError."""
    if not is_simpson:
        raise NotImplementedError("the GPU slice pricer covers the Simpson rule")
    strikes = np.asarray(strikes, dtype=np.float64)
    if strikes.size and not is_spot_measure:
        raise ValueError("not implemented")
    codes = gamma_type_codes(optiontypes)
    phi_grid = np.asarray(phi_grid, dtype=np.complex128).ravel()
    prices = gamma_slice_prices(phi_grid, np.asarray(log_mgf_grid, dtype=np.complex128).ravel(), float(risk_premia_gamma),
                                gamma_shortcut(phi_grid, risk_premia_gamma), float(normalizer), float(gamma_forward),
                                float(forward), strikes.ravel(), codes)
    return prices.reshape(strikes.shape)


def digital_slice_pricer_with_mgf_grid(log_mgf_grid: np.ndarray, phi_grid: np.ndarray, forward: float, strikes: np.ndarray,
                                       optiontypes: np.ndarray, discfactor: float = 1.0, is_simpson: bool = True) -> np.ndarray:
    """digital option prices of one slice from log E on the phi grid (reference :224-269), any model's log-MGF: the payoff
    weight is -(dp / pi) / phi where every Re phi < 0 (the sums are digital calls) and +(dp / pi) / phi otherwise (puts), the
    other type is the complement 1 - sum, a type other than 'C' / 'P' raises ValueError."""
    phi_grid = np.asarray(phi_grid, dtype=np.complex128).ravel()
    strikes = np.asarray(strikes, dtype=np.float64)
    for t in optiontypes:
        if str(t) not in ("C", "P"):
            raise ValueError("not implemented")
    calls = bool(np.all(np.real(phi_grid) < 0.0))                                               # :242
    sums = digital_slice_sums(phi_grid[None, :], np.asarray(log_mgf_grid, dtype=np.complex128).ravel()[None, :], float(forward),
                              strikes.ravel(), calls, is_simpson)[0]
    return digital_prices_from_sums(sums, list(np.asarray(optiontypes).ravel()), float(discfactor), calls).reshape(strikes.shape)


def pdf_with_mgf_grid(log_mgf_grid: np.ndarray, transform_var_grid: np.ndarray, space_grid: np.ndarray, shift: float = 0.0,
                      scale: float = 1.0, is_simpson: bool = True) -> np.ndarray:
    """bin masses dx * density of the variable whose log-MGF is given on its transform grid, at z = (space_grid - shift) / scale
    (reference :361-384; dx = space_grid[1] - space_grid[0]), any model's log-MGF"""
    space = np.asarray(space_grid, dtype=np.float64)
    out = pdf_slices(np.asarray(transform_var_grid, dtype=np.complex128).ravel()[None, :],
                     np.asarray(log_mgf_grid, dtype=np.complex128).ravel()[None, :], space.ravel()[None, :], [float(shift)],
                     [float(scale)], is_simpson)[0]
    return out.reshape(space.shape)
