"""
Impermanent loss (IL) of a concentrated-liquidity range [pa, pb] on the GPU: the Fourier pricers of the reference's
papers/il_hedging/run_logsv_for_il_payoff.py (logsv_il_pricer :20-91, logsv_il_pricer_vector :94,
square_root_payoff_pricer_with_mgf_grid :97-121) under their names, and a Monte Carlo side the reference leaves to its users
(compute_mc_il_payoff, HipEngine.il_payoffs, model_mc_il_payoff of the three pricers).  DESIGN.md row f10.

Per terminal spot S the payoff is the hold-minus-pool value of a unit-liquidity position opened at p0,

    pay(S) = -2 sqrt(S) 1{pa<=S<=pb} + sqrt(p0) (S/p0 + 1) + (pa-S)^+/sqrt(pa) - (S-pb)^+/sqrt(pb) - 2 sqrt(pa) 1{S<pa} - 2 sqrt(pb) 1{S>pb}

(il_payoff below), and the price is -(notional0 notional) E[pay], notional0 = 1 / (2 sqrt(p0) - p0/sqrt(pb) - sqrt(pa)).

Fourier side: the reference re-solves the 1 001 coefficient ODEs for every forward of a profile (np.vectorize); the log-MGF does
not depend on the forward, so here a whole profile is ONE svmc_logsv_mgf_grid launch and ONE svmc_mgf_il_slice_batch launch, the
log-MGF staying on the device between them.  The five sums come back and are composed on the host in the reference's order.
The transform grid is the reference's: get_transform_var_grid(vol_scaler, real_phi=-0.4, max_phi=1001), with its finite-grid
offset at low volatility and short maturities (README, known limits; vol_scaler= is the way out).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from .. import _lib
from ..analytic import AnalyticGrid, _given_log_mgf_call
from ..utils import mgf_pricer as mgfp
from .logsv.affine_expansion import ExpansionOrder, _order_code, note_integrator_flags
from .logsv.logsv_params import LogSvParams

IL_REAL_PHI, IL_MAX_PHI = -0.4, 1001                         # the contour the square-root piece shares with the vanillas and digitals
IL_SLICE_SUMS, IL_CASE_DOUBLES, IL_OUT_DOUBLES, IL_MAX_CASES = 5, 5, 10, 65536           # SVMC_IL_* of include/svmc.h
IL_PIECES = ("square_root", "linear", "put", "call", "digital_put", "digital_call")
IL_MC_FIELDS = ("value", "stderr") + IL_PIECES + ("n_kept", "n_dropped")


# ---- host side, no library ---------------------------------------------------------------------------------------------------
def il_payoff(spot, p0, pa, pb):
    """pay(S) of the module docstring (NumPy, broadcasting): the hold-minus-pool value per unit of liquidity"""
    spot, p0, pa, pb = (np.asarray(a, dtype=np.float64) for a in (spot, p0, pa, pb))
    inside = (spot >= pa) & (spot <= pb)                        # at an end the square root equals the digital's term
    with np.errstate(invalid="ignore"):
        root = np.where(inside, np.sqrt(np.where(inside, spot, 1.0)), 0.0)
    return (-2.0 * root + np.sqrt(p0) * (spot / p0 + 1.0) + np.maximum(pa - spot, 0.0) / np.sqrt(pa)
            - np.maximum(spot - pb, 0.0) / np.sqrt(pb) - 2.0 * np.sqrt(pa) * (spot < pa) - 2.0 * np.sqrt(pb) * (spot > pb))


def il_notional0(p0, pa, pb):
    """1 / (2 sqrt(p0) - p0 / sqrt(pb) - sqrt(pa)) (reference :89)"""
    p0, pa, pb = (np.asarray(a, dtype=np.float64) for a in (p0, pa, pb))
    return 1.0 / (2.0 * np.sqrt(p0) - p0 / np.sqrt(pb) - np.sqrt(pa))


def il_cases(p1, p0, pa, pb, notional=1000000) -> Tuple[np.ndarray, tuple]:
    """the cases of a call: p1, p0, pa, pb and notional broadcast together -> ([n_cases][5] float64, the broadcast shape).
    Raises ValueError unless every input is positive and finite, 0 < pa < pb and pa < p0 < pb -- before any device work."""
    try:
        arrs = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (p1, p0, pa, pb, notional)))
    except ValueError as exc:
        raise ValueError(f"impermanent loss: p1, p0, pa, pb and notional do not broadcast together ({exc})") from None
    shape = arrs[0].shape
    cases = np.ascontiguousarray(np.stack([a.ravel() for a in arrs], axis=1))
    for name, col in zip(("p1", "p0", "pa", "pb", "notional"), cases.T):
        if not np.all(np.isfinite(col) & (col > 0.0)):
            raise ValueError(f"impermanent loss: {name} must be positive and finite")
    if not np.all(cases[:, 2] < cases[:, 3]):
        raise ValueError("impermanent loss: the range needs 0 < pa < pb")
    if not np.all((cases[:, 2] < cases[:, 1]) & (cases[:, 1] < cases[:, 3])):
        raise ValueError("impermanent loss: the range must hold the opening price, pa < p0 < pb")
    if cases.shape[0] > IL_MAX_CASES:
        raise ValueError(f"impermanent loss: at most {IL_MAX_CASES} cases a call")
    return cases, shape


def il_reference_sums(raw_sums: np.ndarray, is_all_calls: bool) -> np.ndarray:
    """svmc_mgf_il_slice_batch's sums [..., 5] as the reference's own five nansums: the digital sums are stored on their put
    side (+(dp / pi) / phi); where every Re phi < 0 the reference sums digital calls (-(dp / pi) / phi, :244): the sign"""
    out = np.array(raw_sums, dtype=np.float64, copy=True)
    if is_all_calls:
        out[..., 3:5] = -out[..., 3:5]
    return out


def il_compose(sums: np.ndarray, p1, p0, pa, pb, notional, is_all_calls: bool = True, discfactor: float = 1.0):
    """the reference's five nansums [..., 5] = (square root, capped at pa, capped at pb, digital at pa, digital at pb) -> (IL
    value, the six pieces [..., 6] in IL_PIECES' order), every step in the reference's order (:56-91, utils/mgf_pricer.py:208-
    210, :254-267): the vanilla put at pa and call at pb, the digital put at pa and call at pb (the complement 1 - sum for the
    type the contour does not sum), then payoff and -(notional0 notional) payoff"""
    sums = np.asarray(sums, dtype=np.float64)
    p1, p0, pa, pb, notional = (np.asarray(a, dtype=np.float64) for a in (p1, p0, pa, pb, notional))
    square_root = discfactor * sums[..., 0]
    bsm_put = discfactor * (pa - pa * sums[..., 1])
    bsm_call = discfactor * (p1 - pb * sums[..., 2])
    digital_put = discfactor * ((1.0 - sums[..., 3]) if is_all_calls else sums[..., 3])
    digital_call = discfactor * (sums[..., 4] if is_all_calls else (1.0 - sums[..., 4]))
    sp0, spa, spb = np.sqrt(p0), np.sqrt(pa), np.sqrt(pb)
    linear = sp0 * (p1 / p0 + 1.0)
    payoff = -2.0 * square_root + linear + \
        (1.0 / spa) * bsm_put - (1.0 / spb) * bsm_call \
        - 2.0 * spa * digital_put - 2.0 * spb * digital_call
    notional0 = 1.0 / (2.0 * sp0 - p0 / spb - spa)
    value = -(notional0 * notional) * payoff
    pieces = np.stack(np.broadcast_arrays(square_root, linear, bsm_put, bsm_call, digital_put, digital_call), axis=-1)
    return value, pieces


def _shaped(flat: np.ndarray, shape: tuple):
    """results of the cases in the broadcast shape of the inputs; a scalar for scalar input"""
    out = np.asarray(flat).reshape(shape + np.shape(flat)[1:])
    return out.item() if out.ndim == 0 else out


def _pieces_dict(pieces: np.ndarray, shape: tuple) -> dict:
    return {name: _shaped(pieces[:, i], shape) for i, name in enumerate(IL_PIECES)}


# ---- Fourier side ------------------------------------------------------------------------------------------------------------
def _slice_launch(lib, phi_ptr: int, log_mgf_ptr: int, n_grid: int, n_sets: int, cases: np.ndarray, is_simpson: bool, out_ptr: int):
    logs = np.ascontiguousarray(np.log(cases[:, [0, 2, 3]]).T)          # log p1, log pa, log pb (:115-117)
    pf = C.POINTER(C.c_double)
    _lib.check(lib.svmc_mgf_il_slice_batch(phi_ptr, log_mgf_ptr, n_grid, n_sets, logs[0].ctypes.data_as(pf),
                                           logs[1].ctypes.data_as(pf), logs[2].ctypes.data_as(pf), cases.shape[0],
                                           int(bool(is_simpson)), out_ptr, None))


def il_slice_sums(phis: np.ndarray, log_mgfs: np.ndarray, cases: np.ndarray, is_simpson: bool = True) -> np.ndarray:
    """the five raw sums of svmc_mgf_il_slice_batch for [n_sets] given log-MGFs and the cases of il_cases in one launch per 32
    cases -> [n_sets][n_cases][5].  Raises compute_integration_weights' ValueErrors before any device work."""
    phi = np.ascontiguousarray(phis, dtype=np.complex128)
    lm = np.ascontiguousarray(log_mgfs, dtype=np.complex128)
    if not (phi.ndim == 2 and phi.shape == lm.shape):
        raise ValueError("il_slice_sums: phis / log_mgfs [n_sets][n_grid]")
    for row in phi:
        mgfp.compute_integration_weights(var_grid=row, is_simpson=is_simpson)
    n_out = phi.shape[0] * cases.shape[0] * IL_SLICE_SUMS

    def launch(lib, dphi, dlm, out):
        _slice_launch(lib, dphi.ptr, dlm.ptr, phi.shape[1], phi.shape[0], cases, is_simpson, out.ptr)

    return _given_log_mgf_call((2 * phi.size, 2 * lm.size, max(n_out, 1)), (phi, lm),
                               (phi.shape[0], cases.shape[0], IL_SLICE_SUMS), launch)


def square_root_payoff_pricer_with_mgf_grid(log_mgf_grid: np.ndarray, phi_grid: np.ndarray, forward: float, pa: float, pb: float,
                                            discfactor: float = 1.0, is_simpson: bool = True) -> float:
    """the price of the payoff sqrt(S) 1{pa < S < pb} from log E on the phi grid (reference :97-121), any model's log-MGF, on a
    contour -1/2 < Re phi < 0: discfactor nansum Re[(dp / pi) (exp((phi + 1/2) xb - phi x) - exp((phi + 1/2) xa - phi x)) /
    (phi + 1/2) exp(log E)] with compute_integration_weights' dp (its ValueErrors are raised before any device work)"""
    cases = np.array([[float(forward), 1.0, float(pa), float(pb), 1.0]])
    for name, v in (("forward", forward), ("pa", pa), ("pb", pb)):
        if not (np.isfinite(v) and v > 0.0):
            raise ValueError(f"square_root_payoff_pricer_with_mgf_grid: {name} must be positive and finite")
    if not pa < pb:
        raise ValueError("square_root_payoff_pricer_with_mgf_grid: the range needs pa < pb")
    sums = il_slice_sums(np.asarray(phi_grid, dtype=np.complex128).ravel()[None, :],
                         np.asarray(log_mgf_grid, dtype=np.complex128).ravel()[None, :], cases, is_simpson)
    return float(discfactor * sums[0, 0, 0])


def _logsv_il(params_list: Sequence[LogSvParams], ttm: float, cases: np.ndarray, order: int, vol_scaler, kwargs):
    """one ODE launch for all sets, one slice launch for all cases and sets -> (values [n_sets][n_cases], pieces
    [n_sets][n_cases][6], given-up counts, grid length)"""
    if not (np.isfinite(ttm) and ttm > 0.0):
        raise ValueError("impermanent loss: ttm must be positive and finite")
    phis = []
    for p in params_list:
        vs = vol_scaler
        if vs is None:                                            # :35-36
            vs = p.sigma0 * np.sqrt(np.minimum(np.min(ttm), 0.5 / 12.0))
        phi, psi, _ = mgfp.get_transform_var_grid(vol_scaler=vs, real_phi=IL_REAL_PHI, max_phi=IL_MAX_PHI)
        mgfp.compute_integration_weights(var_grid=phi, is_simpson=True)
        phis.append(phi)
    grid = AnalyticGrid.acquire(phis, [np.zeros_like(phi) for phi in phis], 5 if order == 2 else 3)
    try:
        rows = np.array([[p.sigma0, p.theta, p.kappa1, p.kappa2, p.beta, p.volvol, 1.0, 0.0] for p in params_list])
        grid.logsv_advance(ttm, rows, True, order, rtol=kwargs.get("ode_rtol"), atol=kwargs.get("ode_atol"))
        n_out = grid.n_sets * cases.shape[0] * IL_SLICE_SUMS
        grid.reserve_results(n_out)
        _slice_launch(grid.lib, grid.phi.ptr, grid.log_mgf.ptr, grid.n, grid.n_sets, cases, True, grid._capped.ptr)
        raw = grid.download_results(n_out).reshape(grid.n_sets, cases.shape[0], IL_SLICE_SUMS)
        given_up, n_grid = grid.last_given_up.copy(), grid.n
    finally:
        grid.release()
    value, pieces = il_compose(il_reference_sums(raw, True), cases[:, 0], cases[:, 1], cases[:, 2], cases[:, 3], cases[:, 4])
    return value, pieces, given_up, n_grid


def logsv_il_pricer(params: LogSvParams, ttm: float, p1, p0, pa, pb, is_stiff_solver: bool = False,
                    expansion_order: ExpansionOrder = ExpansionOrder.SECOND, vol_scaler: float = None, notional=1000000,
                    return_pieces: bool = False, **kwargs):
    """the LogSV price of the impermanent loss of the range [pa, pb] opened at p0, at the forward p1 (reference :20-91): a put
    and a digital put at pa, a call and a digital call at pb and the square-root payoff between them, all from one log-MGF on
    the contour Re phi = -0.4.  p1, p0, pa, pb and notional may be arrays, broadcast together: the log-MGF does not depend on
    them, so a whole profile of forwards costs one ODE launch and one slice launch.  A scalar comes back for scalar input.
    return_pieces=True -> (value, {IL_PIECES: ...}).  ode_rtol= / ode_atol= as logsv_chain_pricer.  Raises ValueError, before any
    device work, unless all prices and notionals are positive and finite with pa < p0 < pb."""
    from .logsv_pricer import _note_given_up
    cases, shape = il_cases(p1, p0, pa, pb, notional)
    note_integrator_flags(is_stiff_solver, False)
    value, pieces, given_up, n_grid = _logsv_il([params], float(ttm), cases, _order_code(expansion_order), vol_scaler, kwargs)
    _note_given_up(int(given_up[0]), n_grid)
    return (_shaped(value[0], shape), _pieces_dict(pieces[0], shape)) if return_pieces else _shaped(value[0], shape)


def logsv_il_pricer_vector(params: LogSvParams, ttm: float, p1, p0, pa, pb, is_stiff_solver: bool = False,
                           expansion_order: ExpansionOrder = ExpansionOrder.SECOND, vol_scaler: float = None, notional=1000000,
                           return_pieces: bool = False, **kwargs):
    """logsv_il_pricer under the reference's name for its np.vectorize form (:94).  Here `params` and `ttm` are scalars (one
    parameter set, one maturity: one log-MGF); p1, p0, pa, pb and notional are the vectorised arguments.  Several parameter
    sets: logsv_il_pricer_batch."""
    return logsv_il_pricer(params, ttm, p1, p0, pa, pb, is_stiff_solver=is_stiff_solver, expansion_order=expansion_order,
                           vol_scaler=vol_scaler, notional=notional, return_pieces=return_pieces, **kwargs)


def logsv_il_pricer_batch(params_list: Sequence[LogSvParams], ttm: float, p1, p0, pa, pb,
                          expansion_order: ExpansionOrder = ExpansionOrder.SECOND, vol_scaler: float = None, notional=1000000,
                          return_pieces: bool = False, **kwargs):
    """logsv_il_pricer for several parameter sets at one maturity and one list of cases: one svmc_logsv_mgf_grid_batch launch
    and one slice launch -> a list with each set's result, bit-equal to its single call.  Not in the reference API."""
    from .logsv_pricer import _note_given_up
    params_list = list(params_list)
    if not params_list:
        return []
    cases, shape = il_cases(p1, p0, pa, pb, notional)
    value, pieces, given_up, n_grid = _logsv_il(params_list, float(ttm), cases, _order_code(expansion_order), vol_scaler, kwargs)
    _note_given_up(given_up, n_grid)
    if return_pieces:
        return [(_shaped(v, shape), _pieces_dict(pc, shape)) for v, pc in zip(value, pieces)]
    return [_shaped(v, shape) for v in value]


# ---- Monte Carlo side --------------------------------------------------------------------------------------------------------
def il_mc_results(out: np.ndarray, shape: tuple, return_pieces: bool):
    """svmc_il_payoff's [n_cases][10] -> (value, stderr), and with return_pieces a dict of the six piece means and the counts"""
    value, stderr = _shaped(out[:, 0], shape), _shaped(out[:, 1], shape)
    if not return_pieces:
        return value, stderr
    extra = _pieces_dict(out[:, 2:8], shape)
    extra["n_kept"], extra["n_dropped"] = int(out[0, 8]), int(out[0, 9])
    return value, stderr, extra


def compute_mc_il_payoff(x0: np.ndarray, p1, p0, pa, pb, notional=1000000, return_pieces: bool = False):
    """the Monte Carlo impermanent loss from terminal log-returns x0 (host array), the estimator of include/svmc.h's
    svmc_il_payoff: spot = p1 exp(x) - (p1 M - p1) with M the mean of exp(x) over the kept paths (compute_mc_vars_payoff's
    recentring, formed once for all cases), a path kept iff x and exp(x) are finite, value = -(notional0 notional) mean(pay) and
    its standard error.  p1, p0, pa, pb, notional broadcast together and share the one path set.  Returns (value, stderr), and
    with return_pieces=True a dict of the six piece means, n_kept and n_dropped.  Upload, reduce on the device, results back."""
    from ..engine import get_engine
    il_cases(p1, p0, pa, pb, notional)                           # ValueError before any device work
    x0 = np.ascontiguousarray(x0, dtype=np.float64).ravel()
    if x0.size < 1:
        raise ValueError("compute_mc_il_payoff: no paths")
    eng = get_engine(x0.shape[0])
    eng.upload(eng.x.ptr, x0)
    return eng.il_payoffs(p1, p0, pa, pb, notional, return_pieces=return_pieces)


def refuse_sharded_il(who: str, kwargs: dict) -> None:
    """the IL reduction runs on one engine: a sharded request raises rather than estimate from one rank's paths"""
    from .. import dist as svdist
    comm = kwargs.get("comm")
    if kwargs.get("devices") is not None or (comm.world if comm is not None else svdist.get_default_comm().world) > 1:
        raise NotImplementedError(f"{who}: the impermanent-loss reduction is not sharded over ranks or devices")
