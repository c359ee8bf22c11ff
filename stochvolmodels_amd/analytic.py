"""
Host side of the analytic (Fourier) chain pricers: AnalyticGrid, the device buffers of n_sets >= 1 transform grids with thin
callers of libsvmc's batch entry points (svmc_logsv_mgf_grid_batch, svmc_hawkesjd_mgf_grid_batch, svmc_mgf_vanilla_slice_batch,
svmc_mgf_gamma_slice_batch, svmc_mgf_pdf_slice_batch; svmc_heston_mgf_grid and svmc_mgf_qvar_slice have no batch form) -- a
single-set pricing is the batch at one set, as it is inside the library -- and chain_sums, the one loop over a chain's expiries
that every analytic chain pricer runs (csrc/svmc_analytic.hip, svmc_hawkes.hip, svmc_density.hip).
Complex arrays travel as numpy.complex128 <-> interleaved doubles.  GPU only, like the Monte Carlo path.
"""
from __future__ import annotations

import ctypes as C
import threading
from itertools import accumulate
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .engine import DeviceBuffer, _current_device

# Dormand-Prince tolerances of the coefficient ODEs.  The reference uses SciPy's RK45 defaults (1e-3 / 1e-6),
# i.e. prices good to ~1e-6..1e-4; these reproduce the reference with its solver tightened to 1e-13 in price.
# The chain pricers take `ode_rtol=` / `ode_atol=` to trade that margin for time (tools/r04/analytic_tolerance_probe.py, a
# 4 x 21 chain, five parameter sets, DOP853: 1e-10 / 1e-12 -> 0.40-0.79 ms; 1e-8 / 1e-10 -> 0.31-0.71 ms, prices within
# 1.1e-11 of the default's; 1e-6 / 1e-8 -> 0.28-0.67 ms, within 4.5e-9; all of them stay 6.8e-7 from the reference as shipped
# -- its own solver's error.  With the 5(4) pair of rounds 1-3 the same settings took 0.92-1.22 / 0.52-0.84 / 0.39-0.69 ms).
ODE_RTOL, ODE_ATOL = 1e-10, 1e-12


# Grids are pooled per (thread, device, n_sets, n_grid, n_coef): a chain pricing took a grid's five allocations, two uploads
# (each with its own wait) and five frees -- 58 us per chain (tools/r04/analytic_grid_probe.py) of an 0.9-1.2 ms pricing, and the
# whole of it again at every objective evaluation of an analytic calibration, whose transform grid never changes.  acquire()
# hands back the pooled object with its ODE state zeroed (queued memsets) and re-uploads phi / psi only when their bytes changed;
# release() returns it.  One pooled grid per key: a second acquire() before the release() builds a private one.
_POOL = {}
_POOL_LOCK = threading.Lock()
MAX_POOLED_GRIDS = 8                        # resident pooled grids per process (a 1000-point, 5-coefficient grid is ~130 KB of HBM)


def _doubles(a) -> C.Array:
    """a small host array (parameter rows, strikes) as a `const double *` argument: a private float64 copy handed over
    through the buffer protocol -- the library reads it before the call returns.  These go out once or twice per expiry, and
    ndarray.ctypes.data_as costs 4 us a time where the copy and from_buffer cost 2."""
    a = np.array(a, dtype=np.float64, order="C")
    return (C.c_double * a.size).from_buffer(a)


class AnalyticGrid:
    """the transform grids phi (and psi) of n_sets >= 1 parameter sets resident on the device, with the per-grid-point ODE state
    of every set carried expiry to expiry: the sets advance in one launch per expiry (logsv_advance, hawkes_advance) and are
    inverted in one launch per expiry (queue_capped_sums, or queue_gamma_slice under the Hawkes risk-premia kernel) -- one
    chain, config C5's five sets, or the bumped parameter vectors of a finite-difference gradient side by side.
    phi / psi: one 1-D grid (one set), or a sequence / 2-D stack of n_sets grids of one length.  Per-set host data always has
    the leading set axis -- A [n_sets][n][n_coef], the log-MGF [n_sets][n], sums [n_sets][k], last_given_up [n_sets] -- and a
    set's bits do not depend on its neighbours in the launch; single-set callers take element 0.  Heston's closed form and the
    quadratic-variance inversion have no batch entry point: heston_advance and queue_qvar_sums need n_sets == 1."""

    @staticmethod
    def _shape(phi) -> Tuple[int, int]:
        """(n_sets, n_grid) of the constructor's phi, without copying it"""
        if len(phi) == 0 or np.ndim(phi[0]) == 0:
            return 1, len(phi)
        return len(phi), len(phi[0])

    @staticmethod
    def _stacked(z) -> np.ndarray:
        """a private [n_sets][n_grid] copy: the pooled object compares the NEXT caller's grids with it -- a caller that reuses and
        mutates its own array in place must not end up comparing the array with itself (and keeping a stale grid on the device)"""
        return np.array(z, dtype=np.complex128, copy=True, order="C", ndmin=2)

    @classmethod
    def acquire(cls, phi, psi, n_coef: int) -> "AnalyticGrid":
        key = (threading.get_ident(), _current_device()) + cls._shape(phi) + (int(n_coef),)
        with _POOL_LOCK:
            obj = _POOL.pop(key, None)
            if len(_POOL) > 8:                                  # grids of threads that ended: free their HBM
                alive = {t.ident for t in threading.enumerate()}
                for k in [k for k in _POOL if k[0] not in alive]:
                    _POOL.pop(k).close()
            while len(_POOL) > MAX_POOLED_GRIDS:                # ... and the least recently released ones beyond the cap: a
                _POOL.pop(next(iter(_POOL))).close()            # live thread that prices many grid shapes does not keep them all
        if obj is None:
            obj = cls(phi, psi, n_coef)
        else:
            obj._reset(phi, psi)
        obj._pool_slot = key
        return obj

    def release(self) -> None:
        key = getattr(self, "_pool_slot", None)
        with _POOL_LOCK:
            if key is not None and key not in _POOL:
                _POOL[key] = self
                return
        self.close()

    def _reset(self, phi, psi) -> None:
        for buf, z, name in ((self.phi, self._stacked(phi), "phi_host"), (self.psi, self._stacked(psi), "psi_host")):
            assert z.shape == (self.n_sets, self.n)
            if not np.array_equal(z, getattr(self, name)):
                _lib.check(self.lib.svmc_memcpy_h2d(buf.ptr, z.ctypes.data, z.nbytes, None))
                setattr(self, name, z)
        _lib.check(self.lib.svmc_stream_synchronize(None))     # pageable sources: the copies must not outlive the arrays
        _lib.check(self.lib.svmc_memset(self.a.ptr, 0, self.a.nbytes, None))
        _lib.check(self.lib.svmc_memset(self.b.ptr, 0, self.b.nbytes, None))     # Heston's chained have_t0 start from zero

    def __init__(self, phi, psi, n_coef: int):
        self.lib = _lib.load()
        cnt = C.c_int()
        _lib.check(self.lib.svmc_device_count(C.byref(cnt)))
        if cnt.value < 1:
            raise _lib.SvmcError("no HIP device visible: the analytic pricers run on the GPU only")
        self.phi_host, self.psi_host = self._stacked(phi), self._stacked(psi)
        self.n_sets, self.n = self.phi_host.shape
        self.n_coef = int(n_coef)
        assert self.psi_host.shape == (self.n_sets, self.n)
        self.phi, self.psi = self._up(self.phi_host), self._up(self.psi_host)
        self.last_given_up = np.zeros(self.n_sets, dtype=int)
        self.a = DeviceBuffer(2 * self.n_sets * self.n * self.n_coef)
        self.b = DeviceBuffer(2 * self.n_sets * self.n)
        self.log_mgf = DeviceBuffer(2 * self.n_sets * self.n)
        _lib.check(self.lib.svmc_memset(self.a.ptr, 0, self.a.nbytes, None))
        _lib.check(self.lib.svmc_memset(self.b.ptr, 0, self.b.nbytes, None))
        self._capped: Optional[DeviceBuffer] = None          # the queued results of a chain (reserve_results)
        self._risk: Optional[DeviceBuffer] = None            # normalizers then gamma forwards, [n_ttms][n_sets] each
        self._var: Optional[DeviceBuffer] = None             # a transform variable other than phi / psi (pdf_sums)
        self._risk_ttms = 0

    def _up(self, z: np.ndarray) -> DeviceBuffer:
        buf = DeviceBuffer(2 * z.size)
        _lib.check(self.lib.svmc_memcpy_h2d(buf.ptr, z.ctypes.data, z.nbytes, None))
        _lib.check(self.lib.svmc_stream_synchronize(None))
        return buf

    def _down(self, buf: DeviceBuffer, shape) -> np.ndarray:
        out = np.empty(shape, dtype=np.complex128)
        _lib.check(self.lib.svmc_memcpy_d2h(out.ctypes.data, buf.ptr, out.nbytes, None))
        _lib.check(self.lib.svmc_stream_synchronize(None))
        return out

    def set_a(self, a_t0: np.ndarray) -> None:
        """A(0) of every set, [n_sets][n_grid][n_coef] (zeros after acquire(); -Theta in the 2nd slot for the volatility)"""
        a_t0 = np.ascontiguousarray(a_t0, dtype=np.complex128)
        assert a_t0.shape == (self.n_sets, self.n, self.n_coef)
        _lib.check(self.lib.svmc_memcpy_h2d(self.a.ptr, a_t0.ctypes.data, a_t0.nbytes, None))
        _lib.check(self.lib.svmc_stream_synchronize(None))

    def get_a(self) -> np.ndarray:
        return self._down(self.a, (self.n_sets, self.n, self.n_coef))

    def get_log_mgf(self) -> np.ndarray:
        return self._down(self.log_mgf, (self.n_sets, self.n))

    def logsv_advance(self, ttm: float, params_rows: np.ndarray, is_spot_measure: bool, expansion_order: int,
                      rtol: Optional[float] = None, atol: Optional[float] = None) -> None:
        """params_rows [n_sets][8] = (sigma0, theta, kappa1, kappa2, beta, volvol, vol_backbone_eta, 0)"""
        assert np.shape(params_rows) == (self.n_sets, 8)
        _lib.check(self.lib.svmc_logsv_mgf_grid_batch(self.phi.ptr, self.psi.ptr, self.n, self.n_sets, float(ttm),
                                                      _doubles(params_rows), int(bool(is_spot_measure)),
                                                      int(expansion_order), self.a.ptr, self.log_mgf.ptr,
                                                      ODE_RTOL if rtol is None else float(rtol),
                                                      ODE_ATOL if atol is None else float(atol), None))

    def hawkes_advance(self, ttm: float, params_rows: np.ndarray, rtol: Optional[float] = None,
                       atol: Optional[float] = None) -> None:
        """params_rows [n_sets][16]: the Hawkes jump-diffusion parameter blocks (include/svmc.h SVMC_HAWKESJD_PARAMS order)"""
        assert np.shape(params_rows) == (self.n_sets, 16) and self.n_coef == 3
        _lib.check(self.lib.svmc_hawkesjd_mgf_grid_batch(self.phi.ptr, self.psi.ptr, self.n, self.n_sets, float(ttm),
                                                         _doubles(params_rows), self.a.ptr,
                                                         self.log_mgf.ptr, ODE_RTOL if rtol is None else float(rtol),
                                                         ODE_ATOL if atol is None else float(atol), None))

    def heston_advance(self, ttm, v0, theta, kappa, volvol, rho, have_t0: bool) -> None:
        assert self.n_sets == 1, "svmc_heston_mgf_grid has no batch form"
        _lib.check(self.lib.svmc_heston_mgf_grid(self.phi.ptr, self.psi.ptr, self.n, float(ttm), float(v0), float(theta),
                                                 float(kappa), float(volvol), float(rho), self.a.ptr, self.b.ptr,
                                                 int(bool(have_t0)), self.log_mgf.ptr, None))

    def risk_forwards(self, params_rows: np.ndarray, gammas: np.ndarray, ttms: np.ndarray, forwards: np.ndarray,
                      rtol: Optional[float] = None, atol: Optional[float] = None) -> None:
        """queue the risk-premia normalizers and gamma forwards of every set and expiry (svmc_hawkesjd_risk_forwards_batch)
        into the grid's device buffer, where queue_gamma_slice reads them; download_risk_results brings them back"""
        rows = np.ascontiguousarray(params_rows, dtype=np.float64)
        gammas = np.ascontiguousarray(gammas, dtype=np.float64)
        ttms = np.ascontiguousarray(ttms, dtype=np.float64)
        forwards = np.ascontiguousarray(forwards, dtype=np.float64)
        assert rows.shape == (self.n_sets, 16) and gammas.shape == (self.n_sets,) and ttms.shape == forwards.shape
        n = max(int(ttms.size), 1) * self.n_sets
        if self._risk is None or self._risk.n < 2 * n:
            if self._risk is not None:
                self._risk.free()
            self._risk = DeviceBuffer(2 * n)
        self._risk_ttms = int(ttms.size)
        pf = C.POINTER(C.c_double)
        _lib.check(self.lib.svmc_hawkesjd_risk_forwards_batch(rows.ctypes.data_as(pf), gammas.ctypes.data_as(pf), self.n_sets,
                                                              ttms.ctypes.data_as(pf), forwards.ctypes.data_as(pf), ttms.size,
                                                              self._risk.ptr, self._risk.offset(n),
                                                              ODE_RTOL if rtol is None else float(rtol),
                                                              ODE_ATOL if atol is None else float(atol), None))

    # -- the inversions are QUEUED into slices of one result buffer, downloaded once per chain: a chain's expiries are then
    #    launched back to back (advance, invert, advance, invert, ...) with no host round trip between them -- the wait for each
    #    expiry's sums cost a wake-up, the interpreter and a launch latency per expiry with the GPU idle (~50 us each)
    def reserve_results(self, n_doubles: int) -> None:
        if self._capped is None or self._capped.n < n_doubles:
            if self._capped is not None:
                self._capped.free()
            self._capped = DeviceBuffer(max(int(n_doubles), 32))

    def queue_capped_sums(self, forward: float, strikes: np.ndarray, offset: int, log_mgf_ptr: Optional[int] = None) -> None:
        """the [n_sets][n_strikes] capped sums of one expiry from the current log-MGF, queued into the result buffer at `offset`"""
        _lib.check(self.lib.svmc_mgf_vanilla_slice_batch(self.phi.ptr, log_mgf_ptr or self.log_mgf.ptr, self.n, self.n_sets,
                                                         float(forward), _doubles(strikes), np.size(strikes),
                                                         self._capped.offset(offset), None))

    def queue_qvar_sums(self, ttm: float, strikes: np.ndarray, offset: int) -> None:
        assert self.n_sets == 1, "svmc_mgf_qvar_slice has no batch form"
        _lib.check(self.lib.svmc_mgf_qvar_slice(self.psi.ptr, self.log_mgf.ptr, self.n, float(ttm), _doubles(strikes),
                                                np.size(strikes), self._capped.offset(offset), None))

    def queue_gamma_slice(self, gammas: np.ndarray, shortcut: np.ndarray, expiry: int, forward: float, strikes: np.ndarray,
                          type_codes: np.ndarray, offset: int) -> None:
        """the [n_sets][n_strikes] undiscounted risk-premia prices of expiry `expiry` from the current log-MGF, queued into
        the result buffer at `offset` (svmc_mgf_gamma_slice_batch; type codes 0 'C', 1 'P')"""
        strikes = np.ascontiguousarray(strikes, dtype=np.float64)
        codes = np.ascontiguousarray(type_codes, dtype=np.int32)
        gammas = np.ascontiguousarray(gammas, dtype=np.float64)
        short = np.ascontiguousarray(shortcut, dtype=np.int32)
        assert 0 <= expiry < self._risk_ttms and codes.shape == strikes.shape
        n = self._risk_ttms * self.n_sets
        pf, pi = C.POINTER(C.c_double), C.POINTER(C.c_int)
        _lib.check(self.lib.svmc_mgf_gamma_slice_batch(self.phi.ptr, self.log_mgf.ptr, self.n, self.n_sets,
                                                       gammas.ctypes.data_as(pf), short.ctypes.data_as(pi), self._risk.ptr,
                                                       self._risk.offset(n), int(expiry), float(forward),
                                                       strikes.ctypes.data_as(pf), codes.ctypes.data_as(pi), strikes.size,
                                                       self._capped.offset(offset), None))

    def _download(self, offset: int, shape) -> np.ndarray:
        """`shape` doubles of the result buffer from `offset` -- and, in the same wait, the log-MGF: a grid point the ODE
        integrator GAVE UP on (step floor / try cap of csrc/svmc_analytic.hip) is NaN there and stays NaN for every later
        expiry, and the inversion drops it like the reference's nansum -- silently.  self.last_given_up counts them per set
        (0 for every sane set): the chain pricers warn and a calibrator can penalise the evaluation."""
        out = np.empty(shape)
        lm = np.empty((self.n_sets, self.n), dtype=np.complex128)
        if out.size:
            _lib.check(self.lib.svmc_memcpy_d2h(out.ctypes.data, self._capped.offset(offset), out.nbytes, None))
        _lib.check(self.lib.svmc_memcpy_d2h(lm.ctypes.data, self.log_mgf.ptr, lm.nbytes, None))
        _lib.check(self.lib.svmc_stream_synchronize(None))
        self.last_given_up = np.isnan(lm).sum(axis=1)          # complex: NaN in either part
        return out

    def download_results(self, n_doubles: int) -> np.ndarray:
        """the queued sums of the chain; sets self.last_given_up (_download)"""
        return self._download(0, int(n_doubles))

    def download_risk_results(self, n_doubles: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(queued prices, normalizers [n_ttms][n_sets], gamma forwards [n_ttms][n_sets]) in one wait; last_given_up as in
        download_results"""
        n = self._risk_ttms * self.n_sets
        risk = np.empty(2 * n)
        if n:
            _lib.check(self.lib.svmc_memcpy_d2h(risk.ctypes.data, self._risk.ptr, risk.nbytes, None))
        out = self.download_results(n_doubles)
        return out, risk[:n].reshape(self._risk_ttms, self.n_sets), risk[n:].reshape(self._risk_ttms, self.n_sets)

    def capped_sums(self, forward: float, strikes: np.ndarray, log_mgf_ptr: Optional[int] = None) -> np.ndarray:
        """-> [n_sets][n_strikes], from the grid's log-MGF or from a caller's device copy of one (utils/mgf_pricer.py's slice
        pricer); the grid's own log-MGF is not looked at, last_given_up stays"""
        k = int(np.size(strikes))
        self.reserve_results(self.n_sets * k)
        self.queue_capped_sums(forward, strikes, 0, log_mgf_ptr=log_mgf_ptr)
        out = np.empty((self.n_sets, k))
        _lib.check(self.lib.svmc_memcpy_d2h(out.ctypes.data, self._capped.ptr, out.nbytes, None))
        _lib.check(self.lib.svmc_stream_synchronize(None))
        return out

    def _var_ptr(self, var_grids: np.ndarray) -> int:
        """`var_grids` uploaded into a buffer the grid keeps: a transform variable other than the resident phi / psi (the theta
        grid of the volatility)"""
        if self._var is None or self._var.n < 2 * var_grids.size:
            if self._var is not None:
                self._var.free()
            self._var = DeviceBuffer(2 * var_grids.size)
        _lib.check(self.lib.svmc_memcpy_h2d(self._var.ptr, var_grids.ctypes.data, var_grids.nbytes, None))
        return self._var.ptr

    def pdf_sums(self, var_grids: Sequence[np.ndarray], space_grids: Sequence[np.ndarray], shifts: Sequence[float],
                 scales: Sequence[float], is_simpson: bool = True, resident: Optional[str] = None) -> np.ndarray:
        """pdf_with_mgf_grid (reference utils/mgf_pricer.py:361-384) of every set from the log-MGF resident on the device, in
        ONE launch (svmc_mgf_pdf_slice_batch) -> [n_sets][n_space]; each set has its own transform grid (the variable the
        density is inverted over), space grid (of one common length), shift and scale.  resident="phi" / "psi" says the
        transform grids ARE the grid's phi / psi buffer, otherwise they are uploaded (the theta grid of the volatility).  The
        space grids and the masses go through the pooled result buffer; self.last_given_up is counted in the same wait."""
        space = np.array([np.ravel(s) for s in space_grids], dtype=np.float64, order="C")
        assert space.shape[0] == self.n_sets and len(var_grids) == np.size(shifts) == np.size(scales) == self.n_sets
        k = space.size
        self.reserve_results(2 * k)                                    # [spaces | masses]
        if resident is None:
            var = np.ascontiguousarray(np.stack([np.asarray(v, dtype=np.complex128).ravel() for v in var_grids]))
            assert var.shape == (self.n_sets, self.n)
        var_ptr = getattr(self, resident).ptr if resident in ("phi", "psi") else self._var_ptr(var)
        _lib.check(self.lib.svmc_memcpy_h2d(self._capped.ptr, space.ctypes.data, space.nbytes, None))
        _lib.check(self.lib.svmc_mgf_pdf_slice_batch(var_ptr, self.log_mgf.ptr, self.n, self.n_sets, self._capped.ptr,
                                                     space.shape[1], _doubles(shifts), _doubles(scales),
                                                     int(bool(is_simpson)), self._capped.offset(k), None))
        return self._download(k, space.shape)

    def close(self) -> None:
        for b in (self.phi, self.psi, self.a, self.b, self.log_mgf, self._capped, self._risk, self._var):
            if b is not None:
                b.free()


def chain_sums(grid: AnalyticGrid, ttms, forwards, strikes_ttms, advance: Callable[[int, float], None],
               inversion: str = "vanilla", gamma: Optional[tuple] = None):
    """the loop every analytic chain pricer runs on a grid of n_sets: reserve the chain's results, then per expiry
    advance(i, ttm_i - ttm_(i-1)) -- the caller's launch moving every set's ODE state on to expiry i -- and the queued
    inversion, then ONE download, so no host round trip separates the expiries.  inversion: "vanilla" (queue_capped_sums),
    "qvar" (queue_qvar_sums: one set) or "gamma" (queue_gamma_slice, with gamma = (gammas, shortcut, type codes per expiry)
    and the caller's risk_forwards launch queued before).  Expiry i's [n_sets][k_i] block sits at cumsum(n_sets * k_i): an
    expiry without strikes takes no space.  -> sums[set][expiry], the views of the one downloaded array; under "gamma"
    (sums, normalizers, gamma forwards) as download_risk_results gives them.  grid.last_given_up is set by the download."""
    n_sets = grid.n_sets
    strikes = [np.asarray(k, dtype=np.float64) for k in strikes_ttms]
    offs = [0, *accumulate(n_sets * k.size for k in strikes)]
    grid.reserve_results(offs[-1])
    ttm0, n_exp = 0.0, 0
    for i, (ttm, forward, k) in enumerate(zip(ttms, forwards, strikes)):
        advance(i, ttm - ttm0)
        if inversion == "vanilla":
            grid.queue_capped_sums(float(forward), k, offs[i])
        elif inversion == "qvar":
            grid.queue_qvar_sums(float(ttm), k, offs[i])
        else:
            grid.queue_gamma_slice(gamma[0], gamma[1], i, float(forward), k.ravel(), gamma[2][i], offs[i])
        ttm0, n_exp = ttm, i + 1
    if inversion == "gamma":
        flat, *risk = grid.download_risk_results(offs[-1])
    else:
        flat, risk = grid.download_results(offs[-1]), []
    sums = [[flat[offs[i] + s * k.size:offs[i] + (s + 1) * k.size] for i, k in enumerate(strikes[:n_exp])] for s in range(n_sets)]
    return (sums, *risk) if inversion == "gamma" else sums


def chain_prices_from_sums(sums: List[List[np.ndarray]], inversion: str, ttms, forwards, discfactors, strikes_ttms,
                           optiontypes_ttms, is_spot_measure: bool = True) -> List[List[np.ndarray]]:
    """chain_sums' "vanilla" or "qvar" sums [set][expiry] -> prices [set][expiry] (vanilla_prices_from_capped,
    qvar_prices_from_sums)"""
    out = [[] for _ in sums]
    for i, (ttm, forward, discfactor, strikes, types) in enumerate(zip(ttms, forwards, discfactors, strikes_ttms,
                                                                       optiontypes_ttms)):
        for s, of_set in enumerate(sums):
            if inversion == "vanilla":
                out[s].append(vanilla_prices_from_capped(of_set[i], float(forward), strikes, types, float(discfactor),
                                                         is_spot_measure))
            else:
                out[s].append(qvar_prices_from_sums(of_set[i], float(ttm), types, float(discfactor)))
    return out


def _given_log_mgf_call(sizes: Sequence[int], uploads: Sequence[np.ndarray], out_shape, launch: Callable) -> np.ndarray:
    """the scaffold of the three given-log-MGF functions below: scratch DeviceBuffers of `sizes` doubles -- the first
    len(uploads) of them filled from those host arrays, the last one the result's -- then launch(lib, *buffers), ONE download of
    `out_shape` doubles from the last buffer, one synchronize, and the frees whatever happened"""
    lib = _lib.load()
    bufs = [DeviceBuffer(n) for n in sizes]
    try:
        for buf, z in zip(bufs, uploads):
            _lib.check(lib.svmc_memcpy_h2d(buf.ptr, z.ctypes.data, z.nbytes, None))
        launch(lib, *bufs)
        out = np.empty(out_shape)
        if out.size:
            _lib.check(lib.svmc_memcpy_d2h(out.ctypes.data, bufs[-1].ptr, out.nbytes, None))
        _lib.check(lib.svmc_stream_synchronize(None))
        return out
    finally:
        for b in bufs:
            b.free()


def gamma_slice_prices(phi: np.ndarray, log_mgf: np.ndarray, gamma: float, shortcut: bool, normalizer: float,
                       gamma_forward: float, forward: float, strikes: np.ndarray, type_codes: np.ndarray) -> np.ndarray:
    """one slice under the risk-premia kernel from a given log-MGF (svmc_mgf_gamma_slice_batch at one set): uploads the grid,
    the log-MGF and the slice's normalizer / gamma forward, returns the undiscounted prices"""
    phi = np.ascontiguousarray(phi, dtype=np.complex128)
    log_mgf = np.ascontiguousarray(log_mgf, dtype=np.complex128)
    strikes = np.ascontiguousarray(strikes, dtype=np.float64)
    codes = np.ascontiguousarray(type_codes, dtype=np.int32)
    nf = np.array([normalizer, gamma_forward], dtype=np.float64)
    gammas, short = np.array([gamma], dtype=np.float64), np.array([int(bool(shortcut))], dtype=np.int32)
    pf, pi = C.POINTER(C.c_double), C.POINTER(C.c_int)

    def launch(lib, dphi, dlm, dnf, out):
        _lib.check(lib.svmc_mgf_gamma_slice_batch(dphi.ptr, dlm.ptr, phi.size, 1, gammas.ctypes.data_as(pf),
                                                  short.ctypes.data_as(pi), dnf.ptr, dnf.offset(1), 0, float(forward),
                                                  strikes.ctypes.data_as(pf), codes.ctypes.data_as(pi), strikes.size, out.ptr, None))

    return _given_log_mgf_call((2 * phi.size, 2 * log_mgf.size, 2, max(strikes.size, 1)), (phi, log_mgf, nf), strikes.size, launch)


def pdf_slices(var_grids: np.ndarray, log_mgfs: np.ndarray, space_grids: np.ndarray, shifts, scales,
               is_simpson: bool = True) -> np.ndarray:
    """pdf_with_mgf_grid for [n_sets] given log-MGFs in one launch (svmc_mgf_pdf_slice_batch): var_grids, log_mgfs
    [n_sets][n_grid] complex, space_grids [n_sets][n_space], shifts / scales [n_sets] -> [n_sets][n_space].  Uploads its
    inputs; the pricers keep the log-MGF on the device instead (AnalyticGrid.pdf_sums)."""
    var = np.ascontiguousarray(var_grids, dtype=np.complex128)
    lm = np.ascontiguousarray(log_mgfs, dtype=np.complex128)
    space = np.ascontiguousarray(space_grids, dtype=np.float64)
    sh, sc = np.ascontiguousarray(shifts, dtype=np.float64), np.ascontiguousarray(scales, dtype=np.float64)
    if not (var.ndim == 2 and var.shape == lm.shape and space.ndim == 2 and space.shape[0] == var.shape[0]
            and sh.shape == sc.shape == (var.shape[0],)):
        raise ValueError("pdf_slices: var_grids / log_mgfs [n_sets][n_grid], space_grids [n_sets][n_space], shifts / scales [n_sets]")
    pf = C.POINTER(C.c_double)

    def launch(lib, dvar, dlm, dspace, out):
        _lib.check(lib.svmc_mgf_pdf_slice_batch(dvar.ptr, dlm.ptr, var.shape[1], var.shape[0], dspace.ptr, space.shape[1],
                                                sh.ctypes.data_as(pf), sc.ctypes.data_as(pf), int(bool(is_simpson)), out.ptr, None))

    return _given_log_mgf_call((2 * var.size, 2 * lm.size, max(space.size, 1), max(space.size, 1)), (var, lm, space), space.shape,
                               launch)


def digital_slice_sums(phis: np.ndarray, log_mgfs: np.ndarray, forward: float, strikes: np.ndarray, negative_contour: bool,
                       is_simpson: bool = True) -> np.ndarray:
    """the strike sums of digital_slice_pricer_with_mgf_grid for [n_sets] given log-MGFs in one launch
    (svmc_mgf_digital_slice_batch) -> [n_sets][n_strikes]"""
    phi = np.ascontiguousarray(phis, dtype=np.complex128)
    lm = np.ascontiguousarray(log_mgfs, dtype=np.complex128)
    strikes = np.ascontiguousarray(strikes, dtype=np.float64).ravel()
    if not (phi.ndim == 2 and phi.shape == lm.shape):
        raise ValueError("digital_slice_sums: phis / log_mgfs [n_sets][n_grid]")

    def launch(lib, dphi, dlm, out):
        _lib.check(lib.svmc_mgf_digital_slice_batch(dphi.ptr, dlm.ptr, phi.shape[1], phi.shape[0], float(forward),
                                                    strikes.ctypes.data_as(C.POINTER(C.c_double)), strikes.size,
                                                    int(bool(negative_contour)), int(bool(is_simpson)), out.ptr, None))

    return _given_log_mgf_call((2 * phi.size, 2 * lm.size, max(strikes.size * phi.shape[0], 1)), (phi, lm),
                               (phi.shape[0], strikes.size), launch)


def digital_prices_from_sums(sums: np.ndarray, optiontypes: Sequence, discfactor: float, is_all_calls: bool) -> np.ndarray:
    """the payoff algebra of digital_slice_pricer_with_mgf_grid, reference utils/mgf_pricer.py:254-267"""
    prices = np.zeros(len(sums))
    for idx, (s, type_) in enumerate(zip(sums, optiontypes)):
        type_ = str(type_)
        if type_ == "C":
            price = s if is_all_calls else 1.0 - s
        elif type_ == "P":
            price = 1.0 - s if is_all_calls else s
        else:
            raise ValueError("not implemented")
        prices[idx] = discfactor * price
    return prices


def histogram_edges(lo: float, hi: float, n_bins: int) -> np.ndarray:
    """the bin edges np.histogram(a, bins=n_bins, range=(lo, hi)) itself forms (its checks and its widening of lo == hi included)"""
    return np.ascontiguousarray(np.histogram_bin_edges(np.empty(0), bins=int(n_bins), range=(float(lo), float(hi))),
                                dtype=np.float64)


def device_histograms(value_ptrs: Sequence[int], n: int, edges_list: Sequence[np.ndarray], divisors: Sequence[float],
                      stream=None) -> list:
    """np.histogram counts of several device vectors of `n` doubles (svmc_histogram_uniform), one launch per vector and ONE
    download of all the counts: [int64 counts [len(edges) - 1]] per vector, equal to np.histogram(values / divisor,
    bins=len(edges) - 1, range=(edges[0], edges[-1]))[0] of the downloaded values"""
    lib = _lib.load()
    edges_list = [np.ascontiguousarray(e, dtype=np.float64) for e in edges_list]
    n_edges = [e.size for e in edges_list]
    eoff = np.concatenate([[0], np.cumsum(n_edges)]).astype(int)
    coff = np.concatenate([[0], np.cumsum([m - 1 for m in n_edges])]).astype(int)
    all_edges = np.concatenate(edges_list)
    bufs = [DeviceBuffer(all_edges.size), DeviceBuffer(max(int(coff[-1]), 1))]           # counts: uint64, 8 bytes each
    try:
        _lib.check(lib.svmc_memcpy_h2d(bufs[0].ptr, all_edges.ctypes.data, all_edges.nbytes, stream))
        for i, (ptr, div) in enumerate(zip(value_ptrs, divisors)):
            _lib.check(lib.svmc_histogram_uniform(ptr, int(n), float(div), bufs[0].offset(eoff[i]), n_edges[i] - 1,
                                                  bufs[1].offset(coff[i]), stream))
        counts = np.empty(int(coff[-1]), dtype=np.uint64)
        _lib.check(lib.svmc_memcpy_d2h(counts.ctypes.data, bufs[1].ptr, counts.nbytes, stream))
        _lib.check(lib.svmc_stream_synchronize(stream))
        return [counts[coff[i]:coff[i + 1]].astype(np.int64) for i in range(len(edges_list))]
    finally:
        for b in bufs:
            b.free()


KDE_TILE, KDE_MAX_POINTS, KDE_STATS_DOUBLES = 8, 4096, 8     # SVMC_KDE_* of include/svmc.h
KDE_STATS_FIELDS = ("n_kept", "n_nan", "n_low", "n_high", "mean", "var", "h", "factor")


def _kde_workspace(size_fn: str, n: int) -> Tuple[int, int]:
    nbytes, chunk = C.c_size_t(0), C.c_size_t(0)
    _lib.check(getattr(_lib.load(), size_fn)(int(n), C.byref(nbytes), C.byref(chunk)))
    return int(nbytes.value), int(chunk.value)


def kde_workspace(n: int) -> Tuple[int, int]:
    """(workspace bytes, chunk length) of svmc_kde_gaussian at `n` samples: both depend on n alone (svmc_kde_workspace_bytes)"""
    return _kde_workspace("svmc_kde_workspace_bytes", n)


def _device_kdes(entry: str, size_fn: str, fields: Sequence[str], weight_args, value_ptrs, n, grids, divisors, limit, bandwidth_factor,
                 stream) -> list:
    """the body of device_kdes and device_kdes_weighted: one upload of all the grids, per vector one call of the library's
    `entry` -- weight_args(i) are the arguments it takes between the values and n -- with the workspace of `size_fn`, one
    download, the slicing into [(density, kde_stats of the `fields`)]"""
    lib = _lib.load()
    grids = [np.ascontiguousarray(g, dtype=np.float64).ravel() for g in grids]
    sizes = [g.size for g in grids]
    goff = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    total, n_vec, nst = int(goff[-1]), len(grids), len(fields)
    all_grids = np.concatenate(grids) if grids else np.empty(0)
    ws_bytes = _kde_workspace(size_fn, n)[0]
    # results: the densities of all vectors, then their stats blocks -- one buffer, one download
    bufs = [DeviceBuffer(max(total, 1)), DeviceBuffer(max(total + nst * n_vec, 1)), DeviceBuffer(max(ws_bytes // 8, 1))]
    try:
        _lib.check(lib.svmc_memcpy_h2d(bufs[0].ptr, all_grids.ctypes.data, all_grids.nbytes, stream))
        for i, (ptr, div) in enumerate(zip(value_ptrs, divisors)):
            _lib.check(getattr(lib, entry)(ptr, *weight_args(i), int(n), float(div), float(limit), bufs[0].offset(goff[i]), sizes[i],
                                           float(bandwidth_factor or 0.0), bufs[1].offset(goff[i]), bufs[1].offset(total + nst * i),
                                           bufs[2].ptr, ws_bytes, stream))
        out = np.empty(total + nst * n_vec)
        _lib.check(lib.svmc_memcpy_d2h(out.ctypes.data, bufs[1].ptr, out.nbytes, stream))
        _lib.check(lib.svmc_stream_synchronize(stream))
    finally:
        for b in bufs:
            b.free()
    return [(out[goff[i]:goff[i + 1]].copy(), kde_stats(out[total + nst * i:total + nst * (i + 1)], fields)) for i in range(n_vec)]


def device_kdes(value_ptrs: Sequence[int], n: int, grids: Sequence[np.ndarray], divisors: Sequence[float], limit: float = 1e16,
                bandwidth_factor: Optional[float] = None, stream=None) -> list:
    """scipy.stats.gaussian_kde(kept)(grid) of several device vectors of `n` doubles (svmc_kde_gaussian): the sample is
    values / divisor, NaNs and samples beyond +-limit are dropped and counted, the bandwidth is Scott's unless a positive
    factor is given.  One upload of all the grids, the launches of all the vectors on one stream, ONE download of all the
    densities and stats blocks: [(density [len(grid)], {n_kept, n_nan, n_low, n_high, mean, var, h, factor})] per vector.
    Raises SciPy's two exceptions: ValueError with fewer than two kept samples, numpy.linalg.LinAlgError where their variance
    is not positive and finite."""
    return _device_kdes("svmc_kde_gaussian", "svmc_kde_workspace_bytes", KDE_STATS_FIELDS, lambda i: (), value_ptrs, n, grids, divisors,
                        limit, bandwidth_factor, stream)


def kde_stats(block: np.ndarray, fields: Sequence[str] = KDE_STATS_FIELDS) -> dict:
    """a downloaded stats block of svmc_kde_gaussian (or, with KDE_WEIGHTED_STATS_FIELDS, of svmc_kde_gaussian_weighted) as a dict
    (the counts as ints), with gaussian_kde's refusals: ValueError for fewer than two kept samples, LinAlgError for a variance
    that is not positive and finite"""
    stats = {k: (int(v) if k.startswith("n_") and np.isfinite(v) else float(v)) for k, v in zip(fields, block)}
    if not stats["n_kept"] >= 2:
        raise ValueError(f"kernel density estimate: {stats['n_kept']} samples kept, at least two are needed")
    if not (np.isfinite(stats["var"]) and stats["var"] > 0.0):
        raise np.linalg.LinAlgError(f"kernel density estimate: the variance of the kept samples is {stats['var']}")
    return stats


KDE_WEIGHTED_STATS_DOUBLES = 12                             # SVMC_KDE_WEIGHTED_STATS_DOUBLES of include/svmc.h
KDE_WEIGHTED_STATS_FIELDS = ("n_kept", "n_nan", "n_low", "n_high", "n_bad_weight", "sum_w", "neff", "mean", "var", "h", "factor",
                             "sum_w2")


def kde_weighted_workspace(n: int) -> Tuple[int, int]:
    """(workspace bytes, chunk length) of svmc_kde_gaussian_weighted at `n` samples (svmc_kde_weighted_workspace_bytes): the
    chunk length is kde_workspace's, the workspace is larger (eight rows of moment partials)"""
    return _kde_workspace("svmc_kde_weighted_workspace_bytes", n)


def device_kdes_weighted(value_ptrs: Sequence[int], n: int, grids: Sequence[np.ndarray], divisors: Sequence[float],
                         weight_ptrs: Optional[Sequence[Optional[int]]] = None, tilt_ptrs: Optional[Sequence[Optional[int]]] = None,
                         gammas: Optional[Sequence[float]] = None, limit: float = 1e16, bandwidth_factor: Optional[float] = None,
                         stream=None) -> list:
    """scipy.stats.gaussian_kde(kept, weights=w_kept)(grid) of several device vectors of `n` doubles
    (svmc_kde_gaussian_weighted): device_kdes with the weight w = weights exp(gamma tilt) per sample.  weight_ptrs, tilt_ptrs:
    per vector a device pointer to `n` doubles or None (the factor is then 1; a whole argument of None means None for every
    vector); gammas: per vector the gamma of its tilt (default 0).  The tilt is NOT divided by the divisor.  Samples with a
    weight that is NaN, negative or not finite (an overflowed exponential included) are dropped and counted in n_bad_weight.
    One upload of all the grids, the launches of all the vectors on one stream, ONE download: [(density [len(grid)],
    {KDE_WEIGHTED_STATS_FIELDS})] per vector.  Raises ValueError with fewer than two kept samples and numpy.linalg.LinAlgError
    where the weighted variance is not positive and finite -- a single non-zero weight among them.  That is this project's own
    rule: SciPy 1.15.3 raises ValueError("array must not contain infs or NaNs") in that corner, and parity of exceptions
    there is not claimed."""
    n_vec = len(grids)
    weight_ptrs = [None] * n_vec if weight_ptrs is None else list(weight_ptrs)
    tilt_ptrs = [None] * n_vec if tilt_ptrs is None else list(tilt_ptrs)
    gammas = [0.0] * n_vec if gammas is None else [float(g) for g in gammas]
    if not (len(value_ptrs) == len(divisors) == len(weight_ptrs) == len(tilt_ptrs) == len(gammas) == n_vec):
        raise ValueError("device_kdes_weighted: one grid, divisor, weights pointer, tilt pointer and gamma per vector")
    return _device_kdes("svmc_kde_gaussian_weighted", "svmc_kde_weighted_workspace_bytes", KDE_WEIGHTED_STATS_FIELDS,
                        lambda i: (weight_ptrs[i] or None, tilt_ptrs[i] or None, gammas[i]), value_ptrs, n, grids, divisors, limit,
                        bandwidth_factor, stream)


def vanilla_prices_from_capped(capped: np.ndarray, forward: float, strikes: np.ndarray, optiontypes: Sequence,
                               discfactor: float, is_spot_measure: bool) -> np.ndarray:
    """the payoff algebra of vanilla_slice_pricer_with_mgf_grid, reference utils/mgf_pricer.py:199-219"""
    strikes = np.asarray(strikes, dtype=np.float64)
    x = np.log(forward / strikes)
    prices = np.zeros_like(x)
    for idx, (xk, strike, type_, cap) in enumerate(zip(x, strikes, optiontypes, capped)):
        type_ = str(type_)
        if is_spot_measure:
            if type_ == "C":
                prices[idx] = discfactor * (forward - strike * cap)
            elif type_ == "P":
                prices[idx] = discfactor * (strike - strike * cap)
            else:
                raise ValueError("not implemented")
        else:
            if type_ in ("IC", "C"):
                prices[idx] = forward * discfactor * (1.0 - cap)
            elif type_ in ("IP", "P"):
                prices[idx] = forward * discfactor * (np.exp(-xk) - cap)
            else:
                raise ValueError("not implemented")
    return prices


def qvar_prices_from_sums(sums: np.ndarray, ttm: float, optiontypes: Sequence, discfactor: float) -> np.ndarray:
    """the payoff algebra of slice_qvar_pricer_with_a_grid, reference utils/mgf_pricer.py:343-356 (calls only)"""
    prices = np.zeros_like(sums)
    for idx, (s, type_) in enumerate(zip(sums, optiontypes)):
        if str(type_) != "C":
            raise ValueError("not implemented")
        prices[idx] = np.maximum(discfactor * s / ttm, 1e-10)
    return prices
