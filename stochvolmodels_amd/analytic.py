"""
Host side of the analytic (Fourier) chain pricers: device buffers for the transform grid and thin callers of
libsvmc's svmc_logsv_mgf_grid / svmc_heston_mgf_grid / svmc_mgf_vanilla_slice (csrc/svmc_analytic.hip).
Complex arrays travel as numpy.complex128 <-> interleaved doubles.  GPU only, like the Monte Carlo path.
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Optional, Sequence, Tuple

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


# Grids are pooled per (thread, device, class, sizes): a chain pricing took a grid's five allocations, two uploads (each with its own
# wait) and five frees -- 58 us per chain (tools/r04/analytic_grid_probe.py) of an 0.9-1.2 ms pricing, and the whole of it
# again at every objective evaluation of an analytic calibration, whose transform grid never changes.  acquire() hands back
# the pooled object with its ODE state zeroed (queued memsets) and re-uploads phi / psi only when their bytes changed;
# release() returns it.  One pooled grid per key: a second acquire() before the release() builds a private one.
_POOL = {}
_POOL_LOCK = threading.Lock()
MAX_POOLED_GRIDS = 8                        # resident pooled grids per process (a 1000-point, 5-coefficient grid is ~130 KB of HBM)


class _Pooled:
    @classmethod
    def acquire(cls, *args):
        key = (threading.get_ident(), _current_device(), cls.__name__) + cls._pool_key(*args)
        with _POOL_LOCK:
            obj = _POOL.pop(key, None)
            if len(_POOL) > 8:                                  # grids of threads that ended: free their HBM
                alive = {t.ident for t in threading.enumerate()}
                for k in [k for k in _POOL if k[0] not in alive]:
                    _POOL.pop(k).close()
            while len(_POOL) > MAX_POOLED_GRIDS:                # ... and the least recently released ones beyond the cap: a
                _POOL.pop(next(iter(_POOL))).close()            # live thread that prices many grid shapes does not keep them all
        if obj is None:
            obj = cls(*args)
        else:
            obj._reset(*args)
        obj._pool_slot = key
        return obj

    def release(self) -> None:
        key = getattr(self, "_pool_slot", None)
        with _POOL_LOCK:
            if key is not None and key not in _POOL:
                _POOL[key] = self
                return
        self.close()


class AnalyticGrid(_Pooled):
    """transform grid phi (and psi) resident on the device, with the per-grid-point ODE state carried slice to slice"""

    @staticmethod
    def _pool_key(phi, psi, n_coef):
        return (int(np.asarray(phi).size), int(n_coef))

    def _reset(self, phi, psi, n_coef) -> None:
        # private copies: the pooled object compares the NEXT caller's grid with these -- a caller that reuses and mutates its
        # own array in place must not end up comparing the array with itself (and keeping a stale grid on the device)
        phi = np.array(phi, dtype=np.complex128, copy=True, order="C")
        psi = np.array(psi, dtype=np.complex128, copy=True, order="C")
        if not np.array_equal(phi, self.phi_host):
            _lib.check(self.lib.svmc_memcpy_h2d(self.phi.ptr, phi.ctypes.data, phi.nbytes, None))
            self.phi_host = phi
        if not np.array_equal(psi, self.psi_host):
            _lib.check(self.lib.svmc_memcpy_h2d(self.psi.ptr, psi.ctypes.data, psi.nbytes, None))
            self.psi_host = psi
        _lib.check(self.lib.svmc_stream_synchronize(None))     # pageable sources: the copies must not outlive the arrays
        _lib.check(self.lib.svmc_memset(self.a.ptr, 0, self.a.nbytes, None))
        _lib.check(self.lib.svmc_memset(self.b.ptr, 0, self.b.nbytes, None))

    def __init__(self, phi: np.ndarray, psi: np.ndarray, n_coef: int):
        self.lib = _lib.load()
        cnt = C.c_int()
        _lib.check(self.lib.svmc_device_count(C.byref(cnt)))
        if cnt.value < 1:
            raise _lib.SvmcError("no HIP device visible: the analytic pricers run on the GPU only")
        self.n = int(phi.size)
        self.n_coef = int(n_coef)
        self.phi_host = np.array(phi, dtype=np.complex128, copy=True, order="C")
        self.phi = self._up(self.phi_host)
        self.psi_host = np.array(psi, dtype=np.complex128, copy=True, order="C")
        self.psi = self._up(self.psi_host)
        self.last_given_up = 0
        self.a = DeviceBuffer(2 * self.n * self.n_coef)
        self.b = DeviceBuffer(2 * self.n)
        self.log_mgf = DeviceBuffer(2 * self.n)
        _lib.check(self.lib.svmc_memset(self.a.ptr, 0, self.a.nbytes, None))
        _lib.check(self.lib.svmc_memset(self.b.ptr, 0, self.b.nbytes, None))
        self._capped: Optional[DeviceBuffer] = None
        self._var: Optional[DeviceBuffer] = None             # a transform variable other than phi / psi (pdf_sums)

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
        a_t0 = np.ascontiguousarray(a_t0, dtype=np.complex128)
        assert a_t0.shape == (self.n, self.n_coef)
        _lib.check(self.lib.svmc_memcpy_h2d(self.a.ptr, a_t0.ctypes.data, a_t0.nbytes, None))
        _lib.check(self.lib.svmc_stream_synchronize(None))

    def get_a(self) -> np.ndarray:
        return self._down(self.a, (self.n, self.n_coef))

    def get_log_mgf(self) -> np.ndarray:
        return self._down(self.log_mgf, (self.n,))

    def logsv_advance(self, ttm, sigma0, theta, kappa1, kappa2, beta, volvol, is_spot_measure, expansion_order,
                      vol_backbone_eta, rtol: Optional[float] = None, atol: Optional[float] = None) -> None:
        _lib.check(self.lib.svmc_logsv_mgf_grid(self.phi.ptr, self.psi.ptr, self.n, float(ttm), float(sigma0),
                                                float(theta), float(kappa1), float(kappa2), float(beta), float(volvol),
                                                int(bool(is_spot_measure)), int(expansion_order), float(vol_backbone_eta),
                                                self.a.ptr, self.log_mgf.ptr, ODE_RTOL if rtol is None else float(rtol),
                                                ODE_ATOL if atol is None else float(atol), None))

    def heston_advance(self, ttm, v0, theta, kappa, volvol, rho, have_t0: bool) -> None:
        _lib.check(self.lib.svmc_heston_mgf_grid(self.phi.ptr, self.psi.ptr, self.n, float(ttm), float(v0), float(theta),
                                                 float(kappa), float(volvol), float(rho), self.a.ptr, self.b.ptr,
                                                 int(bool(have_t0)), self.log_mgf.ptr, None))

    def capped_sums(self, forward: float, strikes: np.ndarray, log_mgf_ptr: Optional[int] = None) -> np.ndarray:
        strikes = np.ascontiguousarray(strikes, dtype=np.float64)
        k = strikes.size
        if self._capped is None or self._capped.n < k:
            self._capped = DeviceBuffer(max(k, 32))
        _lib.check(self.lib.svmc_mgf_vanilla_slice(self.phi.ptr, log_mgf_ptr or self.log_mgf.ptr, self.n, float(forward),
                                                   strikes.ctypes.data_as(C.POINTER(C.c_double)), k, self._capped.ptr, None))
        out = np.empty(k)
        _lib.check(self.lib.svmc_memcpy_d2h(out.ctypes.data, self._capped.ptr, 8 * k, None))
        _lib.check(self.lib.svmc_stream_synchronize(None))
        return out

    # -- the same two reductions QUEUED into slices of one result buffer, downloaded once per chain: a chain's expiries are
    #    then launched back to back (advance, invert, advance, invert, ...) with no host round trip between them -- the wait
    #    for each expiry's sums cost a wake-up, the interpreter and a launch latency per expiry with the GPU idle (~50 us each)
    def reserve_results(self, n_doubles: int) -> None:
        if self._capped is None or self._capped.n < n_doubles:
            if self._capped is not None:
                self._capped.free()
            self._capped = DeviceBuffer(max(int(n_doubles), 32))

    def queue_capped_sums(self, forward: float, strikes: np.ndarray, offset: int) -> None:
        strikes = np.ascontiguousarray(strikes, dtype=np.float64)      # copied by the call (kernel arguments / pinned staging)
        _lib.check(self.lib.svmc_mgf_vanilla_slice(self.phi.ptr, self.log_mgf.ptr, self.n, float(forward),
                                                   strikes.ctypes.data_as(C.POINTER(C.c_double)), strikes.size,
                                                   self._capped.offset(offset), None))

    def queue_qvar_sums(self, ttm: float, strikes: np.ndarray, offset: int) -> None:
        strikes = np.ascontiguousarray(strikes, dtype=np.float64)
        _lib.check(self.lib.svmc_mgf_qvar_slice(self.psi.ptr, self.log_mgf.ptr, self.n, float(ttm),
                                                strikes.ctypes.data_as(C.POINTER(C.c_double)), strikes.size,
                                                self._capped.offset(offset), None))

    def download_results(self, n_doubles: int) -> np.ndarray:
        """the queued sums of the chain -- and, in the same wait, the last expiry's log-MGF: a grid point the ODE integrator
        GAVE UP on (step floor / try cap of csrc/svmc_analytic.hip) is NaN there and stays NaN for every later expiry, and the
        inversion drops it like the reference's nansum -- silently.  self.last_given_up counts them (0 for every sane set):
        the chain pricers warn and a calibrator can penalise the evaluation."""
        out = np.empty(int(n_doubles))
        lm = np.empty(self.n, dtype=np.complex128)
        _lib.check(self.lib.svmc_memcpy_d2h(out.ctypes.data, self._capped.ptr, 8 * int(n_doubles), None))
        _lib.check(self.lib.svmc_memcpy_d2h(lm.ctypes.data, self.log_mgf.ptr, lm.nbytes, None))
        _lib.check(self.lib.svmc_stream_synchronize(None))
        self.last_given_up = int(np.count_nonzero(np.isnan(lm.real) | np.isnan(lm.imag)))
        return out

    def _var_ptr(self, var_grid: np.ndarray, resident: Optional[str]) -> int:
        """the device copy of the transform variable an inversion runs over: the resident phi or psi buffer when the caller
        names it, else `var_grid` uploaded into a buffer the grid keeps (the theta grid of the volatility)"""
        if resident == "phi":
            return self.phi.ptr
        if resident == "psi":
            return self.psi.ptr
        if self._var is None or self._var.n < 2 * var_grid.size:
            if self._var is not None:
                self._var.free()
            self._var = DeviceBuffer(2 * var_grid.size)
        _lib.check(self.lib.svmc_memcpy_h2d(self._var.ptr, var_grid.ctypes.data, var_grid.nbytes, None))
        return self._var.ptr

    def pdf_sums(self, var_grid: np.ndarray, space_grid: np.ndarray, shift: float = 0.0, scale: float = 1.0,
                 is_simpson: bool = True, resident: Optional[str] = None) -> np.ndarray:
        """pdf_with_mgf_grid (reference utils/mgf_pricer.py:361-384) from the log-MGF resident on the device
        (svmc_mgf_pdf_slice_batch at one set).  `var_grid` is the transform variable the density is inverted over;
        resident="phi" / "psi" says it IS the grid's phi / psi buffer, otherwise it is uploaded (the theta grid of the
        volatility).  The space grid and the masses go through the grid's pooled result buffer.  In the same wait the log-MGF
        comes back and self.last_given_up is counted (download_results)."""
        var_grid = np.ascontiguousarray(var_grid, dtype=np.complex128).ravel()
        space = np.ascontiguousarray(space_grid, dtype=np.float64).ravel()
        assert var_grid.size == self.n
        k = space.size
        self.reserve_results(2 * k)                                    # [space | masses]
        var_ptr = self._var_ptr(var_grid, resident)
        _lib.check(self.lib.svmc_memcpy_h2d(self._capped.ptr, space.ctypes.data, space.nbytes, None))
        pf = C.POINTER(C.c_double)
        sh, sc = np.array([float(shift)]), np.array([float(scale)])
        _lib.check(self.lib.svmc_mgf_pdf_slice_batch(var_ptr, self.log_mgf.ptr, self.n, 1, self._capped.ptr, k,
                                                     sh.ctypes.data_as(pf), sc.ctypes.data_as(pf), int(bool(is_simpson)),
                                                     self._capped.offset(k), None))
        out = np.empty(k)
        lm = np.empty(self.n, dtype=np.complex128)
        if k:
            _lib.check(self.lib.svmc_memcpy_d2h(out.ctypes.data, self._capped.offset(k), out.nbytes, None))
        _lib.check(self.lib.svmc_memcpy_d2h(lm.ctypes.data, self.log_mgf.ptr, lm.nbytes, None))
        _lib.check(self.lib.svmc_stream_synchronize(None))
        self.last_given_up = int(np.count_nonzero(np.isnan(lm.real) | np.isnan(lm.imag)))
        return out

    def qvar_sums(self, ttm: float, strikes: np.ndarray) -> np.ndarray:
        strikes = np.ascontiguousarray(strikes, dtype=np.float64)
        k = strikes.size
        if self._capped is None or self._capped.n < k:
            self._capped = DeviceBuffer(max(k, 32))
        _lib.check(self.lib.svmc_mgf_qvar_slice(self.psi.ptr, self.log_mgf.ptr, self.n, float(ttm),
                                                strikes.ctypes.data_as(C.POINTER(C.c_double)), k, self._capped.ptr, None))
        out = np.empty(k)
        _lib.check(self.lib.svmc_memcpy_d2h(out.ctypes.data, self._capped.ptr, 8 * k, None))
        _lib.check(self.lib.svmc_stream_synchronize(None))
        return out

    def close(self) -> None:
        for b in (self.phi, self.psi, self.a, self.b, self.log_mgf, self._capped, self._var):
            if b is not None:
                b.free()


class AnalyticGridBatch(_Pooled):
    """the transform grids of SEVERAL LogSV or Hawkes parameter sets resident on the device, advanced expiry by expiry in one
    launch per expiry (svmc_logsv_mgf_grid_batch, svmc_hawkesjd_mgf_grid_batch) and inverted in one launch per expiry
    (svmc_mgf_vanilla_slice_batch, or svmc_mgf_gamma_slice_batch under the Hawkes risk-premia kernel):
    config C5's five sets, or the bumped parameter vectors of a finite-difference gradient, side by side.  Bit-identical
    to one AnalyticGrid per set."""

    @staticmethod
    def _pool_key(phis, psis, n_coef):
        return (len(phis), int(np.asarray(phis[0]).size), int(n_coef))

    def _reset(self, phis, psis, n_coef) -> None:
        phi = np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.complex128) for p in phis]))
        psi = np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.complex128) for p in psis]))
        for buf, z, name in ((self.phi, phi, "phi_host"), (self.psi, psi, "psi_host")):
            if not np.array_equal(z, getattr(self, name)):
                _lib.check(self.lib.svmc_memcpy_h2d(buf.ptr, z.ctypes.data, z.nbytes, None))
                setattr(self, name, z)
        _lib.check(self.lib.svmc_stream_synchronize(None))
        _lib.check(self.lib.svmc_memset(self.a.ptr, 0, self.a.nbytes, None))

    def __init__(self, phis: Sequence[np.ndarray], psis: Sequence[np.ndarray], n_coef: int):
        self.lib = _lib.load()
        self.n_sets = len(phis)
        self.n = int(np.asarray(phis[0]).size)
        self.n_coef = int(n_coef)
        phi = np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.complex128) for p in phis]))       # np.stack copies: private
        psi = np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.complex128) for p in psis]))
        assert phi.shape == psi.shape == (self.n_sets, self.n)
        self.last_given_up = np.zeros(self.n_sets, dtype=int)
        self.phi_host, self.psi_host = phi, psi
        self.phi, self.psi = DeviceBuffer(2 * phi.size), DeviceBuffer(2 * psi.size)
        for buf, z in ((self.phi, phi), (self.psi, psi)):
            _lib.check(self.lib.svmc_memcpy_h2d(buf.ptr, z.ctypes.data, z.nbytes, None))
        _lib.check(self.lib.svmc_stream_synchronize(None))
        self.a = DeviceBuffer(2 * self.n_sets * self.n * self.n_coef)
        self.log_mgf = DeviceBuffer(2 * self.n_sets * self.n)
        _lib.check(self.lib.svmc_memset(self.a.ptr, 0, self.a.nbytes, None))
        self._capped: Optional[DeviceBuffer] = None
        self._risk: Optional[DeviceBuffer] = None            # normalizers then gamma forwards, [n_ttms][n_sets] each
        self._var: Optional[DeviceBuffer] = None             # a transform variable other than phi / psi (pdf_sums)
        self._risk_ttms = 0

    def logsv_advance(self, ttm: float, params_rows: np.ndarray, is_spot_measure: bool, expansion_order: int,
                      rtol: Optional[float] = None, atol: Optional[float] = None) -> None:
        """params_rows [n_sets][8] = (sigma0, theta, kappa1, kappa2, beta, volvol, vol_backbone_eta, 0)"""
        rows = np.ascontiguousarray(params_rows, dtype=np.float64)
        assert rows.shape == (self.n_sets, 8)
        _lib.check(self.lib.svmc_logsv_mgf_grid_batch(self.phi.ptr, self.psi.ptr, self.n, self.n_sets, float(ttm),
                                                      rows.ctypes.data_as(C.POINTER(C.c_double)), int(bool(is_spot_measure)),
                                                      int(expansion_order), self.a.ptr, self.log_mgf.ptr,
                                                      ODE_RTOL if rtol is None else float(rtol),
                                                      ODE_ATOL if atol is None else float(atol), None))

    def hawkes_advance(self, ttm: float, params_rows: np.ndarray, rtol: Optional[float] = None,
                       atol: Optional[float] = None) -> None:
        """params_rows [n_sets][16]: the Hawkes jump-diffusion parameter blocks (include/svmc.h SVMC_HAWKESJD_PARAMS order)"""
        rows = np.ascontiguousarray(params_rows, dtype=np.float64)
        assert rows.shape == (self.n_sets, 16) and self.n_coef == 3
        _lib.check(self.lib.svmc_hawkesjd_mgf_grid_batch(self.phi.ptr, self.psi.ptr, self.n, self.n_sets, float(ttm),
                                                         rows.ctypes.data_as(C.POINTER(C.c_double)), self.a.ptr,
                                                         self.log_mgf.ptr, ODE_RTOL if rtol is None else float(rtol),
                                                         ODE_ATOL if atol is None else float(atol), None))

    def risk_forwards(self, params_rows: np.ndarray, gammas: np.ndarray, ttms: np.ndarray, forwards: np.ndarray,
                      rtol: Optional[float] = None, atol: Optional[float] = None) -> None:
        """queue the risk-premia normalizers and gamma forwards of every set and expiry (svmc_hawkesjd_risk_forwards_batch)
        into the batch's device buffer, where queue_gamma_slice reads them; download_risk_results brings them back"""
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

    def download_risk_results(self, n_doubles: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(queued prices, normalizers [n_ttms][n_sets], gamma forwards [n_ttms][n_sets]) in one wait; last_given_up as in
        download_results"""
        n = self._risk_ttms * self.n_sets
        risk = np.empty(2 * n)
        if n:
            _lib.check(self.lib.svmc_memcpy_d2h(risk.ctypes.data, self._risk.ptr, risk.nbytes, None))
        out = self.download_results(n_doubles)
        return out, risk[:n].reshape(self._risk_ttms, self.n_sets), risk[n:].reshape(self._risk_ttms, self.n_sets)

    def capped_sums(self, forward: float, strikes: np.ndarray) -> np.ndarray:
        """-> [n_sets][n_strikes]"""
        strikes = np.ascontiguousarray(strikes, dtype=np.float64)
        k = strikes.size
        if self._capped is None or self._capped.n < k * self.n_sets:
            self._capped = DeviceBuffer(max(k * self.n_sets, 32))
        _lib.check(self.lib.svmc_mgf_vanilla_slice_batch(self.phi.ptr, self.log_mgf.ptr, self.n, self.n_sets, float(forward),
                                                         strikes.ctypes.data_as(C.POINTER(C.c_double)), k, self._capped.ptr,
                                                         None))
        out = np.empty((self.n_sets, k))
        _lib.check(self.lib.svmc_memcpy_d2h(out.ctypes.data, self._capped.ptr, out.nbytes, None))
        _lib.check(self.lib.svmc_stream_synchronize(None))
        return out

    def set_a(self, a_t0: np.ndarray) -> None:
        """A(0) of every set, [n_sets][n_grid][n_coef] (zeros after acquire(); -Theta in the 2nd slot for the volatility)"""
        a_t0 = np.ascontiguousarray(a_t0, dtype=np.complex128)
        assert a_t0.shape == (self.n_sets, self.n, self.n_coef)
        _lib.check(self.lib.svmc_memcpy_h2d(self.a.ptr, a_t0.ctypes.data, a_t0.nbytes, None))
        _lib.check(self.lib.svmc_stream_synchronize(None))

    def pdf_sums(self, var_grids: Sequence[np.ndarray], space_grids: Sequence[np.ndarray], shifts: Sequence[float],
                 scales: Sequence[float], is_simpson: bool = True, resident: Optional[str] = None) -> np.ndarray:
        """AnalyticGrid.pdf_sums for every set in ONE launch -> [n_sets][n_space]; each set has its own transform grid, space
        grid (of one common length), shift and scale.  self.last_given_up is counted per set in the same wait."""
        var = np.ascontiguousarray(np.stack([np.asarray(v, dtype=np.complex128).ravel() for v in var_grids]))
        space = np.ascontiguousarray(np.stack([np.asarray(s, dtype=np.float64).ravel() for s in space_grids]))
        sh, sc = np.ascontiguousarray(shifts, dtype=np.float64), np.ascontiguousarray(scales, dtype=np.float64)
        assert var.shape == (self.n_sets, self.n) and space.shape[0] == self.n_sets and sh.shape == sc.shape == (self.n_sets,)
        k = space.size
        self.reserve_results(2 * k)                                    # [spaces | masses]
        var_ptr = AnalyticGrid._var_ptr(self, var, resident)
        _lib.check(self.lib.svmc_memcpy_h2d(self._capped.ptr, space.ctypes.data, space.nbytes, None))
        pf = C.POINTER(C.c_double)
        _lib.check(self.lib.svmc_mgf_pdf_slice_batch(var_ptr, self.log_mgf.ptr, self.n, self.n_sets, self._capped.ptr,
                                                     space.shape[1], sh.ctypes.data_as(pf), sc.ctypes.data_as(pf),
                                                     int(bool(is_simpson)), self._capped.offset(k), None))
        out = np.empty(space.shape)
        lm = np.empty((self.n_sets, self.n), dtype=np.complex128)
        if k:
            _lib.check(self.lib.svmc_memcpy_d2h(out.ctypes.data, self._capped.offset(k), out.nbytes, None))
        _lib.check(self.lib.svmc_memcpy_d2h(lm.ctypes.data, self.log_mgf.ptr, lm.nbytes, None))
        _lib.check(self.lib.svmc_stream_synchronize(None))
        self.last_given_up = np.count_nonzero(np.isnan(lm.real) | np.isnan(lm.imag), axis=1).astype(int)
        return out

    def reserve_results(self, n_doubles: int) -> None:
        if self._capped is None or self._capped.n < n_doubles:
            if self._capped is not None:
                self._capped.free()
            self._capped = DeviceBuffer(max(int(n_doubles), 32))

    def queue_capped_sums(self, forward: float, strikes: np.ndarray, offset: int) -> None:
        """the [n_sets][n_strikes] sums of one expiry, queued into the result buffer at `offset` (AnalyticGrid.queue_capped_sums)"""
        strikes = np.ascontiguousarray(strikes, dtype=np.float64)
        _lib.check(self.lib.svmc_mgf_vanilla_slice_batch(self.phi.ptr, self.log_mgf.ptr, self.n, self.n_sets, float(forward),
                                                         strikes.ctypes.data_as(C.POINTER(C.c_double)), strikes.size,
                                                         self._capped.offset(offset), None))

    def download_results(self, n_doubles: int) -> np.ndarray:
        """as AnalyticGrid.download_results; self.last_given_up is an array, one count per parameter set"""
        out = np.empty(int(n_doubles))
        lm = np.empty((self.n_sets, self.n), dtype=np.complex128)
        _lib.check(self.lib.svmc_memcpy_d2h(out.ctypes.data, self._capped.ptr, 8 * int(n_doubles), None))
        _lib.check(self.lib.svmc_memcpy_d2h(lm.ctypes.data, self.log_mgf.ptr, lm.nbytes, None))
        _lib.check(self.lib.svmc_stream_synchronize(None))
        self.last_given_up = np.count_nonzero(np.isnan(lm.real) | np.isnan(lm.imag), axis=1).astype(int)
        return out

    def close(self) -> None:
        for b in (self.phi, self.psi, self.a, self.log_mgf, self._capped, self._risk, self._var):
            if b is not None:
                b.free()


def gamma_slice_prices(phi: np.ndarray, log_mgf: np.ndarray, gamma: float, shortcut: bool, normalizer: float,
                       gamma_forward: float, forward: float, strikes: np.ndarray, type_codes: np.ndarray) -> np.ndarray:
    """one slice under the risk-premia kernel from a given log-MGF (svmc_mgf_gamma_slice_batch at one set): uploads the grid,
    the log-MGF and the slice's normalizer / gamma forward, returns the undiscounted prices"""
    lib = _lib.load()
    phi = np.ascontiguousarray(phi, dtype=np.complex128)
    log_mgf = np.ascontiguousarray(log_mgf, dtype=np.complex128)
    strikes = np.ascontiguousarray(strikes, dtype=np.float64)
    codes = np.ascontiguousarray(type_codes, dtype=np.int32)
    nf = np.array([normalizer, gamma_forward], dtype=np.float64)
    gammas, short = np.array([gamma], dtype=np.float64), np.array([int(bool(shortcut))], dtype=np.int32)
    bufs = [DeviceBuffer(2 * phi.size), DeviceBuffer(2 * log_mgf.size), DeviceBuffer(2), DeviceBuffer(max(strikes.size, 1))]
    try:
        for buf, z in zip(bufs[:3], (phi, log_mgf, nf)):
            _lib.check(lib.svmc_memcpy_h2d(buf.ptr, z.ctypes.data, z.nbytes, None))
        pf, pi = C.POINTER(C.c_double), C.POINTER(C.c_int)
        _lib.check(lib.svmc_mgf_gamma_slice_batch(bufs[0].ptr, bufs[1].ptr, phi.size, 1, gammas.ctypes.data_as(pf),
                                                  short.ctypes.data_as(pi), bufs[2].ptr, bufs[2].offset(1), 0, float(forward),
                                                  strikes.ctypes.data_as(pf), codes.ctypes.data_as(pi), strikes.size,
                                                  bufs[3].ptr, None))
        out = np.empty(strikes.size)
        _lib.check(lib.svmc_memcpy_d2h(out.ctypes.data, bufs[3].ptr, out.nbytes, None))
        _lib.check(lib.svmc_stream_synchronize(None))
        return out
    finally:
        for b in bufs:
            b.free()


def pdf_slices(var_grids: np.ndarray, log_mgfs: np.ndarray, space_grids: np.ndarray, shifts, scales,
               is_simpson: bool = True) -> np.ndarray:
    """pdf_with_mgf_grid for [n_sets] given log-MGFs in one launch (svmc_mgf_pdf_slice_batch): var_grids, log_mgfs
    [n_sets][n_grid] complex, space_grids [n_sets][n_space], shifts / scales [n_sets] -> [n_sets][n_space].  Uploads its
    inputs; the pricers keep the log-MGF on the device instead (AnalyticGrid.pdf_sums)."""
    lib = _lib.load()
    var = np.ascontiguousarray(var_grids, dtype=np.complex128)
    lm = np.ascontiguousarray(log_mgfs, dtype=np.complex128)
    space = np.ascontiguousarray(space_grids, dtype=np.float64)
    sh, sc = np.ascontiguousarray(shifts, dtype=np.float64), np.ascontiguousarray(scales, dtype=np.float64)
    if not (var.ndim == 2 and var.shape == lm.shape and space.ndim == 2 and space.shape[0] == var.shape[0]
            and sh.shape == sc.shape == (var.shape[0],)):
        raise ValueError("pdf_slices: var_grids / log_mgfs [n_sets][n_grid], space_grids [n_sets][n_space], shifts / scales [n_sets]")
    bufs = [DeviceBuffer(2 * var.size), DeviceBuffer(2 * lm.size), DeviceBuffer(max(space.size, 1)), DeviceBuffer(max(space.size, 1))]
    try:
        for buf, z in zip(bufs[:3], (var, lm, space)):
            _lib.check(lib.svmc_memcpy_h2d(buf.ptr, z.ctypes.data, z.nbytes, None))
        pf = C.POINTER(C.c_double)
        _lib.check(lib.svmc_mgf_pdf_slice_batch(bufs[0].ptr, bufs[1].ptr, var.shape[1], var.shape[0], bufs[2].ptr, space.shape[1],
                                                sh.ctypes.data_as(pf), sc.ctypes.data_as(pf), int(bool(is_simpson)), bufs[3].ptr,
                                                None))
        out = np.empty(space.shape)
        if out.size:
            _lib.check(lib.svmc_memcpy_d2h(out.ctypes.data, bufs[3].ptr, out.nbytes, None))
        _lib.check(lib.svmc_stream_synchronize(None))
        return out
    finally:
        for b in bufs:
            b.free()


def digital_slice_sums(phis: np.ndarray, log_mgfs: np.ndarray, forward: float, strikes: np.ndarray, negative_contour: bool,
                       is_simpson: bool = True) -> np.ndarray:
    """the strike sums of digital_slice_pricer_with_mgf_grid for [n_sets] given log-MGFs in one launch
    (svmc_mgf_digital_slice_batch) -> [n_sets][n_strikes]"""
    lib = _lib.load()
    phi = np.ascontiguousarray(phis, dtype=np.complex128)
    lm = np.ascontiguousarray(log_mgfs, dtype=np.complex128)
    strikes = np.ascontiguousarray(strikes, dtype=np.float64).ravel()
    if not (phi.ndim == 2 and phi.shape == lm.shape):
        raise ValueError("digital_slice_sums: phis / log_mgfs [n_sets][n_grid]")
    bufs = [DeviceBuffer(2 * phi.size), DeviceBuffer(2 * lm.size), DeviceBuffer(max(strikes.size * phi.shape[0], 1))]
    try:
        for buf, z in zip(bufs[:2], (phi, lm)):
            _lib.check(lib.svmc_memcpy_h2d(buf.ptr, z.ctypes.data, z.nbytes, None))
        _lib.check(lib.svmc_mgf_digital_slice_batch(bufs[0].ptr, bufs[1].ptr, phi.shape[1], phi.shape[0], float(forward),
                                                    strikes.ctypes.data_as(C.POINTER(C.c_double)), strikes.size,
                                                    int(bool(negative_contour)), int(bool(is_simpson)), bufs[2].ptr, None))
        out = np.empty((phi.shape[0], strikes.size))
        if out.size:
            _lib.check(lib.svmc_memcpy_d2h(out.ctypes.data, bufs[2].ptr, out.nbytes, None))
        _lib.check(lib.svmc_stream_synchronize(None))
        return out
    finally:
        for b in bufs:
            b.free()


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
