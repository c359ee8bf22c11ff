"""
HipEngine: the host-side owner of one GPU's Monte Carlo state and the thin caller of libsvmc's kernels.

One engine = one HIP device + one stream + the resident per-path state (x, vol, qvar) of `n_path` local
paths, the per-expiry snapshots the payoff pass reads, and the reduction scratch.  State never leaves
HBM between expiries (the reference carries it slice to slice in NumPy arrays,
pricers/logsv_pricer.py:843-856).

The chain drivers in mc_chain.py talk to an engine only through the methods below, so the sharding /
collective logic can be exercised on CPU by a test double (tests/ only); the product always uses this
class and fails loudly when libsvmc.so or a GPU is missing.
"""
from __future__ import annotations

import ctypes as C
import functools
import sys
import threading
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .utils.funcs import chain_step_grid

LOG_RETURN, Q_VAR, SIGMA = 1, 2, 3
HESTON_EULER_FLOOR, HESTON_QE = 0, 1
_TYPE_CODES = {"C": 0, "P": 1, "IC": 2, "IP": 3}


_DP = C.POINTER(C.c_double)
_POINTERS = {np.dtype(t): C.POINTER(c) for t, c in ((np.float64, C.c_double), (np.int8, C.c_int8), (np.int32, C.c_int),
                                                    (np.uint32, C.c_uint32), (np.uint64, C.c_uint64))}


def ptr(a: np.ndarray):
    """the C pointer of a contiguous array, typed by the array's dtype; the pointer keeps the array alive"""
    return a.ctypes.data_as(_POINTERS[a.dtype])


def row_ptr(res: np.ndarray, r: int):
    """the C pointer of row r (along the first axis) of a C-contiguous float64 result block"""
    return C.cast(res.ctypes.data + r * res.strides[0], _DP)


def _flag(v) -> int:
    """a truth value as the C int the ABI takes"""
    return int(bool(v))


def expiry_rows(res: np.ndarray, slices: Sequence[slice]) -> tuple:
    """a result block [R][K] cut into expiries: per row the list of its per-expiry views"""
    return tuple([row[sl] for sl in slices] for row in res)


def expiry_rows_per_job(res: np.ndarray, slices: Sequence[slice]) -> list:
    """a result block [R][J][K] of J jobs (or parameter sets): per job what expiry_rows gives for its [R][K]"""
    return [expiry_rows(res[:, j], slices) for j in range(res.shape[1])]


def chain_etas(etas, m: int) -> np.ndarray:
    """the vol-backbone etas of a LogSV chain of m expiries as a contiguous float64 vector"""
    etas = np.ascontiguousarray(etas, dtype=np.float64).ravel()
    if etas.size != m:
        raise ValueError("vol_backbone_etas must have one entry per maturity")
    return etas


_CODES_CACHE = {}           # (dtype, bytes) of a NumPy array of option types -> its int8 codes (read-only)


def option_type_codes(optiontypes: Sequence) -> np.ndarray:
    """'C','P','IC','IP' -> int8; anything else raises like utils/mc_payoffs.py:84.  The codes of a NumPy array are kept
    (a calibration asks for the same few arrays at every objective evaluation) and come back read-only."""
    key = None
    if isinstance(optiontypes, np.ndarray) and optiontypes.dtype.kind == "U" and optiontypes.size <= 4096:
        key = (optiontypes.dtype.str, optiontypes.shape, optiontypes.tobytes())
        hit = _CODES_CACHE.get(key)
        if hit is not None:
            return hit
        if optiontypes.ndim != 1:
            out = option_type_codes(optiontypes.ravel()).reshape(optiontypes.shape)
            out.flags.writeable = False
            _CODES_CACHE[key] = out
            return out
    out = np.empty(len(optiontypes), dtype=np.int8)
    for i, t in enumerate(optiontypes):
        code = _TYPE_CODES.get(str(t))
        if code is None:
            raise ValueError("unknown option payoff code")
        out[i] = code
    if key is not None:
        if len(_CODES_CACHE) > 256:
            _CODES_CACHE.clear()
        out.flags.writeable = False
        _CODES_CACHE[key] = out
    return out


def payoff_shifts(strikes: np.ndarray, codes: np.ndarray, forward: float, variable_type: int) -> np.ndarray:
    """per-strike constants subtracted inside the payoff sums (include/svmc.h): the intrinsic value at the
    forward for LOG_RETURN (the recentred spots average to the forward exactly), zero otherwise."""
    shifts = np.zeros(len(strikes), dtype=np.float64)
    if variable_type == LOG_RETURN:
        call = (codes == 0) | (codes == 2)
        intrinsic = np.where(call, np.maximum(forward - strikes, 0.0), np.maximum(strikes - forward, 0.0))
        shifts = np.where(codes >= 2, intrinsic / forward, intrinsic).astype(np.float64)
    return np.ascontiguousarray(shifts)


class DeviceBuffer:
    """a caller-owned HBM allocation of `n` doubles (svmc_malloc / svmc_free)."""

    def __init__(self, n: int):
        self.n = int(n)
        self.nbytes = 8 * self.n
        p = C.c_void_p()
        _lib.check(_lib.load().svmc_malloc(C.byref(p), self.nbytes))
        self.ptr = p.value

    def free(self) -> None:
        if getattr(self, "ptr", None):
            _lib.load().svmc_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def offset(self, n_doubles: int) -> int:
        return self.ptr + 8 * int(n_doubles)


# ---- bulk results: resident, or brought to the host at the PCIe rate ---------------------------------------------------
# hipMemcpy into a pageable NumPy array goes through the runtime's small staging buffers on one host thread; an 8.6 GB
# result (simulate_vol_paths at 2^20 x 1024) then takes far longer to fetch than the 2 ms it took to compute.  A bulk
# download here is a pipeline: the device-to-host copies run back to back, asynchronously, into a ring of page-locked
# buffers the process keeps, and a few host threads move each finished chunk into the destination array while the next
# chunks are in flight (NumPy releases the GIL while it copies) -- the GPU link and the host's memory system both stay busy.
import os as _os
PIPELINE_CHUNK_BYTES = int(_os.environ.get("SVMC_PIPELINE_CHUNK_MIB", "32")) << 20
PIPELINE_SLOTS = int(_os.environ.get("SVMC_PIPELINE_SLOTS", "8"))
PIPELINE_THREADS = int(_os.environ.get("SVMC_PIPELINE_THREADS", "6"))        # swept in profiles/r05_pipeline_sweep.jsonl
PIPELINE_MIN_BYTES = 8 << 20                   # below this a plain copy is as fast
_pinned_ring = {"ptr": None, "slots": 0, "chunk": 0, "lock": threading.Lock()}
_copy_pool = None


def _ring(lib):
    r = _pinned_ring
    if r["ptr"] is None:
        buf = C.c_void_p()
        _lib.check(lib.svmc_host_alloc(C.byref(buf), PIPELINE_SLOTS * PIPELINE_CHUNK_BYTES))
        r["ptr"], r["slots"], r["chunk"] = buf.value, PIPELINE_SLOTS, PIPELINE_CHUNK_BYTES
    return r


def pipelined_download(src_ptr: int, n_doubles: int, stream=None, out: Optional[np.ndarray] = None) -> np.ndarray:
    """n_doubles from device memory into `out` (a C-contiguous float64 array; a new one when None) through the pinned ring"""
    global _copy_pool
    lib = _lib.load()
    n = int(n_doubles)
    if out is None:
        out = np.empty(n, dtype=np.float64)
    flat = out.reshape(-1)
    if flat.size != n or flat.dtype != np.float64 or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous float64 array of the result's size")
    if 8 * n < PIPELINE_MIN_BYTES:
        _lib.check(lib.svmc_memcpy_d2h(flat.ctypes.data, src_ptr, 8 * n, stream))
        _lib.check(lib.svmc_stream_synchronize(stream))
        return out
    from concurrent.futures import ThreadPoolExecutor
    with _pinned_ring["lock"]:                     # one bulk download at a time per process: the ring is shared
        ring = _ring(lib)
        if _copy_pool is None:
            _copy_pool = ThreadPoolExecutor(max_workers=PIPELINE_THREADS, thread_name_prefix="svmc-d2h")
        per = ring["chunk"] // 8
        events, pending = [], [None] * ring["slots"]
        for _ in range(ring["slots"]):
            e = C.c_void_p()
            _lib.check(lib.svmc_event_create(C.byref(e)))
            events.append(e)

        def drain(slot, lo, cnt):
            _lib.check(lib.svmc_event_synchronize(events[slot]))
            view = np.ctypeslib.as_array(C.cast(ring["ptr"] + slot * ring["chunk"], C.POINTER(C.c_double)), shape=(cnt,))
            np.copyto(flat[lo:lo + cnt], view)

        try:
            for i, lo in enumerate(range(0, n, per)):
                slot, cnt = i % ring["slots"], min(per, n - lo)
                if pending[slot] is not None:
                    pending[slot].result()         # the slot's previous chunk has left the ring
                _lib.check(lib.svmc_memcpy_d2h(ring["ptr"] + slot * ring["chunk"], src_ptr + 8 * lo, 8 * cnt, stream))
                _lib.check(lib.svmc_event_record(events[slot], stream))
                pending[slot] = _copy_pool.submit(drain, slot, lo, cnt)
            for f in pending:
                if f is not None:
                    f.result()
        finally:
            # an exception inside the loop (a failed copy, a failed drain) must not destroy the events while drain tasks still
            # wait on them: every submitted task is waited for first, its own error swallowed -- the first one is already rising
            for f in pending:
                if f is not None:
                    try:
                        f.result()
                    except Exception:               # noqa: BLE001
                        pass
            for e in events:
                lib.svmc_event_destroy(e)
    return out


class DeviceArray:
    """a float64 [rows][cols] result left RESIDENT in HBM (simulate_vol_paths(..., return_device=True)): nothing crosses
    PCIe until asked.  Consumers: torch / cupy take it zero-copy (`torch.as_tensor(a, device="cuda")` through
    __cuda_array_interface__, `torch.from_dlpack(a)` through __dlpack__); `row_moments` / `expanding_mean_of_squares` do on
    the device what the reference's callers do with the host array; `numpy()` fetches it through the pinned pipeline."""

    def __init__(self, buf: DeviceBuffer, shape: Tuple[int, int], stream=None, device: int = 0, owns: bool = True, scratch=None):
        self._buf, self.shape, self.stream, self.device = buf, (int(shape[0]), int(shape[1])), stream, int(device)
        self.dtype = np.dtype(np.float64)
        self._owns = bool(owns)                    # False: a view of an engine's cached bulk buffer (free() leaves the buffer alone)
        self._scratch = scratch                    # callable(n_doubles, slot) -> DeviceBuffer for temporaries (the engine's cache)

    @property
    def ptr(self) -> int:
        if self._buf is None or self._buf.ptr is None:
            raise _lib.SvmcError("this DeviceArray was freed")
        return self._buf.ptr

    @property
    def nbytes(self) -> int:
        return 8 * self.shape[0] * self.shape[1]

    def synchronize(self) -> None:
        _lib.check(_lib.load().svmc_stream_synchronize(self.stream))

    def numpy(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        res = pipelined_download(self.ptr, self.shape[0] * self.shape[1], self.stream, None if out is None else out)
        return res.reshape(self.shape)

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a if dtype is None else a.astype(dtype, copy=False)

    @property
    def __cuda_array_interface__(self):
        self.synchronize()
        return {"shape": self.shape, "typestr": "<f8", "data": (self.ptr, False), "version": 3, "strides": None}

    def __dlpack_device__(self):
        return (10, self.device)                   # kDLROCM

    def __dlpack__(self, stream=None, **_unused):
        self.synchronize()
        return _dlpack_capsule(self)

    def row_moments(self, center: float = 0.0, n_moments: int = 4) -> Tuple[np.ndarray, np.ndarray]:
        """(mean, std) over the paths, per row, of (a - center)^k for k = 1 .. n_moments: arrays [rows][n_moments];
        std is the population standard deviation (np.std): what moments_vol_qvar.py:48 computes from the host array"""
        lib = _lib.load()
        rows, cols = self.shape
        k2 = 2 * int(n_moments)
        if not 1 <= int(n_moments) <= 4:
            raise ValueError("n_moments must be 1 .. 4")
        sums, ws = DeviceBuffer(rows * k2), DeviceBuffer(rows * 4 * k2)
        try:
            _lib.check(lib.svmc_row_power_sums(self.ptr, cols, rows, cols, float(center), int(n_moments), sums.ptr, ws.ptr,
                                               ws.nbytes, self.stream))
            host = np.empty(rows * k2)
            _lib.check(lib.svmc_memcpy_d2h(host.ctypes.data, sums.ptr, host.nbytes, self.stream))
            self.synchronize()
        finally:
            sums.free()
            ws.free()
        s = host.reshape(k2, rows) / float(cols)               # s[j] = E[d^(j+1)]
        mean = np.stack([s[k] for k in range(n_moments)], axis=1)
        var = np.stack([s[2 * k + 1] - np.square(s[k]) for k in range(n_moments)], axis=1)
        return mean, np.sqrt(np.maximum(var, 0.0))

    def expanding_mean_of_squares(self) -> "DeviceArray":
        """a new resident array q[t][p] = mean of a[u][p]^2 over u <= t (moments_vol_qvar.py:102: the realised variance so far)"""
        rows, cols = self.shape
        if self._scratch is not None:              # a view of an engine's cache: the result lives in the engine's second bulk slot
            out, owns = self._scratch(rows * cols, 1), False
        else:
            out, owns = DeviceBuffer(rows * cols), True
        _lib.check(_lib.load().svmc_expanding_mean_squares(self.ptr, cols, rows, cols, out.ptr, cols, self.stream))
        return DeviceArray(out, self.shape, self.stream, self.device, owns=owns)

    def free(self) -> None:
        if self._buf is not None:
            self.synchronize()
            if self._owns:
                self._buf.free()
            self._buf = None


def _dlpack_capsule(arr: "DeviceArray"):
    """a DLPack capsule ("dltensor") of a DeviceArray: kDLROCM, float64, 2-d, compact strides; the capsule keeps the array
    alive until the consumer's deleter runs"""
    class DLDevice(C.Structure):
        _fields_ = [("device_type", C.c_int), ("device_id", C.c_int)]

    class DLDataType(C.Structure):
        _fields_ = [("code", C.c_uint8), ("bits", C.c_uint8), ("lanes", C.c_uint16)]

    class DLTensor(C.Structure):
        _fields_ = [("data", C.c_void_p), ("device", DLDevice), ("ndim", C.c_int), ("dtype", DLDataType),
                    ("shape", C.POINTER(C.c_int64)), ("strides", C.POINTER(C.c_int64)), ("byte_offset", C.c_uint64)]

    class DLManagedTensor(C.Structure):
        pass
    DELETER = C.CFUNCTYPE(None, C.POINTER(DLManagedTensor))
    DLManagedTensor._fields_ = [("dl_tensor", DLTensor), ("manager_ctx", C.c_void_p), ("deleter", DELETER)]
    shape = (C.c_int64 * 2)(*arr.shape)
    m = DLManagedTensor()
    m.dl_tensor = DLTensor(arr.ptr, DLDevice(10, arr.device), 2, DLDataType(2, 64, 1), shape, None, 0)
    key = id(m)

    @DELETER
    def deleter(_p):
        # called by the consumer THROUGH the ctypes thunk `deleter` itself, with `m` as its argument: dropping the last reference
        # to either from in here would free memory libffi / ctypes still read after this function returns.  The array (the HBM)
        # goes now; the thunk, the tensor struct and its shape retire and are released two capsule creations later
        kept = _DLPACK_ALIVE.pop(key, None)
        if kept is not None:
            _DLPACK_RETIRED[-1].append(kept[:3])
    m.deleter = deleter
    _DLPACK_RETIRED.append([])                             # a new generation; the one before the previous is let go
    del _DLPACK_RETIRED[:-2]
    _DLPACK_ALIVE[key] = (m, shape, deleter, arr)          # owner of everything the consumer may touch
    C.pythonapi.PyCapsule_New.restype = C.py_object
    C.pythonapi.PyCapsule_New.argtypes = [C.c_void_p, C.c_char_p, _CAPSULE_DESTRUCTOR]
    return C.pythonapi.PyCapsule_New(C.addressof(m), b"dltensor", _drop_unconsumed_capsule)


_DLPACK_ALIVE = {}
_DLPACK_RETIRED = [[]]         # generations of (tensor struct, shape, deleter thunk) whose deleter has run (see _dlpack_capsule)
_CAPSULE_DESTRUCTOR = C.CFUNCTYPE(None, C.c_void_p)


@_CAPSULE_DESTRUCTOR
def _drop_unconsumed_capsule(capsule):
    """a capsule nobody consumed (still named "dltensor" when it dies) releases what it kept alive; a consumed one was renamed
    "used_dltensor" and its consumer calls the tensor's deleter"""
    C.pythonapi.PyCapsule_IsValid.restype = C.c_int
    C.pythonapi.PyCapsule_IsValid.argtypes = [C.c_void_p, C.c_char_p]
    if C.pythonapi.PyCapsule_IsValid(capsule, b"dltensor"):
        C.pythonapi.PyCapsule_GetPointer.restype = C.c_void_p
        C.pythonapi.PyCapsule_GetPointer.argtypes = [C.c_void_p, C.c_char_p]
        addr = C.pythonapi.PyCapsule_GetPointer(capsule, b"dltensor")
        for key, kept in list(_DLPACK_ALIVE.items()):
            if C.addressof(kept[0]) == addr:
                _DLPACK_ALIVE.pop(key, None)


_CHAIN_CACHE: dict = {}


def marshalled_chain(ttms, forwards, discfactors, strikes: Sequence[np.ndarray], codes: Sequence[np.ndarray]) -> dict:
    """a chain's arrays as the fused C drivers take them (private contiguous copies, their ctypes pointers, the strike offsets and
    the slices that cut a result row into expiries), kept per chain CONTENT: a pricer is called on the same chain over and over
    (a calibration, a scenario sweep), and building these arrays costs as much as the launches of a small chain"""
    strikes = [np.asarray(k, dtype=np.float64) for k in strikes]
    codes = [np.asarray(c) for c in codes]
    arrs = [np.asarray(ttms), np.asarray(forwards), np.asarray(discfactors)] + strikes + codes
    key = tuple((a.dtype.str, a.shape, a.tobytes()) for a in arrs)
    hit = _CHAIN_CACHE.get(key)
    if hit is not None:
        return hit
    m = len(strikes)
    f64 = lambda a: np.array(a, dtype=np.float64, order="C", copy=True).ravel()      # noqa: E731  (private copies)
    offs = np.concatenate([[0], np.cumsum([int(np.size(k)) for k in strikes])]).astype(np.uintp)
    total = int(offs[-1])
    t, f, d = f64(ttms), f64(forwards), f64(discfactors)
    if not (t.size == f.size == d.size == m == len(codes)):
        raise ValueError("chain arrays must have one entry per maturity")
    k_all = f64(np.concatenate([np.ravel(k) for k in strikes])) if total else np.zeros(1)
    c_all = np.array(np.concatenate([np.ravel(c) for c in codes]), dtype=np.int8) if total else np.zeros(1, dtype=np.int8)
    hit = {
        "keep": (t, f, d, k_all, c_all, offs), "total": total, "offs": offs, "m": m,
        "slices": [slice(int(offs[i]), int(offs[i + 1])) for i in range(m)],
        "ttms": ptr(t), "forwards": ptr(f), "discfactors": ptr(d), "strikes": ptr(k_all), "codes": ptr(c_all),
        "offsets": offs.ctypes.data_as(C.POINTER(C.c_size_t)),
    }
    # the C-argument run every chain entry takes (after its session): ttms, forwards, discfactors, n_expiries, strikes, types, offsets
    hit["args"] = (hit["ttms"], hit["forwards"], hit["discfactors"], m, hit["strikes"], hit["codes"], hit["offsets"])
    if len(_CHAIN_CACHE) >= 16:
        _CHAIN_CACHE.clear()
    _CHAIN_CACHE[key] = hit
    return hit


# ---- prices under the exponential risk-premia kernel (include/svmc.h, svmc_tilted_payoff_chain): host side, no library -------
TILTED_MAX_GAMMAS = 16         # SVMC_TILTED_MAX_GAMMAS
TILTED_STATS_DOUBLES = 8       # SVMC_TILTED_STATS_DOUBLES
TILTED_STATS_FIELDS = ("normalizer", "normalizer_stderr", "gamma_forward", "gamma_forward_stderr", "effective_sample_size",
                       "n_kept", "n_dropped", "sum_weights")
# the conditional estimator under the kernel (include/svmc_ext.h, svmc_tilted_cond_payoff_chain): the same block, the same meanings
TILTED_COND_STATS_FIELDS = TILTED_STATS_FIELDS
JUMP_SETS_MAX = 16             # SVMC_JUMP_SETS_MAX of include/svmc_est.h: (sigma, gamma) sets per svmc_jump_sets_payoff_chain call
# ... and its Greeks (include/svmc_est.h, svmc_tilted_cond_greeks_chain): the result rows, its own statistics block, and the block the
# routes return -- the payoff tail's with the count of cv == 0 paths
TCG_ROWS = 8                   # SVMC_TCG_ROWS
TCG_FIELDS = ("delta", "delta_stderr", "dual_delta", "dual_delta_stderr", "gamma", "gamma_stderr", "dual_gamma", "dual_gamma_stderr")
TCG_STATS_DOUBLES = 4          # SVMC_TCG_STATS_DOUBLES
TCG_STATS_FIELDS = ("sum_weights", "n_kept", "n_dropped", "n_zero_cv")
TILTED_COND_GREEKS_STATS_FIELDS = TILTED_STATS_FIELDS + ("n_zero_cv",)
# the mixture density of the log-return (include/svmc_est.h, svmc_cond_density_chain): its statistics block
CD_STATS_DOUBLES = 5           # SVMC_CD_STATS_DOUBLES
CD_STATS_FIELDS = ("sum_weights", "n_kept", "n_dropped", "n_zero_cv", "n_weight_dropped")


def cond_density_arrays(x_grids: Sequence[np.ndarray], gammas) -> dict:
    """the host arrays of a mixture-density call, checked: at least one expiry, finite points, the gammas of tilted_gammas"""
    g = tilted_gammas(gammas)
    grids = [np.asarray(x, dtype=np.float64) for x in x_grids]
    m = len(grids)
    if m < 1:
        raise ValueError("one grid of points per expiry, at least one expiry")
    offs = np.concatenate([[0], np.cumsum([x.size for x in grids])]).astype(np.uintp)
    total = int(offs[-1])
    x_all = np.ascontiguousarray(np.concatenate([x.ravel() for x in grids])) if total else np.zeros(1)
    if not np.all(np.isfinite(x_all)):
        raise ValueError("the points of a density must be finite")
    return {"m": m, "total": total, "offs": offs, "points": x_all, "gammas": g, "shapes": [x.shape for x in grids]}


def cond_density_stats_dicts(stats: np.ndarray) -> list:
    """stats [m, CD_STATS_DOUBLES] of one gamma -> one dict per expiry, keys CD_STATS_FIELDS (the four counts as ints)"""
    return [{k: (float(v) if k == "sum_weights" else int(v)) for k, v in zip(CD_STATS_FIELDS, row)} for row in stats]


# ---- conditional Monte Carlo (include/svmc.h, svmc_cmc_payoff_chain): the per-expiry statistics ----------------------------------
CMC_STATS_DOUBLES = 5          # SVMC_CMC_STATS_DOUBLES
CMC_STATS_FIELDS = ("forward_mc", "forward_mc_stderr", "corr", "n_kept", "n_dropped")


def cmc_stats_dicts(stats: np.ndarray) -> list:
    """[m][CMC_STATS_DOUBLES] -> one dict of CMC_STATS_FIELDS per expiry (the counts as ints)"""
    out = []
    for row in np.asarray(stats, dtype=np.float64).reshape(-1, CMC_STATS_DOUBLES):
        d = dict(zip(CMC_STATS_FIELDS, (float(v) for v in row)))
        d["n_kept"], d["n_dropped"] = int(d["n_kept"]), int(d["n_dropped"])
        out.append(d)
    return out


# ... and its derivatives in F and K (svmc_cmc_greeks_chain): the result rows and the statistics with the count of cv == 0 paths
CMC_GREEKS_ROWS = 10           # SVMC_CMC_GREEKS_ROWS
CMC_GREEKS_STATS_DOUBLES = 6   # SVMC_CMC_GREEKS_STATS_DOUBLES
CMC_GREEKS_FIELDS = ("price", "stderr", "delta", "delta_stderr", "dual_delta", "dual_delta_stderr", "gamma", "gamma_stderr",
                     "dual_gamma", "dual_gamma_stderr")
CMC_GREEKS_STATS_FIELDS = CMC_STATS_FIELDS + ("n_zero_cv",)
CMC_SENS_ROWS = 3              # SVMC_CMC_SENS_ROWS: sens, its error, n_pairs (row f14)
CMC_SETS_MAX = 8               # SVMC_CMC_SETS_MAX: parameter sets per svmc_*_chain_price_cmc_sets call (row f15)


def cmc_greeks_dict(res: np.ndarray, slices: Sequence[slice]) -> dict:
    """[CMC_GREEKS_ROWS][K] -> {field: [m] -> [K_i]}"""
    return {name: [res[r, sl] for sl in slices] for r, name in enumerate(CMC_GREEKS_FIELDS)}


def cmc_greeks_stats_dicts(stats: np.ndarray) -> list:
    """[m][CMC_GREEKS_STATS_DOUBLES] -> one dict of CMC_GREEKS_STATS_FIELDS per expiry (the counts as ints)"""
    out = []
    for row in np.asarray(stats, dtype=np.float64).reshape(-1, CMC_GREEKS_STATS_DOUBLES):
        d = dict(zip(CMC_GREEKS_STATS_FIELDS, (float(v) for v in row)))
        for k in ("n_kept", "n_dropped", "n_zero_cv"):
            d[k] = int(d[k])
        out.append(d)
    return out


def tilted_type_codes(optiontypes) -> np.ndarray:
    """'C' -> 0, 'P' -> 1 as int8; any other type raises ValueError("not implemented"), as the Fourier risk-premia slice pricer"""
    types = np.asarray(optiontypes).ravel()
    codes = np.empty(types.size, dtype=np.int8)
    for i, t in enumerate(types):
        t = str(t)
        if t not in ("C", "P"):
            raise ValueError("not implemented")
        codes[i] = 0 if t == "C" else 1
    return codes


def tilted_gammas(gammas) -> np.ndarray:
    """the gammas of one call as a float64 vector: 1 .. TILTED_MAX_GAMMAS finite values, else ValueError"""
    g = np.ascontiguousarray(np.atleast_1d(np.asarray(gammas, dtype=np.float64))).ravel()
    if not 1 <= g.size <= TILTED_MAX_GAMMAS:
        raise ValueError(f"between 1 and {TILTED_MAX_GAMMAS} risk-premia gammas per call, got {g.size}")
    if not np.all(np.isfinite(g)):
        raise ValueError("risk-premia gammas must be finite")
    return g


def tilted_chain_arrays(forwards, strikes: Sequence[np.ndarray], codes: Sequence[np.ndarray], gammas, ttms=None) -> dict:
    """the host arrays of a tilted call, checked: one forward (and ttm) per expiry, finite forwards and strikes, codes 0 / 1 of
    the strikes' sizes, the gammas of tilted_gammas"""
    g = tilted_gammas(gammas)
    strikes = [np.asarray(k, dtype=np.float64) for k in strikes]
    codes = [np.ascontiguousarray(np.asarray(c).ravel(), dtype=np.int8) for c in codes]
    f = np.ascontiguousarray(np.asarray(forwards, dtype=np.float64)).ravel()
    m = len(strikes)
    if not (f.size == m == len(codes)) or m < 1:
        raise ValueError("chain arrays must have one entry per maturity")
    for k, c in zip(strikes, codes):
        if k.size != c.size:
            raise ValueError("strikes and optiontypes of a slice differ in length")
        if c.size and (c.min() < 0 or c.max() > 1):
            raise ValueError("not implemented")
    offs = np.concatenate([[0], np.cumsum([k.size for k in strikes])]).astype(np.uintp)
    total = int(offs[-1])
    k_all = np.ascontiguousarray(np.concatenate([k.ravel() for k in strikes])) if total else np.zeros(1)
    c_all = np.ascontiguousarray(np.concatenate(codes)) if total else np.zeros(1, dtype=np.int8)
    if not (np.all(np.isfinite(f)) and np.all(np.isfinite(k_all))):
        raise ValueError("forwards and strikes must be finite")
    out = {"m": m, "total": total, "offs": offs, "forwards": f, "strikes": k_all, "codes": c_all, "gammas": g,
           "strikes_ttms": [k.ravel() for k in strikes], "codes_ttms": codes, "shapes": [k.shape for k in strikes]}
    # the C-argument run of the tilted entries: forwards, n_expiries, strikes, types, offsets (no discount factors; the arrays above
    # keep the pointers' memory alive), and the gammas with their count
    out["args"] = (ptr(f), m, ptr(k_all), ptr(c_all), offs.ctypes.data_as(C.POINTER(C.c_size_t)))
    out["gamma_args"] = (ptr(g), g.size)
    if ttms is not None:
        t = np.ascontiguousarray(np.asarray(ttms, dtype=np.float64)).ravel()
        if t.size != m:
            raise ValueError("chain arrays must have one entry per maturity")
        out["ttms"] = t
        out["ttms_arg"] = ptr(t)                      # the session entries alone take the ttms
    return out


def strike_shifts(ch: dict, shifts=None) -> np.ndarray:
    """the host constant of every strike's sums of a tilted_chain_arrays chain, flat [K] (one zero for a chain without strikes);
    default: the intrinsic value at the forward (payoff_shifts)"""
    K = ch["total"]
    if shifts is None:
        shifts = [payoff_shifts(k, c, float(f), LOG_RETURN) for k, c, f in zip(ch["strikes_ttms"], ch["codes_ttms"], ch["forwards"])]
    sh = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.float64).ravel() for s in shifts])) if K else np.zeros(1)
    if K and sh.size != K:
        raise ValueError("one shift per strike")
    return sh


def tilted_results(prices: np.ndarray, stderrs: np.ndarray, stats: np.ndarray, ch: dict):
    """flat [G][K] prices / errors and [G][m][8] statistics -> ([G][m] arrays in the strikes' shapes, the same, stats [G, m, 8])"""
    G, K, offs = ch["gammas"].size, ch["total"], ch["offs"]
    cut = lambda a: [[a[g * K + int(offs[i]):g * K + int(offs[i + 1])].reshape(ch["shapes"][i]).copy()    # noqa: E731
                      for i in range(ch["m"])] for g in range(G)]
    return cut(prices), cut(stderrs), np.array(stats, dtype=np.float64).reshape(G, ch["m"], TILTED_STATS_DOUBLES)


def tilted_greeks_results(greeks: np.ndarray, stats: np.ndarray, ch: dict):
    """flat [G][TCG_ROWS][K] Greeks and [G][m][TCG_STATS_DOUBLES] statistics -> ([G] dicts {field of TCG_FIELDS: [m] arrays in the
    strikes' shapes}, stats [G, m, TCG_STATS_DOUBLES])"""
    G, K, offs = ch["gammas"].size, ch["total"], ch["offs"]
    rows = np.asarray(greeks, dtype=np.float64)[:G * TCG_ROWS * K].reshape(G, TCG_ROWS, K)
    out = [{name: [rows[g, r, int(offs[i]):int(offs[i + 1])].reshape(ch["shapes"][i]).copy() for i in range(ch["m"])]
            for r, name in enumerate(TCG_FIELDS)} for g in range(G)]
    return out, np.array(stats, dtype=np.float64).reshape(G, ch["m"], TCG_STATS_DOUBLES)


def tilted_greeks_stats_dicts(stats: np.ndarray) -> list:
    """stats [m, 9] of one gamma -> one dict per expiry, keys TILTED_COND_GREEKS_STATS_FIELDS (the three counts as ints)"""
    return [{k: (int(v) if k in ("n_kept", "n_dropped", "n_zero_cv") else float(v)) for k, v in zip(TILTED_COND_GREEKS_STATS_FIELDS, row)}
            for row in stats]


def tilted_stats_dicts(stats: np.ndarray) -> list:
    """stats [m, 8] of one gamma -> one dict per expiry, keys TILTED_STATS_FIELDS (the two counts as ints)"""
    return [{k: (int(v) if k in ("n_kept", "n_dropped") else float(v)) for k, v in zip(TILTED_STATS_FIELDS, row)} for row in stats]


# ---- Monte Carlo chain Greeks (include/svmc.h, svmc_greeks_payoff_chain): the rows of the two result blocks ----------------------
GREEKS_MAX_PARAMS = 31         # SVMC_GREEKS_MAX_PARAMS
GREEKS_BASE_FIELDS = ("delta", "delta_stderr", "dual_delta", "dual_delta_stderr", "n_itm")    # SVMC_GREEKS_BASE_ROWS
GREEKS_SENS_FIELDS = ("sens", "sens_stderr", "n_pairs")                                       # SVMC_GREEKS_SENS_ROWS


# ---- the single-chain session entries svmc_<model>_chain_price{,_cmc,_cmc_greeks} (HipEngine._price_chain_fused) --------------------
def _logsv_args(ch, v0, theta, kappa1, kappa2, beta, volvol, etas, is_spot_measure):
    """LogSV: the etas go between the discount factors and the expiry count, six scalars and the measure after the quotes"""
    return (ptr(chain_etas(etas, ch["m"])),), (float(v0), float(theta), float(kappa1), float(kappa2), float(beta), float(volvol),
                                               int(bool(is_spot_measure)))


def _heston_args(ch, v0, theta, kappa, rho, volvol, scheme=None):
    """Heston: five scalars after the quotes, then the scheme code where the entry takes one (the conditional ones step Euler)"""
    return (), (float(v0), float(theta), float(kappa), float(rho), float(volvol)) + (() if scheme is None else (int(scheme),))


def _hawkesjd_args(ch, params):
    """Hawkes: the SVMC_HAWKESJD_PARAMS doubles of include/svmc.h after the quotes"""
    return (), (ptr(np.ascontiguousarray(params, dtype=np.float64)),)


def _fused_names(model: str, step_one: str, step_chain: str, cond: str) -> dict:
    """result kind -> (C symbol, the stepping kernel's name for one expiry, for a chain) as start_kernel_timing reports them"""
    stem = f"svmc_{model}_chain_price"
    return {"": (stem, step_one, step_chain), "_cmc": (stem + "_cmc", cond, cond), "_cmc_greeks": (stem + "_cmc_greeks", cond, cond)}


# model -> (how the route's parameters become (arguments before the expiry count, arguments after the quotes), the names)
FUSED_MODELS = {
    "logsv": (_logsv_args, _fused_names("logsv", "logsv_rng_kernel", "logsv_chain_rng_kernel", "logsv_chain_cmc_kernel")),
    "heston": (_heston_args, _fused_names("heston", "heston_rng_kernel", "heston_chain_rng_kernel", "heston_chain_cmc_kernel")),
    "hawkesjd": (_hawkesjd_args, _fused_names("hawkesjd", "hawkesjd_chain_rng_kernel", "hawkesjd_chain_rng_kernel",
                                              "hawkes_chain_cond_kernel")),
}
# result kind -> (rows of the result block, doubles per expiry of the statistics, their shaping): (prices, stderrs), the same with
# statistics, (fields, statistics)
FUSED_KINDS = {"": (2, 0, None), "_cmc": (2, CMC_STATS_DOUBLES, cmc_stats_dicts),
               "_cmc_greeks": (CMC_GREEKS_ROWS, CMC_GREEKS_STATS_DOUBLES, cmc_greeks_stats_dicts)}
# the models of the many-job, sensitivity and set routes (HipEngine._model_entry): model -> its entry takes a mode argument
PLAIN_MANY_MODELS = {"logsv": True, "heston": True, "hawkesjd": False}      # is_spot_measure, the scheme code, nothing
GREEKS_MODELS = {"logsv": True, "heston": True}
CMC_MODELS = {"logsv": True, "heston": False}                               # the conditional Heston entries step Euler only

MANY_MAX_JOBS = 64             # jobs per svmc_*_chain_price_many call: SVMC_MANY_MAX_JOBS of include/svmc.h
BULK_KEEP_FRACTION = 0.125     # of the device's memory: what an engine's cached bulk buffers may hold between calls (trim_bulk)


class HipEngine:
    def __init__(self, n_path: int, device: Optional[int] = None, path_offset: int = 0,
                 n_snapshots: int = 0, stream: Optional[int] = None):
        self.lib = _lib.load()
        cnt = C.c_int()
        _lib.check(self.lib.svmc_device_count(C.byref(cnt)))
        if cnt.value < 1:
            raise _lib.SvmcError("no HIP device visible: the svmc Monte Carlo path runs on the GPU only")
        if device is not None:
            _lib.check(self.lib.svmc_set_device(int(device)))
        dev = C.c_int()
        _lib.check(self.lib.svmc_get_device(C.byref(dev)))
        self.device = dev.value
        self.n_path = int(n_path)
        self.path_offset = int(path_offset)
        self.stream = stream  # None = default stream
        self.x = DeviceBuffer(self.n_path)
        self.vol = DeviceBuffer(self.n_path)
        self.qvar = DeviceBuffer(self.n_path)
        ws = C.c_size_t()
        _lib.check(self.lib.svmc_slice_workspace_bytes(self.n_path, C.byref(ws)))
        self.ws_bytes = ws.value
        self.ws = DeviceBuffer(self.ws_bytes // 8)
        self._snap: Optional[DeviceBuffer] = None
        self._snap_rows = 0
        self._rand: Optional[DeviceBuffer] = None
        self._factors: Optional[DeviceBuffer] = None   # rough LogSV: [n_factors][n_path]
        self._cv: Optional[DeviceBuffer] = None        # conditional Monte Carlo: the fourth state array (self.cv)
        self._sums = {}
        self._pinned, self._pinned_doubles = None, 0    # page-locked staging of the small result downloads
        self._bulk = {}                                 # slot -> DeviceBuffer: multi-GB results kept between calls (_bulk_buffer)
        self._device_bytes = None                       # the device's memory, asked once (trim_bulk)
        self._prof = None   # list of (name, start_event, stop_event) while kernel timing is on
        self._fused = None                              # svmc_session_t over this engine's state (fused_chain_session)
        self._fused_size = (0, 0)
        self._fused_graphs = True                       # use_graphs()
        self._fused_timing = False
        self.closed = False
        if n_snapshots:
            self.reserve_snapshots(n_snapshots)

    # ---- plumbing -------------------------------------------------------------------------------
    def synchronize(self) -> None:
        _lib.check(self.lib.svmc_stream_synchronize(self.stream))

    def reserve_snapshots(self, rows: int) -> None:
        if self._snap is None or self._snap_rows < rows:
            if self._snap is not None:
                self._snap.free()
            self._snap = DeviceBuffer(rows * self.n_path)
            self._snap_rows = rows

    def snapshot_ptr(self, row: int) -> int:
        return self._snap.offset(row * self.n_path)

    def alloc_sums(self, n_doubles: int, tag: str = "sums") -> Tuple[int, object]:
        """named device buffer for reduction results; returns (ptr, owner).  Buffers with different tags
        never alias; a tag's buffer is re-used (grown) across calls."""
        buf = self._sums.get(tag)
        if buf is None or buf.n < n_doubles:
            if buf is not None:
                buf.free()
            buf = DeviceBuffer(max(int(n_doubles), 1))
            self._sums[tag] = buf
        return buf.ptr, buf

    PINNED_DOWNLOAD_MAX = 1 << 16       # doubles: the reduction results of a chain; bulk state goes the plain way

    def download(self, ptr: int, n: int) -> np.ndarray:
        """n doubles from device memory.  Small downloads (the payoff sums every chain call ends with) land in a page-locked
        buffer the engine keeps: a copy into pageable memory goes through the runtime's staging path and costs 16 us more
        per call than one into pinned memory (tools/ubench/sync_latency.py: 29.2 vs 16.3 us for kernel + copy + wait)."""
        n = int(n)
        if 0 < n <= self.PINNED_DOWNLOAD_MAX:
            if self._pinned is None or self._pinned_doubles < n:
                if self._pinned is not None:
                    _lib.check(self.lib.svmc_host_free(self._pinned))
                    self._pinned = None
                want = max(n, 4096)
                buf = C.c_void_p()
                _lib.check(self.lib.svmc_host_alloc(C.byref(buf), 8 * want))
                self._pinned, self._pinned_doubles = buf, want
            _lib.check(self.lib.svmc_memcpy_d2h(self._pinned, ptr, 8 * n, self.stream))
            self.synchronize()
            return np.ctypeslib.as_array(C.cast(self._pinned, C.POINTER(C.c_double)), shape=(n,)).copy()
        return pipelined_download(ptr, n, self.stream)      # bulk (terminal state vectors, path arrays): the pinned pipeline

    def upload(self, ptr: int, host: np.ndarray) -> None:
        host = np.ascontiguousarray(host, dtype=np.float64)
        _lib.check(self.lib.svmc_memcpy_h2d(ptr, host.ctypes.data, host.nbytes, self.stream))
        self.synchronize()  # the pageable source may be released by the caller

    # ---- kernel timing (HIP events on the launch stream; bench.py) ---------------------------------
    def start_kernel_timing(self) -> None:
        self._prof = []

    def _timed(self, name: str, launch) -> None:
        if self._prof is None:
            launch()
            return
        e0, e1 = C.c_void_p(), C.c_void_p()
        _lib.check(self.lib.svmc_event_create(C.byref(e0)))
        _lib.check(self.lib.svmc_event_create(C.byref(e1)))
        _lib.check(self.lib.svmc_event_record(e0, self.stream))
        launch()
        _lib.check(self.lib.svmc_event_record(e1, self.stream))
        self._prof.append((name, e0, e1))

    def stop_kernel_timing(self):
        """-> {kernel name: [durations in ms]} of every generator launch since start_kernel_timing()."""
        out = {}
        for name, e0, e1 in self._prof or []:
            if e1 is None:                               # a fused chain call: the session measured it (e0 holds the milliseconds)
                out.setdefault(name, []).append(e0)
                continue
            ms = C.c_float()
            _lib.check(self.lib.svmc_event_elapsed_ms(e0, e1, C.byref(ms)))
            out.setdefault(name, []).append(ms.value)
            self.lib.svmc_event_destroy(e0)
            self.lib.svmc_event_destroy(e1)
        self._prof = None
        return out

    # ---- one C-ABI call per chain (single GPU) -----------------------------------------------------
    def fused_chain_session(self, n_expiries: int, n_strikes: int):
        """a C-ABI session (svmc_session_create_on) over THIS engine's state arrays and stream, grown on demand: the fused
        chain drivers then leave the terminal state where get_state() reads it"""
        if self._fused is None or self._fused_size[0] < n_expiries or self._fused_size[1] < n_strikes:
            if self._fused is not None:
                _lib.check(self.lib.svmc_session_destroy(self._fused))
                self._fused = None
            size = (max(int(n_expiries), self._fused_size[0], 1), max(int(n_strikes), self._fused_size[1], 1))
            sess = C.c_void_p()
            _lib.check(self.lib.svmc_session_create_on(C.byref(sess), self.n_path, size[0], size[1], self.x.ptr, self.vol.ptr,
                                                       self.qvar.ptr, self.path_offset, self.stream))
            self._fused, self._fused_size, self._fused_timing = sess, size, False
            if not self._fused_graphs:
                _lib.check(self.lib.svmc_session_use_graphs(sess, 0))
        return self._fused

    def _price_chain_fused(self, ch: dict, model: str, kind: str, params: tuple, nb_steps_per_year, flag: int, seed: int, call_id: int):
        """ONE svmc_<model>_chain_price<kind> call on this engine's session (ch: marshalled_chain): the single-chain route of every
        model (FUSED_MODELS: how `params` become C arguments, the stepping kernel's names) and result kind (FUSED_KINDS: the output
        buffers and their shaping).  flag: the variable type of the plain kind, recenter of the conditional ones.  While kernel
        timing is on (start_kernel_timing) the session brackets its stepping launch with HIP events and the time is kept under
        the kernel's name"""
        pack, names = FUSED_MODELS[model]
        rows, stats_doubles, stats_dicts = FUSED_KINDS[kind]
        mid, args = pack(ch, *params)
        a = ch["args"]
        res = np.empty((rows, max(ch["total"], 1)))
        outs = (row_ptr(res, 0), row_ptr(res, 1)) if rows == 2 else (ptr(res),)
        if stats_dicts is not None:
            stats = np.empty((ch["m"], stats_doubles))
            outs += (ptr(stats),)
        fn = getattr(self.lib, names[kind][0])
        self._session_call(ch, lambda sess: fn(sess, *a[:3], *mid, *a[3:], *args, int(nb_steps_per_year), flag, int(seed), int(call_id),
                                               *outs), names[kind][1 if ch["m"] == 1 else 2])
        if rows != 2:
            return cmc_greeks_dict(res, ch["slices"]), stats_dicts(stats)
        out = expiry_rows(res, ch["slices"])
        return out if stats_dicts is None else out + (stats_dicts(stats),)

    def _session_call(self, ch: dict, call, kernel_name: str) -> None:
        """run call(session) on the fused chain session of ch's size, the stepping launch timed under kernel_name while kernel
        timing is on"""
        sess = self.fused_chain_session(ch["m"], ch["total"])
        timing = self._prof is not None
        if timing != self._fused_timing:
            _lib.check(self.lib.svmc_session_time_stepping(sess, int(timing)))
            self._fused_timing = timing
        _lib.check(call(sess))
        if timing:
            ms = C.c_float()
            _lib.check(self.lib.svmc_session_last_stepping_ms(sess, C.byref(ms)))
            self._prof.append((kernel_name, float(ms.value), None))

    def price_logsv_chain_fused(self, ch: dict, v0, theta, kappa1, kappa2, beta, volvol, etas, is_spot_measure, nb_steps_per_year,
                                variable_type: int, seed: int, call_id: int):
        """logsv_mc_chain_pricer on one GPU as ONE svmc_logsv_chain_price call on this engine's state (ch: marshalled_chain):
        the kernels, their order and their arguments are those of mc_chain.price_chain_on_engine -- the same bits -- without
        the dozen ctypes calls and NumPy temporaries around them (tools/r06/chain_call_breakdown.py: 0.135 -> 0.114 ms for a
        4 x 13 chain at 2^16 paths)"""
        return self._price_chain_fused(ch, "logsv", "", (v0, theta, kappa1, kappa2, beta, volvol, etas, is_spot_measure),
                                       nb_steps_per_year, int(variable_type), seed, call_id)

    def price_heston_chain_fused(self, ch: dict, v0, theta, kappa, rho, volvol, scheme: int, nb_steps_per_year, variable_type: int,
                                 seed: int, call_id: int):
        """heston_mc_chain_pricer on one GPU as ONE svmc_heston_chain_price call on this engine's state"""
        return self._price_chain_fused(ch, "heston", "", (v0, theta, kappa, rho, volvol, scheme), nb_steps_per_year, int(variable_type),
                                       seed, call_id)

    @staticmethod
    def _many_jobs(params, seeds: Sequence[int], call_ids: Sequence[int], what: str = "one seed and one call id per job"):
        """(J, the C pointers of params [J][...], seeds [J] and call ids [J] as contiguous arrays, each keeping its array alive)"""
        params = np.ascontiguousarray(params, dtype=np.float64)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        ids = np.ascontiguousarray(call_ids, dtype=np.uint32)
        if not (seeds.size == ids.size == params.shape[0]):
            raise ValueError(what)
        return params.shape[0], (ptr(params), ptr(seeds), ptr(ids))

    def _model_entry(self, who: str, model: str, stem: str, allowed: dict, mode, as_c=int):
        """(the entry point svmc_<model>_<stem>, its mode arguments) of the route `who`, open to the models of `allowed` (model ->
        the entry takes as_c(mode))"""
        if model not in allowed:
            raise ValueError(f"{who}: unknown model {model!r}")
        return getattr(self.lib, f"svmc_{model}_{stem}"), ((as_c(mode),) if allowed[model] else ())

    def price_chain_many_fused(self, ch: dict, model: str, params: np.ndarray, seeds: Sequence[int], call_ids: Sequence[int],
                               mode: int, nb_steps_per_year: int, variable_type: int):
        """J jobs of one chain as ONE svmc_logsv_chain_price_many (model "logsv", mode = is_spot_measure, params [J][6 + m]),
        svmc_heston_chain_price_many ("heston", mode = scheme code, params [J][5]) or svmc_hawkesjd_chain_price_many ("hawkesjd",
        mode unused, params [J][SVMC_HAWKESJD_PARAMS]) call on this engine's session, J at most MANY_MAX_JOBS: per job the
        (prices, stderrs) of the single fused call with its (seed, call id), cut into expiries"""
        fn, modes = self._model_entry("price_chain_many_fused", model, "chain_price_many", PLAIN_MANY_MODELS, mode)
        n_jobs, jobs = self._many_jobs(params, seeds, call_ids)
        sess = self.fused_chain_session(ch["m"], ch["total"])
        res = np.empty((2, n_jobs, max(ch["total"], 1)))
        _lib.check(fn(sess, *ch["args"], n_jobs, *jobs, *modes, int(nb_steps_per_year), int(variable_type), row_ptr(res, 0),
                      row_ptr(res, 1)))
        return expiry_rows_per_job(res, ch["slices"])

    def price_hawkesjd_chain_fused(self, ch: dict, params: np.ndarray, nb_steps_per_year: int, variable_type: int, seed: int,
                                   call_id: int):
        """hawkesjd_mc_chain_pricer on one GPU as ONE svmc_hawkesjd_chain_price call on this engine's state (vol / qvar hold
        lambda_p / lambda_m afterwards); params: the SVMC_HAWKESJD_PARAMS doubles of include/svmc.h"""
        return self._price_chain_fused(ch, "hawkesjd", "", (params,), nb_steps_per_year, int(variable_type), seed, call_id)

    def hawkesjd_rng(self, nb_steps: int, dt: float, params: np.ndarray, seed: int, call_id: int, step_offset: int = 0) -> None:
        """simulate_hawkesjd_terminal on this engine's state (x, lambda_p, lambda_m) in place"""
        params = np.ascontiguousarray(params, dtype=np.float64)
        self._timed("hawkesjd_rng_kernel", lambda: _lib.check(self.lib.svmc_hawkesjd_terminal_rng(
            self.x.ptr, self.vol.ptr, self.qvar.ptr, self.n_path, int(nb_steps), float(dt), ptr(params), int(seed), int(call_id),
            self.path_offset, int(step_offset), self.stream)))

    # ---- conditional Monte Carlo for the Hawkes jump-diffusion (include/svmc.h): the state is (mu, lambda_p,
    # lambda_m) in x / vol / qvar; the conditional variance is one double per expiry, formed on the host
    def hawkesjd_chain_cond(self, nb_steps: Sequence[int], dts: Sequence[float], params: np.ndarray, seed: int, call_id: int,
                            step_offset: int = 0, cv_start: float = 0.0, mu_row: Optional[int] = 0,
                            cv_row: Optional[int] = None) -> np.ndarray:
        """svmc_hawkesjd_chain_cond on this engine's (mu, lambda_p, lambda_m): expiry i's mu goes to snapshot row mu_row + i and its
        cv (the same double on every path) to row cv_row + i (default: right after the mu rows; mu_row=None: no snapshots at all).
        Returns the host cv_i [n_slices]; a later call continues the chain with step_offset = the steps so far and cv_start = the
        last of them"""
        n = len(nb_steps)
        nb = np.ascontiguousarray(nb_steps, dtype=np.int32)
        dt, params = np.ascontiguousarray(dts, dtype=np.float64), np.ascontiguousarray(params, dtype=np.float64)
        if dt.size != n:
            raise ValueError("one dt per slice")
        mu_ptr = cv_ptr = None
        if mu_row is not None:
            cv_row = mu_row + n if cv_row is None else cv_row
            mu_ptr, cv_ptr, _ = self._cmc_rows(n, mu_row, cv_row, None)
        cvs = np.empty(max(n, 1))
        self._timed("hawkes_chain_cond_kernel", lambda: _lib.check(self.lib.svmc_hawkesjd_chain_cond(
            self.x.ptr, self.vol.ptr, self.qvar.ptr, self.n_path, n, ptr(nb), ptr(dt), ptr(params), float(cv_start), int(seed),
            int(call_id), self.path_offset, int(step_offset), mu_ptr, cv_ptr, ptr(cvs), self.stream)))
        return cvs[:n]

    def price_hawkesjd_chain_cmc_fused(self, ch: dict, params: np.ndarray, nb_steps_per_year: int, recenter: bool, seed: int,
                                       call_id: int):
        """hawkesjd_mc_chain_pricer_conditional as ONE svmc_hawkesjd_chain_price_cmc call on this engine's state; returns (prices,
        stderrs, stats) cut into expiries"""
        return self._price_chain_fused(ch, "hawkesjd", "_cmc", (params,), nb_steps_per_year, int(bool(recenter)), seed, call_id)

    def price_hawkesjd_chain_cmc_greeks_fused(self, ch: dict, params: np.ndarray, nb_steps_per_year: int, recenter: bool, seed: int,
                                              call_id: int):
        """hawkesjd_mc_chain_greeks_conditional as ONE svmc_hawkesjd_chain_price_cmc_greeks call on this engine's state; returns
        (fields, stats) as conditional_greeks"""
        return self._price_chain_fused(ch, "hawkesjd", "_cmc_greeks", (params,), nb_steps_per_year, int(bool(recenter)), seed, call_id)

    # ---- state ----------------------------------------------------------------------------------
    def fill_state(self, x0: float, vol0: float, qvar0: float) -> None:
        _lib.check(self.lib.svmc_fill_state(self.x.ptr, self.vol.ptr, self.qvar.ptr, self.n_path,
                                            float(x0), float(vol0), float(qvar0), self.stream))

    def set_state(self, x: np.ndarray, vol: np.ndarray, qvar: np.ndarray) -> None:
        for buf, a in ((self.x, x), (self.vol, vol), (self.qvar, qvar)):
            a = np.ascontiguousarray(a, dtype=np.float64)
            assert a.shape == (self.n_path,)
            self.upload(buf.ptr, a)

    def get_state(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        return (self.download(self.x.ptr, self.n_path), self.download(self.vol.ptr, self.n_path),
                self.download(self.qvar.ptr, self.n_path))

    def snapshot(self, row: int, which: str = "x") -> None:
        src = self.x.ptr if which == "x" else self.qvar.ptr
        _lib.check(self.lib.svmc_memcpy_d2d(self.snapshot_ptr(row), src, 8 * self.n_path, self.stream))

    def _bulk_buffer(self, n_doubles: int, slot: int = 0) -> DeviceBuffer:
        """the engine's cached buffer for a bulk result that does not leave the call (the path array behind a NumPy return, the
        arrays vol_path_moments reduces): grown when needed, kept until close() / release_bulk().  Allocating and freeing 8.6 GB
        per call costs the runtime 0.25-0.7 s every other call (the VRAM is mapped and unmapped; profiles/r05_moments_timing
        .jsonl) -- two hundred times the kernel that fills it."""
        buf = self._bulk.get(slot)
        if buf is None or buf.n < n_doubles:
            if buf is not None:
                buf.free()
            buf = DeviceBuffer(int(n_doubles))
            self._bulk[slot] = buf
        return buf

    def trim_bulk(self) -> None:
        """after a call whose bulk result has left the device: keep the cached buffers only while together they stay under an
        eighth of the device's memory (36 GB of an MI355X's 288: C2-sized path arrays, 8.6 GB each, stay; a caller that once
        simulated 10^7 paths does not pin 80 GB for the life of the process) -- BULK_KEEP_FRACTION, release_bulk() for all of it"""
        held = 8 * sum(b.n for b in self._bulk.values())
        if held == 0:
            return
        if self._device_bytes is None:
            name, cus, khz, mem = C.create_string_buffer(128), C.c_int(), C.c_int(), C.c_size_t()
            _lib.check(self.lib.svmc_device_info(self.device, name, 128, C.byref(cus), C.byref(khz), C.byref(mem)))
            self._device_bytes = int(mem.value)
        if held > BULK_KEEP_FRACTION * self._device_bytes:
            self.release_bulk()

    def release_bulk(self) -> None:
        """give the cached bulk buffers back (they otherwise stay with the engine: up to two path arrays of the largest size seen)"""
        self.synchronize()
        for b in self._bulk.values():
            b.free()
        self._bulk = {}

    # ---- randoms --------------------------------------------------------------------------------
    def _rand_buffer(self, n_doubles: int) -> DeviceBuffer:
        if self._rand is None or self._rand.n < n_doubles:
            if self._rand is not None:
                self._rand.free()
            self._rand = DeviceBuffer(n_doubles)
        return self._rand

    def upload_randoms(self, arrays: Sequence[np.ndarray], col0: int = 0) -> Tuple[int, ...]:
        """upload the local column range [col0, col0 + n_path) of host [nb_steps, nb_path_total] arrays."""
        nb = arrays[0].shape[0]
        buf = self._rand_buffer(len(arrays) * nb * self.n_path)
        ptrs, keep = [], []         # `keep`: converted temporaries must outlive the asynchronous copies below
        for i, a in enumerate(arrays):
            a = np.asarray(a)
            if a.dtype != np.float64 or not a.flags.c_contiguous:
                a = np.ascontiguousarray(a, dtype=np.float64)
            keep.append(a)
            assert a.ndim == 2 and a.shape[0] == nb and a.shape[1] >= col0 + self.n_path
            dst = buf.offset(i * nb * self.n_path)
            _lib.check(self.lib.svmc_memcpy2d_h2d(dst, 8 * self.n_path, a.ctypes.data + 8 * col0, 8 * a.shape[1],
                                                  8 * self.n_path, nb, self.stream))
            ptrs.append(dst)
        self.synchronize()
        del keep
        return tuple(ptrs)

    def fill_normals(self, nb_steps: int, seed: int, call_id: int = 0, step_offset: int = 0) -> Tuple[int, int]:
        buf = self._rand_buffer(2 * nb_steps * self.n_path)
        w0, w1 = buf.ptr, buf.offset(nb_steps * self.n_path)
        _lib.check(self.lib.svmc_fill_normals(w0, w1, self.n_path, self.n_path, nb_steps, seed, call_id,
                                              self.path_offset, step_offset, self.stream))
        return w0, w1

    # ---- generators -----------------------------------------------------------------------------
    def logsv_rng(self, nb_steps, dt, theta, kappa1, kappa2, beta, volvol, eta, is_spot_measure, seed, call_id,
                  step_offset) -> None:
        self._timed("logsv_rng_kernel", lambda: _lib.check(self.lib.svmc_logsv_terminal_rng(
            self.x.ptr, self.vol.ptr, self.qvar.ptr, self.n_path, int(nb_steps), float(dt), float(theta),
            float(kappa1), float(kappa2), float(beta), float(volvol), float(eta), int(bool(is_spot_measure)),
            int(seed), int(call_id), self.path_offset, int(step_offset), self.stream)))

    def logsv_slice_rng(self, nb_steps, dt, theta, kappa1, kappa2, beta, volvol, eta, is_spot_measure, seed, call_id,
                        step_offset, forward, snap_row, qvar_row, spot_ptr, start=None) -> None:
        """advance + snapshot + spot sums of one expiry in one kernel (svmc_logsv_slice_rng).  start = (x0, sigma0, qvar0):
        every path starts there (svmc_logsv_slice_rng_from: no fill launch, the state buffers are outputs only)"""
        fn = self.lib.svmc_logsv_slice_rng if start is None else functools.partial(self.lib.svmc_logsv_slice_rng_from,
                                                                                   *[float(v) for v in start])
        self._timed("logsv_rng_kernel", lambda: _lib.check(fn(
            self.x.ptr, self.vol.ptr, self.qvar.ptr, self.n_path, int(nb_steps), float(dt), float(theta),
            float(kappa1), float(kappa2), float(beta), float(volvol), float(eta), int(bool(is_spot_measure)),
            int(seed), int(call_id), self.path_offset, int(step_offset), float(forward), self.snapshot_ptr(snap_row),
            None if qvar_row is None else self.snapshot_ptr(qvar_row), spot_ptr, self.ws.ptr, self.ws_bytes,
            self.stream)))

    def logsv_chain_rng(self, nb_steps: Sequence[int], dts: Sequence[float], etas: Sequence[float],
                        forwards: Sequence[float], theta, kappa1, kappa2, beta, volvol, is_spot_measure, seed, call_id,
                        step_offset, need_qvar: bool, spot_ptr: int, start=None) -> None:
        """every expiry of a chain in one stepping launch (svmc_logsv_chain_rng): snapshot rows 0..m-1 get the
        terminal x of each expiry, rows m..2m-1 the quadratic variance (need_qvar), spot_ptr the 2m spot sums;
        start = (x0, sigma0, qvar0) as in logsv_slice_rng"""
        m = len(nb_steps)
        nbs = (C.c_int * m)(*[int(v) for v in nb_steps])
        d, e, f = (np.ascontiguousarray(a, dtype=np.float64) for a in (dts, etas, forwards))
        fn = self.lib.svmc_logsv_chain_rng if start is None else functools.partial(self.lib.svmc_logsv_chain_rng_from,
                                                                                   *[float(v) for v in start])
        self._timed("logsv_chain_rng_kernel", lambda: _lib.check(fn(
            self.x.ptr, self.vol.ptr, self.qvar.ptr, self.n_path, m, nbs, ptr(d), ptr(e),
            ptr(f), float(theta), float(kappa1), float(kappa2), float(beta), float(volvol),
            int(bool(is_spot_measure)), int(seed), int(call_id), self.path_offset, int(step_offset), self.snapshot_ptr(0),
            self.snapshot_ptr(m) if need_qvar else None, spot_ptr, self.ws.ptr, self.ws_bytes, self.stream)))

    def heston_chain_rng(self, nb_steps: Sequence[int], dts: Sequence[float], forwards: Sequence[float], theta, kappa,
                         rho, volvol, scheme, seed, call_id, step_offset, need_qvar: bool, spot_ptr: int, start=None) -> None:
        """every expiry of a Heston chain in one stepping launch (svmc_heston_chain_rng); layout and `start` as
        logsv_chain_rng"""
        m = len(nb_steps)
        nbs = (C.c_int * m)(*[int(v) for v in nb_steps])
        d, f = (np.ascontiguousarray(a, dtype=np.float64) for a in (dts, forwards))
        fn = self.lib.svmc_heston_chain_rng if start is None else functools.partial(self.lib.svmc_heston_chain_rng_from,
                                                                                    *[float(v) for v in start])
        self._timed("heston_chain_rng_kernel", lambda: _lib.check(fn(
            self.x.ptr, self.vol.ptr, self.qvar.ptr, self.n_path, m, nbs, ptr(d), ptr(f),
            float(theta), float(kappa), float(rho), float(volvol), int(scheme), int(seed), int(call_id), self.path_offset,
            int(step_offset), self.snapshot_ptr(0), self.snapshot_ptr(m) if need_qvar else None, spot_ptr, self.ws.ptr,
            self.ws_bytes, self.stream)))

    def heston_slice_rng(self, nb_steps, dt, theta, kappa, rho, volvol, scheme, seed, call_id, step_offset, forward,
                         snap_row, qvar_row, spot_ptr, start=None) -> None:
        fn = self.lib.svmc_heston_slice_rng if start is None else functools.partial(self.lib.svmc_heston_slice_rng_from,
                                                                                    *[float(v) for v in start])
        self._timed("heston_rng_kernel", lambda: _lib.check(fn(
            self.x.ptr, self.vol.ptr, self.qvar.ptr, self.n_path, int(nb_steps), float(dt), float(theta),
            float(kappa), float(rho), float(volvol), int(scheme), int(seed), int(call_id), self.path_offset,
            int(step_offset), float(forward), self.snapshot_ptr(snap_row),
            None if qvar_row is None else self.snapshot_ptr(qvar_row), spot_ptr, self.ws.ptr, self.ws_bytes,
            self.stream)))

    def finish_slice(self, forward, snap_row, qvar_row, spot_ptr) -> None:
        """the un-fused equivalent for generators without a slice epilogue (streamed randoms)"""
        self.snapshot(snap_row, "x")
        if qvar_row is not None:
            self.snapshot(qvar_row, "qvar")
        self.spot_sums(self.snapshot_ptr(snap_row), forward, spot_ptr)

    def logsv_w(self, nb_steps, dt, theta, kappa1, kappa2, beta, volvol, eta, is_spot_measure, w0_ptr, w1_ptr,
                ldw=None) -> None:
        self._timed("logsv_w_kernel", lambda: _lib.check(self.lib.svmc_logsv_terminal_w(
            self.x.ptr, self.vol.ptr, self.qvar.ptr, self.n_path, int(nb_steps), float(dt), float(theta),
            float(kappa1), float(kappa2), float(beta), float(volvol), float(eta), int(bool(is_spot_measure)),
            w0_ptr, w1_ptr, self.n_path if ldw is None else int(ldw), self.stream)))

    def rough_logsv(self, nb_steps, h, nodes, weights, v0, theta, kappa1, kappa2, rho, volvol, z0_ptr=None,
                    z1_ptr=None, ldw=None, seed=0, call_id=0, step_offset=0, from_origin=True, slice_out=None) -> None:
        """rough LogSV terminal state in (x, factor buffer, qvar); randoms streamed from z0/z1 or drawn on device.
        slice_out = (forward, snap_row, qvar_row | None, spot_ptr) adds the slice epilogue (svmc_rough_logsv_slice)."""
        nodes, weights, v0 = (np.ascontiguousarray(a, dtype=np.float64) for a in (nodes, weights, v0))
        if not (nodes.ndim == 1 and nodes.shape == weights.shape == v0.shape):
            raise ValueError("nodes, weights and v0 must be 1-d arrays of one length")
        if self._factors is None:
            self._factors = DeviceBuffer(3 * self.n_path)
        args = (self.x.ptr, self._factors.ptr, self.qvar.ptr, self.n_path, int(nb_steps), float(h), int(nodes.size),
                ptr(nodes), ptr(weights), ptr(v0), float(theta), float(kappa1),
                float(kappa2), float(rho), float(volvol), z0_ptr, z1_ptr, self.n_path if ldw is None else int(ldw),
                int(seed), int(call_id), self.path_offset, int(step_offset), int(bool(from_origin)))
        if slice_out is None:
            self._timed("rough_logsv_kernel",
                        lambda: _lib.check(self.lib.svmc_rough_logsv_terminal(*args, self.stream)))
            return
        forward, snap_row, qvar_row, spot_ptr = slice_out
        self._timed("rough_logsv_kernel", lambda: _lib.check(self.lib.svmc_rough_logsv_slice(
            *args, float(forward), self.snapshot_ptr(snap_row), None if qvar_row is None else self.snapshot_ptr(qvar_row),
            spot_ptr, self.ws.ptr, self.ws_bytes, self.stream)))

    def rough_logsv_chain(self, nb_steps: Sequence[int], hs: Sequence[float], forwards: Sequence[float], nodes, weights, v0,
                          theta, kappa1, kappa2, rho, volvol, need_qvar: bool, spot_ptr: int, z0_ptr=None, z1_ptr=None,
                          ldw=None, seed=0, call_id=0) -> None:
        """every expiry of a rough-LogSV chain in one stepping launch (svmc_rough_logsv_chain): each expiry simulated from
        time 0 on its own step, side by side; snapshot rows 0..m-1 get the terminal x, rows m..2m-1 the quadratic
        variance (need_qvar), spot_ptr the 2m spot sums"""
        nodes, weights, v0 = (np.ascontiguousarray(a, dtype=np.float64) for a in (nodes, weights, v0))
        if not (nodes.ndim == 1 and nodes.shape == weights.shape == v0.shape):
            raise ValueError("nodes, weights and v0 must be 1-d arrays of one length")
        if self._factors is None:
            self._factors = DeviceBuffer(3 * self.n_path)
        m = len(nb_steps)
        nbs = (C.c_int * m)(*[int(v) for v in nb_steps])
        h, f = (np.ascontiguousarray(a, dtype=np.float64) for a in (hs, forwards))
        self._timed("rough_logsv_expiries_kernel", lambda: _lib.check(self.lib.svmc_rough_logsv_chain(
            self.x.ptr, self._factors.ptr, self.qvar.ptr, self.n_path, m, nbs, ptr(h), ptr(f),
            int(nodes.size), ptr(nodes), ptr(weights), ptr(v0), float(theta),
            float(kappa1), float(kappa2), float(rho), float(volvol), z0_ptr, z1_ptr, self.n_path if ldw is None else int(ldw),
            int(seed), int(call_id), self.path_offset, self.snapshot_ptr(0), self.snapshot_ptr(m) if need_qvar else None,
            spot_ptr, self.ws.ptr, self.ws_bytes, self.stream)))

    def get_factors(self, n_factors: int) -> np.ndarray:
        return self.download(self._factors.ptr, n_factors * self.n_path).reshape(n_factors, self.n_path)

    def logsv_slice_w(self, nb_steps, dt, theta, kappa1, kappa2, beta, volvol, eta, is_spot_measure, w0_ptr, w1_ptr,
                      forward, snap_row, qvar_row, spot_ptr, ldw=None) -> None:
        """streamed-randoms advance + snapshot + spot sums of one expiry in one stepping launch (svmc_logsv_slice_w)"""
        self._timed("logsv_w_kernel", lambda: _lib.check(self.lib.svmc_logsv_slice_w(
            self.x.ptr, self.vol.ptr, self.qvar.ptr, self.n_path, int(nb_steps), float(dt), float(theta),
            float(kappa1), float(kappa2), float(beta), float(volvol), float(eta), int(bool(is_spot_measure)),
            w0_ptr, w1_ptr, self.n_path if ldw is None else int(ldw), float(forward), self.snapshot_ptr(snap_row),
            None if qvar_row is None else self.snapshot_ptr(qvar_row), spot_ptr, self.ws.ptr, self.ws_bytes,
            self.stream)))

    def logsv_vol_paths(self, nb_steps, dt, v0, theta, kappa1, kappa2, beta, volvol, is_spot_measure, seed, call_id,
                        brownians: Optional[np.ndarray] = None, return_device=False, out_host: Optional[np.ndarray] = None):
        """full-grid sigma paths [(nb_steps+1), n_path] (svmc_logsv_vol_paths): the host array (fetched through the pinned
        pipeline, into out_host when given); with return_device=True the resident DeviceArray (a fresh allocation the caller
        owns and frees); with return_device="view" a DeviceArray over the engine's cached bulk buffer (valid until the engine's
        next bulk call; what vol_path_moments reduces)"""
        n_out = (nb_steps + 1) * self.n_path
        out = DeviceBuffer(n_out) if return_device is True else self._bulk_buffer(n_out, 0)
        b_ptr = None
        if brownians is not None:
            (b_ptr,) = self.upload_randoms((brownians,))
        _lib.check(self.lib.svmc_logsv_vol_paths(out.ptr, self.n_path, self.n_path, int(nb_steps), float(dt), float(v0),
                                                 float(theta), float(kappa1), float(kappa2), float(beta), float(volvol),
                                                 int(bool(is_spot_measure)), b_ptr, self.n_path, int(seed),
                                                 int(call_id), self.path_offset, self.stream))
        arr = DeviceArray(out, (nb_steps + 1, self.n_path), self.stream, self.device, owns=return_device is True,
                          scratch=None if return_device is True else self._bulk_buffer)
        if return_device:
            return arr
        host = arr.numpy(out_host)
        arr.free()
        self.trim_bulk()
        return host

    def heston_rng(self, nb_steps, dt, theta, kappa, rho, volvol, scheme, seed, call_id, step_offset) -> None:
        self._timed("heston_rng_kernel", lambda: _lib.check(self.lib.svmc_heston_terminal_rng(
            self.x.ptr, self.vol.ptr, self.qvar.ptr, self.n_path, int(nb_steps), float(dt), float(theta),
            float(kappa), float(rho), float(volvol), int(scheme), int(seed), int(call_id), self.path_offset,
            int(step_offset), self.stream)))

    def heston_w(self, nb_steps, dt, theta, kappa, rho, volvol, w0_ptr, w1_ptr, ldw=None) -> None:
        _lib.check(self.lib.svmc_heston_terminal_w(
            self.x.ptr, self.vol.ptr, self.qvar.ptr, self.n_path, int(nb_steps), float(dt), float(theta),
            float(kappa), float(rho), float(volvol), w0_ptr, w1_ptr,
            self.n_path if ldw is None else int(ldw), self.stream))

    def heston_qe_w(self, nb_steps, dt, theta, kappa, rho, volvol, z0_ptr, z1_ptr, u_ptr, ldw=None) -> None:
        _lib.check(self.lib.svmc_heston_qe_terminal_w(
            self.x.ptr, self.vol.ptr, self.qvar.ptr, self.n_path, int(nb_steps), float(dt), float(theta),
            float(kappa), float(rho), float(volvol), z0_ptr, z1_ptr, u_ptr,
            self.n_path if ldw is None else int(ldw), self.stream))

    # ---- payoff reduction -----------------------------------------------------------------------
    def spot_sums(self, x_ptr: int, forward: float, out_ptr: int) -> None:
        _lib.check(self.lib.svmc_spot_sums(x_ptr, self.n_path, float(forward), out_ptr, self.ws.ptr,
                                           self.ws_bytes, self.stream))

    def payoff_sums(self, x_ptr: int, qvar_ptr: Optional[int], forward: float, ttm: float, spot_sums_ptr: int,
                    strikes: np.ndarray, codes: np.ndarray, shifts: np.ndarray, variable_type: int,
                    out_ptr: int) -> None:
        k = len(strikes)
        _lib.check(self.lib.svmc_payoff_sums(
            x_ptr, qvar_ptr, self.n_path, float(forward), float(ttm), spot_sums_ptr,
            strikes.ctypes.data_as(C.POINTER(C.c_double)), codes.ctypes.data_as(C.POINTER(C.c_int8)),
            shifts.ctypes.data_as(C.POINTER(C.c_double)), k, int(variable_type), out_ptr, self.ws.ptr,
            self.ws_bytes, self.stream))

    def payoff_sums_chain(self, snap_rows: Sequence[int], qvar_rows: Optional[Sequence[int]], forwards, ttms,
                          spot_sums_ptr: int, strikes: Sequence[np.ndarray], codes: Sequence[np.ndarray],
                          shifts: Sequence[np.ndarray], variable_type: int, out_ptr: int) -> None:
        """per-strike payoff sums of ALL expiries in one pair of launches (svmc_payoff_sums_chain); expiry i reads
        snapshot row snap_rows[i] (and qvar_rows[i]) and the recentring sums at spot_sums_ptr + 16 i"""
        m = len(strikes)
        offs = np.concatenate([[0], np.cumsum([len(k) for k in strikes])]).astype(np.uintp)
        if int(offs[-1]) == 0:
            return
        k_all = np.ascontiguousarray(np.concatenate(strikes), dtype=np.float64)
        c_all = np.ascontiguousarray(np.concatenate(codes), dtype=np.int8)
        s_all = np.ascontiguousarray(np.concatenate(shifts), dtype=np.float64)
        fw = np.ascontiguousarray(forwards, dtype=np.float64)
        tt = np.ascontiguousarray(ttms, dtype=np.float64)
        xs = (C.c_void_p * m)(*[self.snapshot_ptr(r) for r in snap_rows])
        qs = None if qvar_rows is None else (C.c_void_p * m)(*[self.snapshot_ptr(r) for r in qvar_rows])
        _lib.check(self.lib.svmc_payoff_sums_chain(
            xs, qs, self.n_path, ptr(fw), ptr(tt), spot_sums_ptr, m, ptr(k_all),
            ptr(c_all), ptr(s_all), offs.ctypes.data_as(C.POINTER(C.c_size_t)),
            int(variable_type), out_ptr, self.ws.ptr, self.ws_bytes, self.stream))

    def tilted_payoffs(self, forwards, strikes: Sequence[np.ndarray], codes: Sequence[np.ndarray], gammas, recenter: bool = False,
                       snap_rows: Optional[Sequence[int]] = None):
        """prices under the exponential risk-premia kernel exp(gamma x) (svmc_tilted_payoff_chain, include/svmc.h) of the
        resident log-returns, whichever generator left them: expiry i reads snapshot row snap_rows[i], or, with snap_rows None,
        the one expiry reads the current state x.  codes: 0 ('C') / 1 ('P') per strike.  Returns (prices [G][m] -> [K_i],
        stderrs the same, stats [G, m, TILTED_STATS_FIELDS]) for the G gammas; one download."""
        ch = tilted_chain_arrays(forwards, strikes, codes, gammas)
        m, K, G = ch["m"], ch["total"], ch["gammas"].size
        if (m != 1) if snap_rows is None else (len(snap_rows) != m):
            raise ValueError("one snapshot row per expiry (the current state serves one expiry)")
        ptrs = [self.x.ptr] if snap_rows is None else [self.snapshot_ptr(r) for r in snap_rows]
        shifts = np.ascontiguousarray(np.concatenate([payoff_shifts(k, c, float(f), LOG_RETURN)
                                                      for k, c, f in zip(ch["strikes_ttms"], ch["codes_ttms"], ch["forwards"])]))
        spot_ptr = None
        if recenter:
            spot_ptr, _ = self.alloc_sums(2 * m, "tilted_spot")
            for i, p in enumerate(ptrs):
                self.spot_sums(p, float(ch["forwards"][i]), spot_ptr + 16 * i)
        n_out = 2 * G * K + G * m * TILTED_STATS_DOUBLES
        out_ptr, _ = self.alloc_sums(n_out, "tilted")
        xs, a = (C.c_void_p * m)(*ptrs), ch["args"]
        _lib.check(self.lib.svmc_tilted_payoff_chain(
            xs, self.n_path, *a[:4], ptr(shifts), a[4], *ch["gamma_args"], int(bool(recenter)), spot_ptr, out_ptr, out_ptr + 8 * G * K,
            out_ptr + 16 * G * K, self.ws.ptr, self.ws_bytes, self.stream))
        out = self.download(out_ptr, n_out)
        return tilted_results(out[:G * K], out[G * K:2 * G * K], out[2 * G * K:], ch)

    # ---- conditional Monte Carlo (include/svmc.h, svmc_cmc.hip): the state is (mu, cv, sigma | var, qvar), mu in self.x ---------
    @property
    def cv(self) -> DeviceBuffer:
        """the fourth state array of the conditional generators, allocated on first use"""
        if self._cv is None:
            self._cv = DeviceBuffer(self.n_path)
        return self._cv

    def set_state_cmc(self, mu: np.ndarray, cv: np.ndarray, vol: np.ndarray, qvar: np.ndarray) -> None:
        self.set_state(mu, vol, qvar)
        a = np.ascontiguousarray(cv, dtype=np.float64)
        assert a.shape == (self.n_path,)
        self.upload(self.cv.ptr, a)

    def fill_state_cmc(self, mu0: float, vol0: float, qvar0: float) -> None:
        """fill_state with the conditional variance at 0: what a conditional chain pricing begins with"""
        self.fill_state(mu0, vol0, qvar0)
        _lib.check(self.lib.svmc_memset(self.cv.ptr, 0, 8 * self.n_path, self.stream))

    def get_state_cmc(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        mu, vol, qvar = self.get_state()
        return mu, self.download(self.cv.ptr, self.n_path), vol, qvar

    def _cmc_rows(self, n: int, mu_row: int, cv_row: int, qvar_row: Optional[int]):
        self.reserve_snapshots(max(mu_row, cv_row, -1 if qvar_row is None else qvar_row) + n)
        return (self.snapshot_ptr(mu_row), self.snapshot_ptr(cv_row), None if qvar_row is None else self.snapshot_ptr(qvar_row))

    def logsv_chain_cmc(self, nb_steps: Sequence[int], dts: Sequence[float], etas: Sequence[float], theta, kappa1, kappa2, beta,
                        volvol, is_spot_measure, seed, call_id, step_offset: int = 0, mu_row: int = 0,
                        cv_row: Optional[int] = None, qvar_row: Optional[int] = None) -> None:
        """svmc_logsv_chain_cmc on this engine's (mu, cv, sigma, qvar): expiry i's mu and cv go to snapshot rows mu_row + i and
        cv_row + i (default: right after the mu rows), its qvar to qvar_row + i when asked"""
        n = len(nb_steps)
        cv_row = mu_row + n if cv_row is None else cv_row
        nb = np.ascontiguousarray(nb_steps, dtype=np.int32)
        dt, et = np.ascontiguousarray(dts, dtype=np.float64), np.ascontiguousarray(etas, dtype=np.float64)
        rows = self._cmc_rows(n, mu_row, cv_row, qvar_row)
        self._timed("logsv_chain_cmc_kernel", lambda: _lib.check(self.lib.svmc_logsv_chain_cmc(
            self.x.ptr, self.cv.ptr, self.vol.ptr, self.qvar.ptr, self.n_path, n, ptr(nb),
            ptr(dt), ptr(et), float(theta), float(kappa1), float(kappa2), float(beta), float(volvol),
            int(bool(is_spot_measure)), int(seed), int(call_id), self.path_offset, int(step_offset), *rows, self.stream)))

    def heston_chain_cmc(self, nb_steps: Sequence[int], dts: Sequence[float], theta, kappa, rho, volvol, seed, call_id,
                         step_offset: int = 0, mu_row: int = 0, cv_row: Optional[int] = None,
                         qvar_row: Optional[int] = None) -> None:
        """svmc_heston_chain_cmc (the reference's Euler step) on this engine's (mu, cv, var, qvar); rows as logsv_chain_cmc"""
        n = len(nb_steps)
        cv_row = mu_row + n if cv_row is None else cv_row
        nb = np.ascontiguousarray(nb_steps, dtype=np.int32)
        dt = np.ascontiguousarray(dts, dtype=np.float64)
        rows = self._cmc_rows(n, mu_row, cv_row, qvar_row)
        self._timed("heston_chain_cmc_kernel", lambda: _lib.check(self.lib.svmc_heston_chain_cmc(
            self.x.ptr, self.cv.ptr, self.vol.ptr, self.qvar.ptr, self.n_path, n, ptr(nb),
            ptr(dt), float(theta), float(kappa), float(rho), float(volvol), int(seed), int(call_id),
            self.path_offset, int(step_offset), *rows, self.stream)))

    def _cond_row_ptrs(self, m: int, mu_rows, cv_rows):
        """the device pointers of the (mu, cv) rows of m expiries: snapshot rows mu_rows[i] and cv_rows[i], or, with both None, the
        current state (x, cv) for the one expiry"""
        if (mu_rows is None) != (cv_rows is None) or ((m != 1) if mu_rows is None else (len(mu_rows) != m or len(cv_rows) != m)):
            raise ValueError("one mu row and one cv row per expiry (the current state serves one expiry)")
        mus = [self.x.ptr] if mu_rows is None else [self.snapshot_ptr(r) for r in mu_rows]
        cvs = [self.cv.ptr] if cv_rows is None else [self.snapshot_ptr(r) for r in cv_rows]
        return mus, cvs

    def _side_workspace(self, size_fn, size_args: tuple, tag: str, what: Optional[str] = None):
        """(device pointer, bytes) of the workspace size_fn(*size_args, &bytes) asks for, in this engine's `tag` buffer; what: the
        entry's name for a tail of libsvmc_ext.so / libsvmc_est.so, which keep no message of their own (_lib.check_ext)"""
        nbytes = C.c_size_t(0)
        rc = size_fn(*size_args, C.byref(nbytes))
        _lib.check(rc) if what is None else _lib.check_ext(rc, what)
        ws_ptr, _ = self.alloc_sums((nbytes.value + 7) // 8, tag)
        return ws_ptr, nbytes.value

    def conditional_payoffs(self, forwards, discfactors, strikes: Sequence[np.ndarray], codes: Sequence[np.ndarray],
                            recenter: bool = True, mu_rows: Optional[Sequence[int]] = None,
                            cv_rows: Optional[Sequence[int]] = None):
        """the conditional estimator (svmc_cmc_payoff_chain, include/svmc.h) on resident (mu, cv): expiry i reads snapshot rows
        mu_rows[i] and cv_rows[i], or, with both None, the one expiry reads the current state.  codes: 0 ('C') / 1 ('P') per
        strike.  Returns (prices [m] -> [K_i], stderrs the same, stats [m] dicts of CMC_STATS_FIELDS)."""
        ch = marshalled_chain(np.zeros(len(strikes)), forwards, discfactors, strikes, codes)
        m, K = ch["m"], ch["total"]
        mus, cvs = self._cond_row_ptrs(m, mu_rows, cv_rows)
        ws_ptr, nbytes = self._side_workspace(self.lib.svmc_cmc_payoff_workspace_bytes, (self.n_path, m, K), "cmc_workspace")
        res, stats = np.empty((2, max(K, 1))), np.empty((m, CMC_STATS_DOUBLES))
        _lib.check(self.lib.svmc_cmc_payoff_chain(
            (C.c_void_p * m)(*mus), (C.c_void_p * m)(*cvs), self.n_path, *ch["args"][1:], int(bool(recenter)), row_ptr(res, 0),
            row_ptr(res, 1), ptr(stats), ws_ptr, nbytes, self.stream))
        return expiry_rows(res, ch["slices"]) + (cmc_stats_dicts(stats),)

    # ---- conditional Monte Carlo under the exponential risk-premia kernel (include/svmc_ext.h): libsvmc_ext.so,
    # the library beside the closed core -- caller-owned device rows, no session
    def tilted_conditional_payoffs(self, forwards, strikes: Sequence[np.ndarray], codes: Sequence[np.ndarray], gammas,
                                   recenter: bool = False, mu_rows: Optional[Sequence[int]] = None,
                                   cv_rows: Optional[Sequence[int]] = None, shifts: Optional[Sequence[np.ndarray]] = None):
        """the conditional estimator under exp(gamma x) (svmc_tilted_cond_payoff_chain, include/svmc_ext.h) on resident (mu, cv),
        whichever generator left them: expiry i reads snapshot rows mu_rows[i] and cv_rows[i], or, with both None, the one expiry
        reads the current state (x, cv).  codes: 0 ('C') / 1 ('P') per strike.  shifts: the host constant of every strike's sums
        (default: the intrinsic value at the forward, as tilted_payoffs; any finite value gives the same estimate).  Returns as
        tilted_payoffs: (prices [G][m] -> [K_i], stderrs the same, stats [G, m, TILTED_COND_STATS_FIELDS]); prices are undiscounted."""
        ch = tilted_chain_arrays(forwards, strikes, codes, gammas)
        m, K, G = ch["m"], ch["total"], ch["gammas"].size
        mus, cvs = self._cond_row_ptrs(m, mu_rows, cv_rows)
        sh = strike_shifts(ch, shifts)
        ext = _lib.load_ext()
        what = "svmc_tilted_cond_payoff_chain"
        ws_ptr, nbytes = self._side_workspace(ext.svmc_tilted_cond_workspace_bytes, (self.n_path, m, K, G), "tilted_cond_workspace", what)
        prices, stderrs, stats = np.empty(max(G * K, 1)), np.empty(max(G * K, 1)), np.empty(G * m * TILTED_STATS_DOUBLES)
        a = ch["args"]
        self._timed("tilted_cond_payoff_kernel", lambda: _lib.check_ext(ext.svmc_tilted_cond_payoff_chain(
            (C.c_void_p * m)(*mus), (C.c_void_p * m)(*cvs), self.n_path, *a[:4], ptr(sh), a[4], *ch["gamma_args"], int(bool(recenter)),
            ptr(prices), ptr(stderrs), ptr(stats), ws_ptr, nbytes, self.stream), what))
        return tilted_results(prices[:G * K], stderrs[:G * K], stats, ch)

    def tilted_conditional_greeks(self, forwards, strikes: Sequence[np.ndarray], codes: Sequence[np.ndarray], gammas,
                                  recenter: bool = False, mu_rows: Optional[Sequence[int]] = None,
                                  cv_rows: Optional[Sequence[int]] = None):
        """delta, dual delta, gamma and dual gamma of tilted_conditional_payoffs' prices, each with its error
        (svmc_tilted_cond_greeks_chain, include/svmc_est.h: libsvmc_est.so) on the same resident (mu, cv): expiry i reads snapshot
        rows mu_rows[i] and cv_rows[i], or, with both None, the one expiry reads the current state (x, cv).  Returns ([G] dicts
        {field of TCG_FIELDS: [m] -> [K_i]}, stats [G, m, TCG_STATS_FIELDS]); undiscounted.  Price and error are the payoff
        tail's: call tilted_conditional_payoffs on the same rows."""
        ch = tilted_chain_arrays(forwards, strikes, codes, gammas)
        m, K, G = ch["m"], ch["total"], ch["gammas"].size
        mus, cvs = self._cond_row_ptrs(m, mu_rows, cv_rows)
        est = _lib.load_est()
        what = "svmc_tilted_cond_greeks_chain"
        ws_ptr, nbytes = self._side_workspace(est.svmc_tilted_cond_greeks_workspace_bytes, (self.n_path, m, K, G),
                                              "tilted_cond_greeks_workspace", what)
        greeks, stats = np.empty(max(G * TCG_ROWS * K, 1)), np.empty(G * m * TCG_STATS_DOUBLES)
        self._timed("tilted_cond_greeks_kernel", lambda: _lib.check_ext(est.svmc_tilted_cond_greeks_chain(
            (C.c_void_p * m)(*mus), (C.c_void_p * m)(*cvs), self.n_path, *ch["args"], *ch["gamma_args"], int(bool(recenter)),
            ptr(greeks), ptr(stats), ws_ptr, nbytes, self.stream), what))
        return tilted_greeks_results(greeks, stats, ch)

    def conditional_densities(self, x_grids: Sequence[np.ndarray], gammas=(0.0,), mu_rows: Optional[Sequence[int]] = None,
                              cv_rows: Optional[Sequence[int]] = None):
        """the mixture density of the log-return at the points of x_grids, under exp(gamma x) for every gamma
        (svmc_cond_density_chain, include/svmc_est.h: libsvmc_est.so) on resident (mu, cv), whichever generator
        left them: expiry i reads snapshot rows mu_rows[i] and cv_rows[i], or, with both None, the one expiry reads the current
        state (x, cv).  Returns (pdf [G][m] -> x_i's shape, stderr likewise, stats [G, m, CD_STATS_FIELDS]).  A gamma with
        n_weight_dropped > 0 has NaN for its pdf and its error."""
        ch = cond_density_arrays(x_grids, gammas)
        m, P, G = ch["m"], ch["total"], ch["gammas"].size
        mus, cvs = self._cond_row_ptrs(m, mu_rows, cv_rows)
        est = _lib.load_est()
        what = "svmc_cond_density_chain"
        ws_ptr, nbytes = self._side_workspace(est.svmc_cond_density_workspace_bytes, (self.n_path, m, P, G), "cond_density_workspace", what)
        pdf, err, stats = np.empty(max(G * P, 1)), np.empty(max(G * P, 1)), np.empty(G * m * CD_STATS_DOUBLES)
        self._timed("cond_density_kernel", lambda: _lib.check_ext(est.svmc_cond_density_chain(
            (C.c_void_p * m)(*mus), (C.c_void_p * m)(*cvs), self.n_path, m, ptr(ch["points"]),
            ch["offs"].ctypes.data_as(C.POINTER(C.c_size_t)), ptr(ch["gammas"]), G, ptr(pdf), ptr(err), ptr(stats), ws_ptr, nbytes,
            self.stream), what))
        offs = ch["offs"]
        cut = lambda a: [[a[g * P + int(offs[i]):g * P + int(offs[i + 1])].reshape(ch["shapes"][i]).copy()    # noqa: E731
                          for i in range(m)] for g in range(G)]
        return cut(pdf), cut(err), stats.reshape(G, m, CD_STATS_DOUBLES)

    def step_hawkesjd_chain_cond_rows(self, ch: dict, params: np.ndarray, nb_steps_per_year: int, seed: int, call_id: int) -> None:
        """hawkesjd_chain_cond from the origin (0, lambda_p, lambda_m) into snapshot rows [0, m) (mu) and [m, 2m) (cv) for the
        expiries of ch (tilted_chain_arrays with ttms).  The step grid is the fused drivers' (svmc_chain.hip expiry_grids), so the
        mu rows are those svmc_hawkesjd_chain_price_cmc steps at this seed."""
        nbs, dts = chain_step_grid(ch["ttms"], nb_steps_per_year)
        self.fill_state(0.0, float(params[6]), float(params[11]))         # SVMC_HAWKESJD_PARAMS: lambda_p, lambda_m
        self.hawkesjd_chain_cond(nbs, dts, params, seed, call_id, mu_row=0, cv_row=ch["m"])

    # ---- many (sigma, gamma) sets on one set of jump rows (include/svmc_est.h): libsvmc_est.so
    def step_hawkesjd_jump_rows(self, ch: dict, params: np.ndarray, nb_steps_per_year: int, seed: int, call_id: int) -> None:
        """step_hawkesjd_chain_cond_rows with the parameter block's sigma set to 0.0: snapshot rows [0, m) hold a_j -- drift,
        compensators and jumps, which depend on neither sigma nor gamma -- and rows [m, 2m) zeros.  The jumps are those of
        step_hawkesjd_chain_cond_rows at this (seed, call id) whatever its sigma."""
        block = np.array(params, dtype=np.float64)
        block[1] = 0.0                                                     # SVMC_HAWKESJD_PARAMS: sigma
        self.step_hawkesjd_chain_cond_rows(ch, block, nb_steps_per_year, seed, call_id)

    def copy_rows(self, dst_ptr: int, src_ptr: int, n_doubles: int) -> None:
        """n_doubles from one device address to another on this engine's stream"""
        _lib.check(self.lib.svmc_memcpy_d2d(dst_ptr, src_ptr, 8 * int(n_doubles), self.stream))

    def jump_sets_payoffs(self, forwards, strikes: Sequence[np.ndarray], codes: Sequence[np.ndarray], variances, gammas,
                          recenter: bool = False, a_rows: Optional[Sequence[int]] = None,
                          shifts: Optional[Sequence[np.ndarray]] = None, a_ptrs: Optional[Sequence[int]] = None):
        """the conditional estimator under exp(gamma x) for up to JUMP_SETS_MAX sets (gamma_q, v_qi) on rows a with
        x | a ~ N(a - v / 2, v), v the same on every path (svmc_jump_sets_payoff_chain, include/svmc_est.h): expiry i reads snapshot
        row a_rows[i], or the device pointer a_ptrs[i] of a caller-owned row of n_path doubles, or, with both None, the one expiry
        reads the current state x.  variances: [Q][m], gammas: [Q].  codes: 0 ('C') / 1 ('P') per strike.  shifts: the host constant
        of every strike's sums, shared by the sets (default payoff_shifts at the forward).  Returns (prices [Q][m] -> [K_i], stderrs
        the same, stats [Q, m, TILTED_COND_STATS_FIELDS], corr [m]); prices are undiscounted."""
        ch = tilted_chain_arrays(forwards, strikes, codes, gammas)
        m, K, Q = ch["m"], ch["total"], ch["gammas"].size
        var = np.ascontiguousarray(np.asarray(variances, dtype=np.float64))
        if var.shape != (Q, m):
            raise ValueError("variances: one per (set, expiry)")
        if not (np.all(np.isfinite(var)) and np.all(var >= 0.0)):
            raise ValueError("variances must be finite and not negative")
        if a_rows is not None and a_ptrs is not None:
            raise ValueError("a_rows or a_ptrs, not both")
        if a_ptrs is not None:
            ptrs = [int(p) for p in a_ptrs]
        elif a_rows is not None:
            ptrs = [self.snapshot_ptr(r) for r in a_rows]
        else:
            ptrs = [self.x.ptr]
        if len(ptrs) != m:
            raise ValueError("one row of a per expiry (the current state serves one expiry)")
        sh = strike_shifts(ch, shifts)
        est = _lib.load_est()
        what = "svmc_jump_sets_payoff_chain"
        ws_ptr, nbytes = self._side_workspace(est.svmc_jump_sets_workspace_bytes, (self.n_path, m, K, Q), "jump_sets_workspace", what)
        prices, stderrs = np.empty(max(Q * K, 1)), np.empty(max(Q * K, 1))
        stats, corr = np.empty(Q * m * TILTED_STATS_DOUBLES), np.empty(m)
        a = ch["args"]
        self._timed("jump_sets_payoff_kernel", lambda: _lib.check_ext(est.svmc_jump_sets_payoff_chain(
            (C.c_void_p * m)(*ptrs), self.n_path, *a[:4], ptr(sh), a[4], ptr(var), *ch["gamma_args"], int(bool(recenter)), ptr(prices),
            ptr(stderrs), ptr(stats), ptr(corr), ws_ptr, nbytes, self.stream), what))
        return tilted_results(prices[:Q * K], stderrs[:Q * K], stats, ch) + (corr,)

    def price_hawkesjd_chain_tilted_cond(self, ch: dict, params: np.ndarray, nb_steps_per_year: int, seed: int, call_id: int, gammas,
                                         recenter: bool):
        """the Hawkes chain by conditional Monte Carlo under the risk-premia kernel for every gamma from ONE stepping launch (ch:
        tilted_chain_arrays with ttms): step_hawkesjd_chain_cond_rows, then tilted_conditional_payoffs on the rows.  TWO C calls:
        there is no fused session entry, because sessions belong to the closed core (libsvmc.so, 143 entry points) and the tail
        lives in libsvmc_ext.so."""
        params = np.ascontiguousarray(params, dtype=np.float64)
        m = ch["m"]
        self.step_hawkesjd_chain_cond_rows(ch, params, nb_steps_per_year, seed, call_id)
        return self.tilted_conditional_payoffs(ch["forwards"], [k.reshape(s) for k, s in zip(ch["strikes_ttms"], ch["shapes"])],
                                               ch["codes_ttms"], gammas, recenter, mu_rows=list(range(m)),
                                               cv_rows=list(range(m, 2 * m)))

    def price_hawkesjd_chain_tilted_cond_greeks(self, ch: dict, params: np.ndarray, nb_steps_per_year: int, seed: int, call_id: int,
                                                gammas, recenter: bool):
        """price_hawkesjd_chain_tilted_cond with the derivatives of its prices in the forward and the strike: ONE
        stepping call for all gammas, then the two tails on the same rows -- svmc_tilted_cond_payoff_chain (libsvmc_ext.so: price,
        error, statistics) and svmc_tilted_cond_greeks_chain (libsvmc_est.so).  Returns ([G] dicts {field of CMC_GREEKS_FIELDS:
        [m] -> [K_i] in the strikes' shapes}, stats [G, m, TILTED_COND_GREEKS_STATS_FIELDS])."""
        params = np.ascontiguousarray(params, dtype=np.float64)
        m = ch["m"]
        self.step_hawkesjd_chain_cond_rows(ch, params, nb_steps_per_year, seed, call_id)
        strikes = [k.reshape(s) for k, s in zip(ch["strikes_ttms"], ch["shapes"])]
        rows = dict(mu_rows=list(range(m)), cv_rows=list(range(m, 2 * m)))
        prices, stderrs, stats = self.tilted_conditional_payoffs(ch["forwards"], strikes, ch["codes_ttms"], gammas, recenter, **rows)
        greeks, gstats = self.tilted_conditional_greeks(ch["forwards"], strikes, ch["codes_ttms"], gammas, recenter, **rows)
        out = [dict(price=p, stderr=e, **g) for p, e, g in zip(prices, stderrs, greeks)]
        return out, np.concatenate([stats, gstats[:, :, 3:4]], axis=2)

    def price_logsv_chain_cmc_fused(self, ch: dict, v0, theta, kappa1, kappa2, beta, volvol, etas, is_spot_measure,
                                    nb_steps_per_year, recenter: bool, seed: int, call_id: int):
        """logsv_mc_chain_pricer_conditional as ONE svmc_logsv_chain_price_cmc call on this engine's state; returns (prices,
        stderrs, stats) cut into expiries"""
        return self._price_chain_fused(ch, "logsv", "_cmc", (v0, theta, kappa1, kappa2, beta, volvol, etas, is_spot_measure),
                                       nb_steps_per_year, int(bool(recenter)), seed, call_id)

    def price_heston_chain_cmc_fused(self, ch: dict, v0, theta, kappa, rho, volvol, nb_steps_per_year, recenter: bool, seed: int,
                                     call_id: int):
        """heston_mc_chain_pricer_conditional as ONE svmc_heston_chain_price_cmc call on this engine's state"""
        return self._price_chain_fused(ch, "heston", "_cmc", (v0, theta, kappa, rho, volvol), nb_steps_per_year, int(bool(recenter)),
                                       seed, call_id)

    # ---- conditional Monte Carlo Greeks (include/svmc.h): delta, dual delta, gamma, dual gamma ----------------
    def conditional_greeks(self, forwards, discfactors, strikes: Sequence[np.ndarray], codes: Sequence[np.ndarray],
                           recenter: bool = True, mu_rows: Optional[Sequence[int]] = None,
                           cv_rows: Optional[Sequence[int]] = None):
        """svmc_cmc_greeks_chain on resident (mu, cv), rows as conditional_payoffs.  Returns ({field of CMC_GREEKS_FIELDS: [m] ->
        [K_i]}, stats [m] dicts of CMC_GREEKS_STATS_FIELDS)."""
        ch = marshalled_chain(np.zeros(len(strikes)), forwards, discfactors, strikes, codes)
        m, K = ch["m"], ch["total"]
        mus, cvs = self._cond_row_ptrs(m, mu_rows, cv_rows)
        ws_ptr, nbytes = self._side_workspace(self.lib.svmc_cmc_greeks_workspace_bytes, (self.n_path, m, K), "cmc_greeks_workspace")
        res, stats = np.empty((CMC_GREEKS_ROWS, max(K, 1))), np.empty((m, CMC_GREEKS_STATS_DOUBLES))
        _lib.check(self.lib.svmc_cmc_greeks_chain(
            (C.c_void_p * m)(*mus), (C.c_void_p * m)(*cvs), self.n_path, *ch["args"][1:], int(bool(recenter)), ptr(res), ptr(stats),
            ws_ptr, nbytes, self.stream))
        return cmc_greeks_dict(res, ch["slices"]), cmc_greeks_stats_dicts(stats)

    def price_logsv_chain_cmc_greeks_fused(self, ch: dict, v0, theta, kappa1, kappa2, beta, volvol, etas, is_spot_measure,
                                           nb_steps_per_year, recenter: bool, seed: int, call_id: int):
        """logsv_mc_chain_greeks_conditional as ONE svmc_logsv_chain_price_cmc_greeks call on this engine's state; returns
        (fields, stats) as conditional_greeks"""
        return self._price_chain_fused(ch, "logsv", "_cmc_greeks", (v0, theta, kappa1, kappa2, beta, volvol, etas, is_spot_measure),
                                       nb_steps_per_year, int(bool(recenter)), seed, call_id)

    def price_heston_chain_cmc_greeks_fused(self, ch: dict, v0, theta, kappa, rho, volvol, nb_steps_per_year, recenter: bool,
                                            seed: int, call_id: int):
        """heston_mc_chain_greeks_conditional as ONE svmc_heston_chain_price_cmc_greeks call on this engine's state"""
        return self._price_chain_fused(ch, "heston", "_cmc_greeks", (v0, theta, kappa, rho, volvol), nb_steps_per_year,
                                       int(bool(recenter)), seed, call_id)

    # ---- many conditional jobs in one stepping launch and the parameter sensitivities (include/svmc.h) ---------
    def chain_cmc_many(self, model: str, nb_steps: Sequence[int], dts: Sequence[float], params: np.ndarray, seeds: Sequence[int],
                       call_ids: Sequence[int], mode: int = 1, mu_row: int = 0) -> None:
        """svmc_logsv_chain_cmc_many (model "logsv", mode = is_spot_measure, params [J][6 + m]) or svmc_heston_chain_cmc_many
        ("heston", params [J][5]): expiry i of job j goes to snapshot rows mu_row + j m + i (mu) and mu_row + (J + j) m + i (cv)"""
        fn, modes = self._model_entry("chain_cmc_many", model, "chain_cmc_many", CMC_MODELS, mode, _flag)
        n_jobs, jobs = self._many_jobs(params, seeds, call_ids)
        m = len(nb_steps)
        nb = np.ascontiguousarray(nb_steps, dtype=np.int32)
        dt = np.ascontiguousarray(dts, dtype=np.float64)
        self.reserve_snapshots(mu_row + 2 * n_jobs * m)
        ws_ptr, nbytes = self._side_workspace(self.lib.svmc_cmc_many_workspace_bytes, (n_jobs, m), "cmc_many_table")
        _lib.check(fn(self.n_path, n_jobs, m, ptr(nb), ptr(dt), jobs[0], *modes, jobs[1], jobs[2], self.path_offset,
                      self.snapshot_ptr(mu_row), self.snapshot_ptr(mu_row + n_jobs * m), ws_ptr, nbytes, self.stream))

    def conditional_sens(self, forwards, discfactors, strikes: Sequence[np.ndarray], codes: Sequence[np.ndarray], steps,
                         recenter: bool = True, up_rows=None, dn_rows=None, host_rows=None):
        """the sensitivity tail (svmc_cmc_sens_chain) on resident (mu, cv): parameter p's up job reads snapshot rows up_rows[p] =
        (mu rows [m], cv rows [m]), its dn job dn_rows[p].  host_rows = (mu_up, cv_up, mu_dn, cv_dn), each [P][m] host arrays,
        instead: uploaded to snapshot rows first.  Returns sens [P][CMC_SENS_ROWS][K] and the chain's slices."""
        ch = marshalled_chain(np.zeros(len(strikes)), forwards, discfactors, strikes, codes)
        m, K = ch["m"], ch["total"]
        h = np.ascontiguousarray(np.atleast_1d(np.asarray(steps, dtype=np.float64))).ravel()
        P = h.size
        if host_rows is not None:
            self.reserve_snapshots(4 * P * m)
            for a, block in enumerate(host_rows):                          # block a's job p sits in rows (a P + p) m ...
                if len(block) != P or any(len(job) != m for job in block):
                    raise ValueError("one host array per (parameter, expiry) for each of mu_up, cv_up, mu_dn, cv_dn")
                self._upload_snapshot_rows([x for job in block for x in job], a * P * m)
            job_rows = lambda a, p: list(range((a * P + p) * m, (a * P + p + 1) * m))               # noqa: E731
            up_rows = [(job_rows(0, p), job_rows(1, p)) for p in range(P)]
            dn_rows = [(job_rows(2, p), job_rows(3, p)) for p in range(P)]
        if up_rows is None or dn_rows is None or len(up_rows) != P or len(dn_rows) != P or \
                any(len(mu) != m or len(cv) != m for mu, cv in list(up_rows) + list(dn_rows)):
            raise ValueError("one mu row and one cv row per expiry for each up / dn job of the P steps")
        ptrs = lambda which, jobs: (C.c_void_p * max(P * m, 1))(*[self.snapshot_ptr(r) for job in jobs for r in job[which]])  # noqa: E731
        ws_ptr, nbytes = self._side_workspace(self.lib.svmc_cmc_sens_workspace_bytes, (self.n_path, m, K, P), "cmc_sens_workspace")
        sens = np.empty((max(P, 1), CMC_SENS_ROWS, max(K, 1)))
        _lib.check(self.lib.svmc_cmc_sens_chain(
            ptrs(0, up_rows), ptrs(1, up_rows), ptrs(0, dn_rows), ptrs(1, dn_rows), self.n_path, *ch["args"][1:], P, ptr(h),
            int(bool(recenter)), ptr(sens), ws_ptr, nbytes, self.stream))
        return sens[:P, :, :K], ch["slices"]

    def _upload_snapshot_rows(self, arrays, first_row: int) -> None:
        """host arrays of one value per path into consecutive snapshot rows from first_row (reserved by the caller)"""
        for r, x in enumerate(arrays, first_row):
            a = np.ascontiguousarray(x, dtype=np.float64)
            if a.shape != (self.n_path,):
                raise ValueError("a host row must hold one value per path of the engine")
            self.upload(self.snapshot_ptr(r), a)

    def price_chain_cmc_many_fused(self, ch: dict, model: str, params: np.ndarray, seeds: Sequence[int], call_ids: Sequence[int],
                                   mode: int, nb_steps_per_year: int, recenter: bool):
        """J conditional jobs of one chain as ONE svmc_logsv_chain_price_cmc_many (model "logsv", mode = is_spot_measure, params
        [J][6 + m]) or svmc_heston_chain_price_cmc_many ("heston", params [J][5]) call on this engine's session, J at most
        MANY_MAX_JOBS: per job the (prices, stderrs, stats) of the single fused call with its (seed, call id)"""
        fn, modes = self._model_entry("price_chain_cmc_many_fused", model, "chain_price_cmc_many", CMC_MODELS, mode, _flag)
        n_jobs, jobs = self._many_jobs(params, seeds, call_ids)
        res, stats = np.empty((2, n_jobs, max(ch["total"], 1))), np.empty((n_jobs, ch["m"], CMC_STATS_DOUBLES))
        self._session_call(ch, lambda sess: fn(
            sess, *ch["args"], n_jobs, *jobs, *modes, int(nb_steps_per_year), int(bool(recenter)), row_ptr(res, 0), row_ptr(res, 1),
            ptr(stats)), f"{model}_chain_cond_many_kernel")
        return [rows + (cmc_stats_dicts(st),) for rows, st in zip(expiry_rows_per_job(res, ch["slices"]), stats)]

    def price_chain_cmc_sens_fused(self, ch: dict, model: str, rows: np.ndarray, steps: np.ndarray, mode: int, nb_steps_per_year: int,
                                   recenter: bool, seed: int, call_id: int):
        """svmc_logsv_chain_price_cmc_sens (model "logsv", mode = is_spot_measure, rows [1 + 2P][6 + m]) or
        svmc_heston_chain_price_cmc_sens ("heston", rows [1 + 2P][5]) on this engine's session: the job table's rows on ONE (seed,
        call id).  Returns (fields, stats) as conditional_greeks for the base job, and sens [P][CMC_SENS_ROWS][K]."""
        fn, modes = self._model_entry("price_chain_cmc_sens_fused", model, "chain_price_cmc_sens", CMC_MODELS, mode, _flag)
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        h = np.ascontiguousarray(steps, dtype=np.float64).ravel()
        P, K = h.size, max(ch["total"], 1)
        if rows.ndim != 2 or rows.shape[0] != 1 + 2 * P:
            raise ValueError("the job table has one base row and an up and a dn row per step")
        res, stats = np.empty((CMC_GREEKS_ROWS, K)), np.empty((ch["m"], CMC_GREEKS_STATS_DOUBLES))
        sens = np.empty((max(P, 1), CMC_SENS_ROWS, K))
        self._session_call(ch, lambda sess: fn(
            sess, *ch["args"], P, ptr(rows), ptr(h), *modes, int(nb_steps_per_year), int(bool(recenter)), int(seed), int(call_id),
            ptr(res), ptr(stats), ptr(sens)), f"{model}_chain_cond_many_kernel")
        return cmc_greeks_dict(res, ch["slices"]), cmc_greeks_stats_dicts(stats), sens[:P]

    # ---- the conditional calibration objective: parameter sets of one chain on one replayed graph (include/svmc.h, row f15) ------
    def price_chain_cmc_sets_fused(self, ch: dict, model: str, params: np.ndarray, mode: int, nb_steps_per_year: int, recenter: bool,
                                   seed: int, call_id: int, want_ivols: bool = True):
        """up to CMC_SETS_MAX parameter sets of one chain on ONE (seed, call id) as one svmc_logsv_chain_price_cmc_sets (model
        "logsv", mode = is_spot_measure, params [P][6 + m]) or svmc_heston_chain_price_cmc_sets ("heston", params [P][5]) call on
        this engine's session -- one graph replay.  Per set (prices, stderrs, ivols or None, stats), the first three cut into
        expiries; ch is marshalled once per chain content (marshalled_chain)."""
        fn, modes = self._model_entry("price_chain_cmc_sets_fused", model, "chain_price_cmc_sets", CMC_MODELS, mode, _flag)
        params = np.ascontiguousarray(params, dtype=np.float64)
        if params.ndim != 2 or params.shape[1] != (6 + ch["m"] if model == "logsv" else 5):
            raise ValueError("one row per parameter set: [6 + n_expiries] for logsv, [5] for heston")
        P, K = params.shape[0], max(ch["total"], 1)
        res, stats = np.empty((3 if want_ivols else 2, P, K)), np.empty((P, ch["m"], CMC_STATS_DOUBLES))
        sess = self.fused_chain_session(ch["m"], ch["total"])
        _lib.check(fn(sess, *ch["args"], P, ptr(params), *modes, int(nb_steps_per_year), int(bool(recenter)), int(seed), int(call_id),
                      row_ptr(res, 0), row_ptr(res, 1), ptr(stats), row_ptr(res, 2) if want_ivols else None))
        return [rows[:2] + (rows[2] if want_ivols else None, cmc_stats_dicts(st))
                for rows, st in zip(expiry_rows_per_job(res, ch["slices"]), stats)]

    def use_graphs(self, enable: bool) -> None:
        """whether the fused session's graph drivers replay a captured graph (default) or issue their launches directly"""
        self._fused_graphs = bool(enable)
        if self._fused is not None:
            _lib.check(self.lib.svmc_session_use_graphs(self._fused, int(self._fused_graphs)))

    def graph_launches(self) -> int:
        """how many calls on the fused session were hipGraph replays (diagnostics; a regrown session starts at 0)"""
        if self._fused is None:
            return 0
        n = C.c_size_t()
        _lib.check(self.lib.svmc_session_graph_launches(self._fused, C.byref(n)))
        return int(n.value)

    # ---- Monte Carlo chain Greeks on common random numbers (include/svmc.h, svmc_greeks.hip) ------------------------------------
    def greeks_payoffs(self, forwards, discfactors, strikes: Sequence[np.ndarray], codes: Sequence[np.ndarray], steps=(),
                       base_rows: Optional[Sequence[int]] = None, up_rows: Optional[Sequence[Sequence[int]]] = None,
                       dn_rows: Optional[Sequence[Sequence[int]]] = None, host_rows=None) -> dict:
        """the Greeks tail (svmc_greeks_payoff_chain) on resident log-returns: expiry i of the base job reads snapshot row
        base_rows[i], of parameter p's bumped jobs rows up_rows[p][i] and dn_rows[p][i]; steps: the P step sizes h_p.  host_rows =
        (base [m], up [P][m], dn [P][m]) host arrays instead: uploaded to snapshot rows 0 .. (1 + 2P) m - 1 in job order (base, up_0,
        dn_0, ...).  Each job's spot sums are formed on the device (svmc_spot_sums).  codes: 0 ('C') / 1 ('P') per strike.  Returns
        {field: [m] -> [K_i]} for delta, delta_stderr, dual_delta, dual_delta_stderr, n_itm; "sens", "sens_stderr", "n_pairs":
        [P][m] -> [K_i]; "spot_sums": [1 + 2P, m, 2], the jobs' [sum F exp(x), count]."""
        ch = marshalled_chain(np.zeros(len(strikes)), forwards, discfactors, strikes, codes)
        m, K = ch["m"], ch["total"]
        h = np.ascontiguousarray(np.atleast_1d(np.asarray(steps, dtype=np.float64))).ravel()
        P = h.size
        if host_rows is not None:
            base, up, dn = host_rows
            jobs = [list(base)] + [job for p in range(P) for job in (list(up[p]), list(dn[p]))]
            if len(jobs) != 1 + 2 * P or any(len(job) != m for job in jobs):
                raise ValueError("one host array per expiry for the base job and for each up / dn job of the P steps")
            self.reserve_snapshots((1 + 2 * P) * m)
            self._upload_snapshot_rows([x for job in jobs for x in job], 0)
            base_rows = list(range(m))
            up_rows = [list(range((1 + 2 * p) * m, (2 + 2 * p) * m)) for p in range(P)]
            dn_rows = [list(range((2 + 2 * p) * m, (3 + 2 * p) * m)) for p in range(P)]
        up_rows, dn_rows = list(up_rows or []), list(dn_rows or [])
        if base_rows is None or len(base_rows) != m or len(up_rows) != P or len(dn_rows) != P or \
                any(len(r) != m for r in up_rows + dn_rows):
            raise ValueError("one snapshot row per expiry for the base job and for each up / dn job of the P steps")
        job_rows = [list(base_rows)] + [r for p in range(P) for r in (list(up_rows[p]), list(dn_rows[p]))]
        spot_ptr, _ = self.alloc_sums(2 * m * (1 + 2 * P), "greeks_spot")
        f = ch["keep"][1]
        for j, rows in enumerate(job_rows):
            for i, r in enumerate(rows):
                self.spot_sums(self.snapshot_ptr(r), float(f[i]), spot_ptr + 16 * (j * m + i))
        ws_ptr, nbytes = self._side_workspace(self.lib.svmc_greeks_payoff_workspace_bytes, (self.n_path, m, K, P), "greeks_workspace")
        base_out, sens_out = np.empty((len(GREEKS_BASE_FIELDS), max(K, 1))), np.empty((max(P, 1), len(GREEKS_SENS_FIELDS), max(K, 1)))
        ptrs = lambda rows: (C.c_void_p * max(len(rows), 1))(*[self.snapshot_ptr(r) for r in rows])      # noqa: E731
        _lib.check(self.lib.svmc_greeks_payoff_chain(
            ptrs(job_rows[0]), ptrs([r for rows in up_rows for r in rows]), ptrs([r for rows in dn_rows for r in rows]), self.n_path,
            *ch["args"][1:], P, ptr(h), spot_ptr, ptr(base_out), ptr(sens_out), ws_ptr, nbytes, self.stream))
        out = dict(zip(GREEKS_BASE_FIELDS, expiry_rows(base_out, ch["slices"])))
        for r, field in enumerate(GREEKS_SENS_FIELDS):
            out[field] = [[sens_out[p, r, sl] for sl in ch["slices"]] for p in range(P)]
        out["spot_sums"] = self.download(spot_ptr, 2 * m * (1 + 2 * P)).reshape(1 + 2 * P, m, 2)
        return out

    def price_chain_greeks_fused(self, ch: dict, model: str, rows: np.ndarray, steps: np.ndarray, mode: int, nb_steps_per_year: int,
                                 seed: int, call_id: int):
        """svmc_logsv_chain_price_greeks (model "logsv", mode = is_spot_measure, rows [1 + 2P][6 + m]) or
        svmc_heston_chain_price_greeks ("heston", mode = scheme code, rows [1 + 2P][5]) on this engine's session: the job table's
        rows on ONE (seed, call id).  Returns (prices [m] -> [K_i], stderrs the same, base [5][K], sens [P][3][K])."""
        fn, modes = self._model_entry("price_chain_greeks_fused", model, "chain_price_greeks", GREEKS_MODELS, mode)
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        h = np.ascontiguousarray(steps, dtype=np.float64).ravel()
        P, K = h.size, max(ch["total"], 1)
        if rows.ndim != 2 or rows.shape[0] != 1 + 2 * P:
            raise ValueError("the job table has one base row and an up and a dn row per step")
        res, base, sens = np.empty((2, K)), np.empty((len(GREEKS_BASE_FIELDS), K)), np.empty((max(P, 1), len(GREEKS_SENS_FIELDS), K))
        self._session_call(ch, lambda sess: fn(
            sess, *ch["args"], P, ptr(rows), ptr(h), *modes, int(nb_steps_per_year), int(seed), int(call_id), row_ptr(res, 0),
            row_ptr(res, 1), ptr(base), ptr(sens)), f"{model}_chain_rng_many_kernel")
        return expiry_rows(res, ch["slices"]) + (base, sens[:P])

    def il_payoffs(self, p1, p0, pa, pb, notional=1000000, snap_row: Optional[int] = None, return_pieces: bool = False):
        """the Monte Carlo impermanent loss of the ranges [pa, pb] opened at p0, at the forwards p1, from the resident
        log-returns, whichever generator left them (svmc_il_payoff, include/svmc.h): the current state x, or snapshot row
        snap_row.  p1, p0, pa, pb, notional broadcast together and share one path set, one recentring and one pass.  Returns
        (value, stderr) in the broadcast shape (scalars for scalar input), and with return_pieces a dict of the six piece means,
        n_kept and n_dropped.  ValueError before any device work for an invalid case."""
        from .pricers.il_pricer import IL_OUT_DOUBLES, il_cases, il_mc_results
        cases, shape = il_cases(p1, p0, pa, pb, notional)
        n = cases.shape[0]
        ws_ptr, nbytes = self._side_workspace(self.lib.svmc_il_payoff_workspace_bytes, (self.n_path, n), "il_workspace")
        out = np.empty((n, IL_OUT_DOUBLES))
        _lib.check(self.lib.svmc_il_payoff(self.x.ptr if snap_row is None else self.snapshot_ptr(snap_row), self.n_path,
                                           ptr(cases), n, ptr(out), ws_ptr, nbytes, self.stream))
        return il_mc_results(out, shape, return_pieces)

    def price_hawkesjd_chain_tilted_fused(self, ch: dict, params: np.ndarray, nb_steps_per_year: int, seed: int, call_id: int,
                                          gammas, recenter: bool):
        """the Hawkes chain under the risk-premia kernel for every gamma from ONE stepping launch, as one
        svmc_hawkesjd_chain_price_tilted call on this engine's state (ch: tilted_chain_arrays); returns as tilted_payoffs.  The
        plain measure is not a separate output: gamma = 0 with recenter is svmc_hawkesjd_chain_price at discount factors 1, so a
        caller who wants both measures puts 0 among the gammas"""
        params = np.ascontiguousarray(params, dtype=np.float64)
        m, K, G = ch["m"], ch["total"], ch["gammas"].size
        prices, stderrs, stats = np.empty(max(G * K, 1)), np.empty(max(G * K, 1)), np.empty(G * m * TILTED_STATS_DOUBLES)
        self._session_call(ch, lambda sess: self.lib.svmc_hawkesjd_chain_price_tilted(
            sess, ch["ttms_arg"], *ch["args"], ptr(params), int(nb_steps_per_year), int(seed), int(call_id), *ch["gamma_args"],
            int(bool(recenter)), ptr(prices), ptr(stderrs), ptr(stats)), "hawkesjd_chain_rng_kernel")
        return tilted_results(prices[:G * K], stderrs[:G * K], stats, ch)

    def price_hawkesjd_chain_tilted_many_fused(self, ch: dict, params: np.ndarray, nb_steps_per_year: int, seeds: Sequence[int],
                                               call_ids: Sequence[int], gammas: np.ndarray, recenter: bool):
        """J Hawkes jobs of one chain under the risk-premia kernel as ONE svmc_hawkesjd_chain_price_tilted_many call on this
        engine's session (ch: tilted_chain_arrays; params [J][SVMC_HAWKESJD_PARAMS]; gammas [J][G], every row a job's gammas):
        one stepping launch for all jobs, then each job's tilted payoff launches.  Returns per job what
        price_hawkesjd_chain_tilted_fused returns for it, J at most MANY_MAX_JOBS"""
        n_jobs, jobs = self._many_jobs(params, seeds, call_ids, "one seed, one call id and one row of gammas per job")
        gammas = np.ascontiguousarray(gammas, dtype=np.float64)
        if gammas.ndim != 2 or gammas.shape[0] != n_jobs:
            raise ValueError("one seed, one call id and one row of gammas per job")
        m, K, G = ch["m"], ch["total"], gammas.shape[1]
        prices, stderrs = np.empty((n_jobs, max(G * K, 1))), np.empty((n_jobs, max(G * K, 1)))
        stats = np.empty((n_jobs, G * m * TILTED_STATS_DOUBLES))
        sess = self.fused_chain_session(m, K)
        _lib.check(self.lib.svmc_hawkesjd_chain_price_tilted_many(
            sess, ch["ttms_arg"], *ch["args"], n_jobs, *jobs, int(nb_steps_per_year), ptr(gammas), G, int(bool(recenter)), ptr(prices),
            ptr(stderrs), ptr(stats)))
        # the C rows are [G K] with no padding; the host arrays above are padded to one double for an empty chain only
        out = []
        for j in range(n_jobs):
            out.append(tilted_results(prices.ravel()[j * G * K:(j + 1) * G * K], stderrs.ravel()[j * G * K:(j + 1) * G * K],
                                      stats[j], dict(ch, gammas=gammas[j])))
        return out

    def close(self) -> None:
        """free every HBM buffer of the engine; any later launch through it fails in the C ABI's null-pointer
        checks (SvmcError), it never touches freed memory"""
        self.closed = True
        if self._fused is not None:                 # the session borrows x / vol / qvar: it goes first
            self.lib.svmc_session_destroy(self._fused)
            self._fused, self._fused_size = None, (0, 0)
        self.__dict__.pop("_comm_bufs", None)       # a communicator's reduction tensors that lived on this engine (dist.TorchComm)
        for b in (self.x, self.vol, self.qvar, self._cv, self.ws, self._snap, self._rand, self._factors, *self._sums.values(),
                  *self._bulk.values()):
            if b is not None:
                b.free()
        if self._pinned is not None:
            self.lib.svmc_host_free(self._pinned)
            self._pinned, self._pinned_doubles = None, 0


class DeviceRandoms:
    """fixed randoms of a chain kept resident in HBM: upload once, re-price at kernel speed on
    every calibration iterate.  Holds, per expiry, this rank's column range of W0 and W1 ([nb_steps_i][n_local])."""

    def __init__(self, W0s: Sequence[np.ndarray], W1s: Sequence[np.ndarray], dts: Sequence[float], n_local: int,
                 col0: int = 0):
        lib = _lib.load()
        self.nb_path = int(np.asarray(W0s[0]).shape[1])
        self.n_local, self.col0 = int(n_local), int(col0)
        self.dts = [float(d) for d in dts]
        self.nb_steps, self.w0, self.w1 = [], [], []
        self._session, self._session_strikes = None, 0
        self._session_sets, self._session_sets_size = None, (0, 0)
        for W0, W1 in zip(W0s, W1s):
            W0 = np.ascontiguousarray(W0, dtype=np.float64)
            W1 = np.ascontiguousarray(W1, dtype=np.float64)
            if W0.shape != W1.shape or W0.shape[1] != self.nb_path:
                raise ValueError("every W0/W1 must have shape [nb_steps_i, nb_path]")
            nb = W0.shape[0]
            bufs = []
            for a in (W0, W1):
                buf = DeviceBuffer(nb * self.n_local)
                _lib.check(lib.svmc_memcpy2d_h2d(buf.ptr, 8 * self.n_local, a.ctypes.data + 8 * self.col0,
                                                 8 * a.shape[1], 8 * self.n_local, nb, None))
                bufs.append(buf)
            _lib.check(lib.svmc_stream_synchronize(None))
            self.nb_steps.append(nb)
            self.w0.append(bufs[0])
            self.w1.append(bufs[1])

    @classmethod
    def drawn_on_device(cls, nb_steps: Sequence[int], dts: Sequence[float], nb_path: int, n_local: int, col0: int,
                        seed: int, call_id: int = 0) -> "DeviceRandoms":
        """the chain's fixed randoms drawn IN HBM by the counter-based generator (svmc_fill_normals) instead of being
        drawn by NumPy and uploaded: expiry i holds the normals the on-device-RNG generators consume for
        (seed, call_id) at steps sum(nb_steps[:i]) .. -- so a chain priced on them is the on-device-RNG chain with its
        randoms frozen, and a calibration no longer starts with a second of host Mersenne-Twister draws."""
        lib = _lib.load()
        self = cls.__new__(cls)
        self.nb_path, self.n_local, self.col0 = int(nb_path), int(n_local), int(col0)
        self.dts = [float(d) for d in dts]
        self.nb_steps, self.w0, self.w1 = [int(n) for n in nb_steps], [], []
        self._session, self._session_strikes = None, 0
        self._session_sets, self._session_sets_size = None, (0, 0)
        step0 = 0
        for nb in self.nb_steps:
            b0, b1 = DeviceBuffer(nb * self.n_local), DeviceBuffer(nb * self.n_local)
            _lib.check(lib.svmc_fill_normals(b0.ptr, b1.ptr, self.n_local, self.n_local, nb, int(seed), int(call_id),
                                             self.col0, step0, None))
            self.w0.append(b0)
            self.w1.append(b1)
            step0 += nb
        _lib.check(lib.svmc_stream_synchronize(None))
        return self

    @classmethod
    def frozen(cls, nb_steps: Sequence[int], dts: Sequence[float], nb_path: int, n_local: int, col0: int, seed: int,
               call_id: int = 0) -> "DeviceRandoms":
        """the chain's fixed randoms as NOTHING BUT their definition: the counter-based stream of (seed, call_id).  No array
        exists, on the host or in HBM -- every pricing regenerates the same normals in registers (svmc_logsv_chain_price_
        frozen_sets), so a chain priced on this object is logsv_mc_chain_pricer(seed=seed) with the given call id, bit for
        bit, at every call.  The reference's MC calibration keeps RandomState arrays for the same purpose
        (pricers/logsv_pricer.py:244-265, 520-527); drawn_on_device() kept 16 bytes per path-step of HBM."""
        self = cls.__new__(cls)
        self.nb_path, self.n_local, self.col0 = int(nb_path), int(n_local), int(col0)
        self.dts = [float(d) for d in dts]
        self.nb_steps, self.w0, self.w1 = [int(n) for n in nb_steps], [], []
        self._session, self._session_strikes = None, 0
        self._session_sets, self._session_sets_size = None, (0, 0)
        self.frozen_stream = (int(seed), int(call_id))
        return self

    @property
    def is_frozen(self) -> bool:
        return getattr(self, "frozen_stream", None) is not None

    def __len__(self):
        return len(self.nb_steps)

    def free(self) -> None:
        for b in self.w0 + self.w1:
            b.free()
        if self._session is not None:
            _lib.check(_lib.load().svmc_session_destroy(self._session))
            self._session = None
        if self._session_sets is not None:
            _lib.check(_lib.load().svmc_session_destroy(self._session_sets))
            self._session_sets = None

    def graph_launches(self) -> int:
        """how many chain pricings of this object were hipGraph replays (diagnostics)"""
        if self._session is None:
            return 0
        n = C.c_size_t()
        _lib.check(_lib.load().svmc_session_graph_launches(self._session, C.byref(n)))
        return int(n.value)

    def price_logsv_chain(self, ttms, forwards, discfactors, strikes: Sequence[np.ndarray], codes: Sequence[np.ndarray],
                          v0, theta, kappa1, kappa2, beta, volvol, etas, is_spot_measure: bool, variable_type: int,
                          use_graph: bool = True, want_ivols: bool = False):
        """one call of the fused single-GPU driver svmc_logsv_chain_price_fixed on these randoms: the chain's launches
        captured once into a hipGraph and replayed per parameter set (use_graph=False: queued back to back instead),
        one synchronisation, prices and stderrs back -- the inner loop of an MC calibration.  Same kernels in the
        same order as mc_chain.price_chain_on_engine, hence the same bits.  want_ivols: a third list, the Black-76
        implied vols of the prices, computed by the graph's last kernel (svmc_logsv_chain_price_fixed_iv)."""
        self._check_expiries(strikes)
        if self.is_frozen:
            row = np.concatenate([[v0, theta, kappa1, kappa2, beta, volvol], np.asarray(etas, dtype=np.float64).ravel()])
            return self.price_logsv_chain_sets(ttms, forwards, discfactors, strikes, codes, row[None, :], is_spot_measure,
                                               variable_type, want_ivols=want_ivols, use_graph=use_graph)[0]
        lib = _lib.load()
        m = len(self)
        ch = marshalled_chain(ttms, forwards, discfactors, strikes, codes)
        total = ch["total"]
        if self._session is None or self._session_strikes < total:
            if self._session is not None:
                _lib.check(lib.svmc_session_destroy(self._session))
            sess = C.c_void_p()
            _lib.check(lib.svmc_session_create(C.byref(sess), self.n_local, m, max(total, 1)))
            self._session, self._session_strikes = sess, max(total, 1)
        _lib.check(lib.svmc_session_use_graphs(self._session, int(bool(use_graph))))
        dp = C.POINTER(C.c_double)
        etas = np.ascontiguousarray(etas, dtype=np.float64)
        w0 = (C.c_void_p * m)(*[b.ptr for b in self.w0])
        w1 = (C.c_void_p * m)(*[b.ptr for b in self.w1])
        nbs, dts = self._step_grid
        prices, stderrs = np.empty(max(total, 1)), np.empty(max(total, 1))
        ivols = np.empty(max(total, 1)) if want_ivols else None
        _lib.check(lib.svmc_logsv_chain_price_fixed_iv(
            self._session, ch["ttms"], ch["forwards"], ch["discfactors"], etas.ctypes.data_as(dp), m, ch["strikes"], ch["codes"],
            ch["offsets"], float(v0), float(theta), float(kappa1), float(kappa2), float(beta), float(volvol),
            int(bool(is_spot_measure)), int(variable_type), w0, w1, nbs, dts, self.n_local, prices.ctypes.data_as(dp),
            stderrs.ctypes.data_as(dp), ivols.ctypes.data_as(dp) if want_ivols else None))
        split = lambda a: [a[sl].copy() for sl in ch["slices"]]      # noqa: E731
        return (split(prices), split(stderrs), split(ivols)) if want_ivols else (split(prices), split(stderrs))

    def _check_expiries(self, strikes) -> None:
        if len(strikes) != len(self):
            raise ValueError(f"the chain has {len(strikes)} expiries, the randoms {len(self)}")

    @functools.cached_property
    def _step_grid(self):
        """the randoms' step grid as the C drivers take it: nb_steps as a C int array, dts as a double pointer (which keeps its
        array alive)"""
        return (C.c_int * len(self))(*self.nb_steps), np.array(self.dts, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))

    def price_logsv_chain_sets(self, ttms, forwards, discfactors, strikes: Sequence[np.ndarray], codes: Sequence[np.ndarray],
                               params_rows: np.ndarray, is_spot_measure: bool, variable_type: int, want_ivols: bool = False,
                               use_graph: bool = True, comm_handle=None, rank: int = 0, world: int = 1):
        """SEVERAL parameter sets on these randoms in one call of svmc_logsv_chain_price_fixed_sets: with 2..8 sets one
        replayed graph whose stepping launch reads the randoms once for all of them.  params_rows [n_sets][6 + m] =
        (v0, theta, kappa1, kappa2, beta, volvol, vol-backbone eta per expiry).  Returns per set what price_logsv_chain
        returns -- the same bits."""
        self._check_expiries(strikes)
        lib = _lib.load()
        m = len(self)
        params_rows = np.ascontiguousarray(params_rows, dtype=np.float64)
        n_sets = params_rows.shape[0]
        if params_rows.ndim != 2 or params_rows.shape[1] != 6 + m or n_sets < 1:
            raise ValueError("params_rows must have shape [n_sets, 6 + n_expiries]")
        ch = marshalled_chain(ttms, forwards, discfactors, strikes, codes)
        total = ch["total"]
        nbs, dts = self._step_grid
        per_launch = min(n_sets, 8)
        need = (m * per_launch, max(total * per_launch, 1))
        if self.is_frozen:
            need = (m * 8, max(total * 8, 1))       # one session for every set count of an optimizer run (1 .. 8 per launch)
        if self._session_sets is None or self._session_sets_size[0] < need[0] or self._session_sets_size[1] < need[1]:
            if self._session_sets is not None:
                _lib.check(lib.svmc_session_destroy(self._session_sets))
            sess = C.c_void_p()
            _lib.check(lib.svmc_session_create(C.byref(sess), self.n_local, need[0], need[1]))
            self._session_sets, self._session_sets_size = sess, need
            self._graphs_on = None
            if comm_handle is not None:
                _lib.check(lib.svmc_session_set_comm(sess, comm_handle, int(rank), int(world), self.nb_path, self.col0))
        dp = C.POINTER(C.c_double)
        # one result block per call, cut into per-set, per-expiry VIEWS (nothing else refers to the block)
        res = np.empty((3 if want_ivols else 2, n_sets, max(total, 1)))
        p_res = res.ctypes.data
        row_bytes = res.strides[0]
        ptr = lambda j: C.cast(p_res + j * row_bytes, dp)      # noqa: E731
        slices = ch["slices"]
        if self.is_frozen:
            if self.__dict__.get("_graphs_on") != bool(use_graph):
                _lib.check(lib.svmc_session_use_graphs(self._session_sets, int(bool(use_graph))))
                self._graphs_on = bool(use_graph)
            seed, call_id = self.frozen_stream
            _lib.check(lib.svmc_logsv_chain_price_frozen_sets(
                self._session_sets, ch["ttms"], ch["forwards"], ch["discfactors"], m, ch["strikes"], ch["codes"], ch["offsets"],
                n_sets, params_rows.ctypes.data_as(dp), int(bool(is_spot_measure)), int(variable_type), nbs, dts,
                seed, call_id, ptr(0), ptr(1), ptr(2) if want_ivols else None))
        else:
            w0 = (C.c_void_p * m)(*[b.ptr for b in self.w0])
            w1 = (C.c_void_p * m)(*[b.ptr for b in self.w1])
            _lib.check(lib.svmc_logsv_chain_price_fixed_sets(
                self._session_sets, ch["ttms"], ch["forwards"], ch["discfactors"], m, ch["strikes"], ch["codes"], ch["offsets"],
                n_sets, params_rows.ctypes.data_as(dp), int(bool(is_spot_measure)), int(variable_type), w0, w1, nbs,
                dts, self.n_local, ptr(0), ptr(1), ptr(2) if want_ivols else None))
        return [tuple([part[q, sl] for sl in slices] for part in res) for q in range(n_sets)]


def payoff_finalize(sums: np.ndarray, shifts: np.ndarray, discfactor: float, n_path_total: float
                    ) -> Tuple[np.ndarray, np.ndarray]:
    """host arithmetic of utils/mc_payoffs.py:85-88 on the reduced sums (svmc_payoff_finalize)."""
    lib = _lib.load()
    k = len(shifts)
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    shifts = np.ascontiguousarray(shifts, dtype=np.float64)
    prices, stderrs = np.empty(k), np.empty(k)
    pd = C.POINTER(C.c_double)
    _lib.check(lib.svmc_payoff_finalize(sums.ctypes.data_as(pd), shifts.ctypes.data_as(pd), k, float(discfactor),
                                        float(n_path_total), prices.ctypes.data_as(pd), stderrs.ctypes.data_as(pd)))
    return prices, stderrs


def payoff_finalize_chain(sums: np.ndarray, shifts: np.ndarray, discfactors: np.ndarray, n_path_total: float
                          ) -> Tuple[np.ndarray, np.ndarray]:
    """payoff_finalize for all the strikes of a chain in one call (svmc_payoff_finalize_chain): discfactors holds one
    discount factor per strike.  The same arithmetic per strike, hence the same bits as expiry-by-expiry calls."""
    lib = _lib.load()
    k = len(shifts)
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    shifts = np.ascontiguousarray(shifts, dtype=np.float64)
    discfactors = np.ascontiguousarray(discfactors, dtype=np.float64)
    prices, stderrs = np.empty(k), np.empty(k)
    pd = C.POINTER(C.c_double)
    _lib.check(lib.svmc_payoff_finalize_chain(sums.ctypes.data_as(pd), shifts.ctypes.data_as(pd), discfactors.ctypes.data_as(pd),
                                              k, float(n_path_total), prices.ctypes.data_as(pd), stderrs.ctypes.data_as(pd)))
    return prices, stderrs


# Engines are cached per (device id, n_path, path_offset, THREAD) so that buffers stay resident across calls and two threads
# that price chains of the same size concurrently never share state buffers, reduction scratch or the pinned download
# buffer: each gets its own engine (the launches of all of them are serialised by the HIP runtime on the stream they
# were given -- the default stream unless the caller built its own HipEngine with another).  The cache is process-global and
# guarded by a lock.  Eviction (more than MAX_CACHED_ENGINES resident) only ever closes an engine nobody else references
# -- a caller that kept the object returned by get_engine() keeps its HBM; the engines of threads that ended are the
# first to go -- and an engine that was closed raises SvmcError (null pointer) on its next launch instead of touching
# freed memory.
MAX_CACHED_ENGINES = 4
_ENGINES = {}
_ENGINES_LOCK = threading.Lock()


def _current_device() -> int:
    dev = C.c_int()
    _lib.check(_lib.load().svmc_get_device(C.byref(dev)))
    return dev.value


def get_engine(n_path: int, path_offset: int = 0, device: Optional[int] = None) -> HipEngine:
    dev = _current_device() if device is None else int(device)     # None = the CURRENT HIP device, resolved now
    key = (dev, int(n_path), int(path_offset), threading.get_ident())
    with _ENGINES_LOCK:
        eng = _ENGINES.get(key)
        if eng is not None and not eng.closed:
            _ENGINES[key] = _ENGINES.pop(key)          # most recently used last
            return eng
        if len(_ENGINES) >= MAX_CACHED_ENGINES:        # bound resident HBM: drop FREE engines, dead threads' first, then LRU
            alive = {t.ident for t in threading.enumerate()}
            for k in sorted(_ENGINES, key=lambda k_: k_[3] in alive):      # stable: keeps the LRU order within each class
                # references: the dict, the loop variable below, getrefcount's argument
                cand = _ENGINES[k]
                if sys.getrefcount(cand) <= 3:
                    _ENGINES.pop(k).close()
                    break
                del cand
        eng = HipEngine(n_path, device=dev, path_offset=path_offset)
        _ENGINES[key] = eng
        return eng
