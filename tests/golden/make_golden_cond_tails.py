"""
Record what the four weighted conditional tails -- svmc_tilted_cond_payoff_chain (libsvmc_ext.so) and svmc_tilted_cond_greeks_chain,
svmc_cond_density_chain, svmc_jump_sets_payoff_chain (libsvmc_est.so) -- answer, so that a change which moves their statements keeps
their behaviour.  This project's own output, in two files:

    python tests/golden/make_golden_cond_tails.py host      # cond_tails_host.json: no GPU is touched
    python tests/golden/make_golden_cond_tails.py gpu       # cond_tails.npz, on a GPU box; the file is replayed once after it is written

Recorded on commit 785b96a ("Price every (sigma, gamma) of a Hawkes chain on one set of jump paths"), the parent of the change that
gave the four tails one table walk, one payoff and finish body, one quote check and one host driver (csrc/svmc_tilted_cond.h).
tests/test_cond_tails_host.py and tests/test_gpu_cond_tails.py replay the files on every later build.

cond_tails_host.json: the four *_workspace_bytes values on a grid of (n_path, (m, K), gamma or set count), and the status with which
each chain entry refuses a call with ONE fault.  Every call carries a workspace too small for it, so that nothing is ever launched:
a call without a fault answers SVMC_ERR_WORKSPACE, and the row pointers are never dereferenced.

cond_tails.npz: the outputs of the four entries as bits, with the small inputs.  n_path = 2 x 256 + 37 (three path blocks, the last
partial); five expiries of 1, 0, 9, 8 and 0 strikes or points (empty expiries in the middle and at the end, ragged groups at widths
8 and 4, a full group of 8), calls and puts mixed and strike 3 at -0.5, so that K + corr <= 0; gammas (0, -0.5, 0.75, 2.5, -3) for
the payoffs and the Greeks, 3 gammas (one tile of 4, ragged) and 9 gammas (the wide tile, its second tile ragged) for the density,
3 sets of which the last has variance 0; recenter 0 and 1.  Variants:
  planted        in every row one cv == 0, one cv < 0, one NaN mu, one +inf mu, and one mu = -150: its weight squared overflows at the
                 gamma that is largest in size, -3, alone (a path at +150 would carry every sum of every gamma)
  path0_dropped  path 0 of every row is NaN besides
  no_kept_path   expiry 2 keeps no path besides
  large          planted, at n_path = 1024 x 256 + 3 (the stride loop takes a second trip in three lanes), recenter 1; its rows come
                 from an integer formula (large_rows) and are not stored
Every recorded price, error, Greek and density is finite, except the quotes of expiry 2 in no_kept_path (0 / 0) and the density at
gamma -3, where a path's weight is dropped (the header: NaN).  The jump rows are the mu rows (a = mu); their cv is not read.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(HERE, "cond_tails.npz")
HOST_FIXTURE = os.path.join(HERE, "cond_tails_host.json")

N_PATH, N_LARGE, COUNTS = 2 * 256 + 37, 1024 * 256 + 3, (1, 0, 9, 8, 0)
M, K = len(COUNTS), sum(COUNTS)
VARIANTS = ("planted", "path0_dropped", "no_kept_path", "large")
EMPTY_EXPIRY = 2
GAMMAS = np.array([0.0, -0.5, 0.75, 2.5, -3.0])
CD_GAMMAS = {"g3": np.array([0.0, 0.75, -3.0]), "g9": np.array([0.0, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 2.5, -3.0])}
DROP_GAMMA = -3.0
SET_GAMMAS = np.array([0.75, -3.0, 1.5])
SET_VARIANCES = np.array([[0.02 * (i + 1) for i in range(M)], [0.03 * (i + 1) for i in range(M)], [0.0] * M])
TILTED_STATS, TCG_ROWS, TCG_STATS, CD_STATS = 8, 8, 4, 5
OK, ERR_WORKSPACE = 0, 5
DP, SZP, I8P = C.POINTER(C.c_double), C.POINTER(C.c_size_t), C.POINTER(C.c_int8)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
def plant(mu: np.ndarray, cv: np.ndarray, variant: str) -> None:
    n = mu.shape[-1]
    cv[..., 5] = 0.0
    cv[..., 17] = -0.01
    mu[..., 300] = np.nan
    mu[..., n - 1] = np.inf
    mu[..., 40] = -150.0
    if variant in ("path0_dropped", "no_kept_path"):
        mu[..., 0] = np.nan
    if variant == "no_kept_path":
        cv[EMPTY_EXPIRY, :] = -1.0
        mu[EMPTY_EXPIRY, :] = np.nan               # (the jump rows have no cv to drop a path by)


def large_rows():
    """(mu, cv) [M][N_LARGE] from integers alone: two multiplicative hashes of (path, expiry) mod 2^32, scaled by sums and products that
    IEEE arithmetic rounds the same everywhere"""
    i = np.arange(N_LARGE, dtype=np.uint64)[None, :]
    j = np.arange(1, M + 1, dtype=np.uint64)[:, None]
    u1 = ((i * np.uint64(2654435761) + j * np.uint64(40503)) % np.uint64(1 << 32)).astype(np.float64) / float(1 << 32)
    u2 = ((i * np.uint64(2246822519) + j * np.uint64(3266489917)) % np.uint64(1 << 32)).astype(np.float64) / float(1 << 32)
    scale = np.arange(1, M + 1, dtype=np.float64)[:, None]
    mu = -0.01 * scale + (0.3 * np.sqrt(scale)) * (u1 - 0.5)
    cv = (0.004 + 0.02 * u2) * scale
    plant(mu, cv, "large")
    return mu, cv


def make_inputs() -> dict:
    """{name: array} of the chain, the points and, per stored variant, the rows"""
    rng = np.random.default_rng(20261021)
    forwards = np.array([1.0, 1.02, 0.98, 1.05, 1.01])
    offsets = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.uintp)
    strikes = np.concatenate([forwards[i] * np.linspace(0.8, 1.2, c) if c > 1 else forwards[i] * np.full(c, 0.95) for i, c in enumerate(COUNTS)])
    strikes[3] = -0.5
    types = (np.arange(K) % 2 == 0).astype(np.int8)             # put, call, put, ...
    expiry = np.repeat(np.arange(M), COUNTS)
    shifts = np.where(types == 1, np.maximum(strikes - forwards[expiry], 0.0), np.maximum(forwards[expiry] - strikes, 0.0))
    points = np.concatenate([np.linspace(-0.45, 0.35, c) if c > 1 else np.full(c, -0.05) for c in COUNTS])
    a = dict(forwards=forwards, offsets=offsets, strikes=strikes, types=types, shifts=shifts, points=points)
    scale = np.sqrt(np.arange(1, M + 1))[:, None]
    mu = -0.01 * scale ** 2 + 0.15 * scale * rng.standard_normal((M, N_PATH))
    cv = (0.004 + 0.02 * rng.random((M, N_PATH))) * scale ** 2
    for variant in VARIANTS[:3]:
        rows = dict(mu=mu.copy(), cv=cv.copy())
        plant(rows["mu"], rows["cv"], variant)
        for name, arr in rows.items():
            a[f"{variant}__{name}"] = np.ascontiguousarray(arr, dtype=np.float64)
    return a


def rows_of(a: dict, variant: str):
    return large_rows() if variant == "large" else (a[f"{variant}__mu"], a[f"{variant}__cv"])


# ---- device memory through the core library's allocator -----------------------------------------------------------------------------
class Device:
    def __init__(self, L):
        from stochvolmodels_amd import _lib
        self.L, self.check, self.owned = L, _lib.check, []

    def alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self.check(self.L.svmc_malloc(C.byref(p), max(int(nbytes), 8)))
        self.owned.append(p)
        self.check(self.L.svmc_memset(p, 0, max(int(nbytes), 8), None))
        return p.value

    def rows(self, a: np.ndarray):
        """the rows of an [m][n] array on the device as a C array of pointers"""
        a = np.ascontiguousarray(a, dtype=np.float64)
        base = self.alloc(a.nbytes)
        self.check(self.L.svmc_memcpy_h2d(base, a.ctypes.data, a.nbytes, None))
        self.check(self.L.svmc_stream_synchronize(None))
        return (C.c_void_p * a.shape[0])(*[base + 8 * a.shape[1] * r for r in range(a.shape[0])])

    def download(self, ptr: int, n_doubles: int) -> np.ndarray:
        out = np.empty(n_doubles)
        self.check(self.L.svmc_memcpy_d2h(out.ctypes.data, ptr, out.nbytes, None))
        self.check(self.L.svmc_stream_synchronize(None))
        return out

    def free(self):
        for p in self.owned:
            self.check(self.L.svmc_free(p))
        self.owned = []


def _p(a, ctype=DP):
    return a.ctypes.data_as(ctype)


def _size(fn, *args) -> int:
    out = C.c_size_t(0)
    rc = fn(*args, C.byref(out))
    if rc != OK:
        raise RuntimeError(f"{fn.__name__}{args}: status {rc}")
    return out.value


def _ok(rc: int, what: str) -> None:
    if rc != OK:
        raise RuntimeError(f"{what}: status {rc}")


# ---- the four entries on one variant ------------------------------------------------------------------------------------------------
def run_tails(libs, a: dict, variant: str) -> dict:
    """{variant__entry__(rR | gN)__output: array}"""
    L, X, E = libs
    mu_h, cv_h = rows_of(a, variant)
    n = mu_h.shape[1]
    dev, out = Device(L), {}
    fw, ks, ty, sh, offs, pts = (a[k] for k in ("forwards", "strikes", "types", "shifts", "offsets", "points"))
    NG, Q = GAMMAS.size, SET_GAMMAS.size
    G8 = sum(max((c + 7) // 8, 1) for c in COUNTS)
    try:
        mu, cv = dev.rows(mu_h), dev.rows(cv_h)
        for recenter in ((1,) if variant == "large" else (0, 1)):
            tag = f"{variant}__{{}}__r{recenter}__{{}}"
            nb = _size(X.svmc_tilted_cond_workspace_bytes, n, M, K, NG)
            ws = dev.alloc(nb)
            prices, errs, stats = np.empty(NG * K), np.empty(NG * K), np.empty(NG * M * TILTED_STATS)
            _ok(X.svmc_tilted_cond_payoff_chain(mu, cv, n, _p(fw), M, _p(ks), _p(ty, I8P), _p(sh), _p(offs, SZP), _p(GAMMAS), NG, recenter,
                                                _p(prices), _p(errs), _p(stats), ws, nb, None), "svmc_tilted_cond_payoff_chain")
            # fwd [m][4] where the workspace's walk puts it: behind the image and the two device-computed strike columns
            fwd = dev.download(ws + 40 * M + 16 * G8 + 8 * (3 * K + NG) + 16 * K, 4 * M)
            out.update({tag.format("payoff", "prices"): prices, tag.format("payoff", "stderrs"): errs, tag.format("payoff", "stats"): stats,
                        tag.format("payoff", "fwd"): fwd})
            nb = _size(E.svmc_tilted_cond_greeks_workspace_bytes, n, M, K, NG)
            greeks, stats = np.empty(NG * TCG_ROWS * K), np.empty(NG * M * TCG_STATS)
            _ok(E.svmc_tilted_cond_greeks_chain(mu, cv, n, _p(fw), M, _p(ks), _p(ty, I8P), _p(offs, SZP), _p(GAMMAS), NG, recenter,
                                                _p(greeks), _p(stats), dev.alloc(nb), nb, None), "svmc_tilted_cond_greeks_chain")
            out.update({tag.format("greeks", "greeks"): greeks, tag.format("greeks", "stats"): stats})
            nb = _size(E.svmc_jump_sets_workspace_bytes, n, M, K, Q)
            prices, errs, stats, corr = np.empty(Q * K), np.empty(Q * K), np.empty(Q * M * TILTED_STATS), np.empty(M)
            _ok(E.svmc_jump_sets_payoff_chain(mu, n, _p(fw), M, _p(ks), _p(ty, I8P), _p(sh), _p(offs, SZP), _p(SET_VARIANCES), _p(SET_GAMMAS),
                                              Q, recenter, _p(prices), _p(errs), _p(stats), _p(corr), dev.alloc(nb), nb, None),
                "svmc_jump_sets_payoff_chain")
            out.update({tag.format("sets", "prices"): prices, tag.format("sets", "stderrs"): errs, tag.format("sets", "stats"): stats,
                        tag.format("sets", "corr"): corr})
        for name, gammas in CD_GAMMAS.items():
            if variant == "large" and name != "g9":
                continue
            g = gammas.size
            nb = _size(E.svmc_cond_density_workspace_bytes, n, M, K, g)
            pdf, err, stats = np.empty(g * K), np.empty(g * K), np.empty(g * M * CD_STATS)
            _ok(E.svmc_cond_density_chain(mu, cv, n, M, _p(pts), _p(offs, SZP), _p(gammas), g, _p(pdf), _p(err), _p(stats), dev.alloc(nb), nb,
                                          None), "svmc_cond_density_chain")
            out.update({f"{variant}__density__{name}__pdf": pdf, f"{variant}__density__{name}__stderr": err,
                        f"{variant}__density__{name}__stats": stats})
    finally:
        dev.free()
    return out


def self_check(out: dict) -> list:
    """the outputs that break the rule of the module's docstring (statistics, corr and the forward block are not values)"""
    bad = []
    lo, hi = sum(COUNTS[:EMPTY_EXPIRY]), sum(COUNTS[:EMPTY_EXPIRY + 1])
    for name, arr in out.items():
        variant, entry, which, output = name.split("__")
        if output in ("stats", "fwd", "corr"):
            continue
        finite = np.isfinite(arr.reshape(-1, K)).copy()                # rows of [K]: one per gamma or set (and Greek)
        if variant == "no_kept_path":
            finite[:, lo:hi] = True
        if entry == "density":
            finite[np.flatnonzero(CD_GAMMAS[which] == DROP_GAMMA)] = True
        if not finite.all():
            bad.append(name)
    return bad


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run(libs, a: dict):
    """({out__name: the output's bits}, the names that break the self-check)"""
    out = {}
    for variant in VARIANTS:
        out.update(run_tails(libs, a, variant))
    return {"out__" + k: bits(v) for k, v in out.items()}, self_check(out)


# ---- the size functions on the grid -----------------------------------------------------------------------------------------------
SIZE_N, SIZE_MK, SIZE_Z = (1, 256, 257, 300000), ((1, 0), (1, 1), (3, 17), (16, 208)), (1, 4, 5, 16)
SIZE_FNS = ("svmc_tilted_cond_workspace_bytes", "svmc_tilted_cond_greeks_workspace_bytes", "svmc_cond_density_workspace_bytes",
            "svmc_jump_sets_workspace_bytes")


def size_fn(X, E, name):
    return getattr(X if name == "svmc_tilted_cond_workspace_bytes" else E, name)


def run_sizes(X, E) -> list:
    """[n][(m, K)][z][4]"""
    return [[[[_size(size_fn(X, E, f), n, m, k, z) for f in SIZE_FNS] for z in SIZE_Z] for m, k in SIZE_MK] for n in SIZE_N]


# ---- single-fault calls -------------------------------------------------------------------------------------------------------------
# The good call: two expiries of 1 and 5 quotes -- at both group widths the groups are as many as the size functions allow for, so that
# the size they return is the size the entry asks for -- 64 paths, one gamma or set.
ERR_COUNTS, ERR_N = (1, 5), 64
SIGNATURES = {
    "svmc_tilted_cond_payoff_chain": ("mu", "cv", "n_path", "forwards", "n_expiries", "strikes", "types", "shifts", "offsets", "gammas", "n_z",
                                      "recenter", "out0", "out1", "out2", "workspace", "workspace_bytes", "stream"),
    "svmc_tilted_cond_greeks_chain": ("mu", "cv", "n_path", "forwards", "n_expiries", "strikes", "types", "offsets", "gammas", "n_z", "recenter",
                                      "out0", "out1", "workspace", "workspace_bytes", "stream"),
    "svmc_cond_density_chain": ("mu", "cv", "n_path", "n_expiries", "points", "offsets", "gammas", "n_z", "out0", "out1", "out2", "workspace",
                                "workspace_bytes", "stream"),
    "svmc_jump_sets_payoff_chain": ("mu", "n_path", "forwards", "n_expiries", "strikes", "types", "shifts", "offsets", "variances", "gammas",
                                    "n_z", "recenter", "out0", "out1", "out2", "out3", "workspace", "workspace_bytes", "stream"),
}
WIDTH = {"svmc_tilted_cond_payoff_chain": 8, "svmc_tilted_cond_greeks_chain": 4, "svmc_cond_density_chain": 4, "svmc_jump_sets_payoff_chain": 4}
SIZE_OF = dict(zip(SIGNATURES, SIZE_FNS))
POINTERS = ("mu", "cv", "forwards", "strikes", "types", "shifts", "offsets", "gammas", "points", "variances", "out0", "out1", "out2", "out3",
            "workspace")
VALUES = {"strikes": "strike", "shifts": "shift", "points": "point", "gammas": "gamma"}


def _null(key):
    return lambda a: a.__setitem__(key, None)


def _set(key, value):
    return lambda a: a.__setitem__(key, value)


def _put(key, index, value):
    return lambda a: a[key].__setitem__(index, value)


def _null_row(key):
    return lambda a: a.__setitem__(key, (C.c_void_p * 2)(0x1000, None))


def _too_many_groups(a):
    k = 65535 * WIDTH[a["entry"]] + 1
    a.update(n_expiries=1, offsets=np.array([0, k], dtype=np.uintp), strikes=np.ones(k), shifts=np.zeros(k), points=np.zeros(k),
             types=np.zeros(k, dtype=np.int8))


def _too_many_expiries(a):
    m = 65536
    a.update(n_expiries=m, offsets=np.zeros(m + 1, dtype=np.uintp), mu=(C.c_void_p * m)(*[0x1000] * m), cv=(C.c_void_p * m)(*[0x1000] * m))


def _exact_workspace_less_one(a):
    a["workspace_bytes"] = a["need"] - 1


def defects(entry: str) -> list:
    """[(name, change)]: every single fault the entry refuses, in the order of its argument list"""
    args = SIGNATURES[entry]
    d = [("null_" + k, _null(k)) for k in args if k in POINTERS]
    d += [("null_row_" + k, _null_row(k)) for k in ("mu", "cv") if k in args]
    d += [("n_path_0", _set("n_path", 0)), ("n_expiries_0", _set("n_expiries", 0)), ("n_z_0", _set("n_z", 0)), ("n_z_17", _set("n_z", 17)),
          ("offsets_start_1", _put("offsets", 0, 1)), ("decreasing_offsets", _put("offsets", slice(0, 3), (0, 4, 3))),
          ("offset_above_2^30", _put("offsets", 2, (1 << 30) + 1)), ("too_many_groups", _too_many_groups)]
    if "forwards" in args:
        d += [("forward_0", _put("forwards", 0, 0.0)), ("forward_inf", _put("forwards", 1, np.inf)), ("forward_nan", _put("forwards", 1, np.nan)),
              ("forward_negative", _put("forwards", 0, -1.0))]
    d += [(f"{VALUES[k]}_{v}", _put(k, 0 if k == "gammas" else 4, float(v))) for k in args if k in VALUES for v in ("nan", "inf")]
    if "variances" in args:
        d += [("variance_negative", _put("variances", 1, -1e-9)), ("variance_nan", _put("variances", 0, np.nan)),
              ("variance_inf", _put("variances", 1, np.inf))]
    if "types" in args:
        d += [("type_2", _put("types", 1, 2)), ("type_-1", _put("types", 5, -1))]
    if entry == "svmc_cond_density_chain":
        d.append(("too_many_expiries", _too_many_expiries))
    return d + [("workspace_one_byte_short", _exact_workspace_less_one)]


def base_arguments(entry: str, need: int) -> dict:
    """a good call of `entry` but for its workspace of 8 bytes; fresh arrays, so that a defect may write into them"""
    m, k = len(ERR_COUNTS), sum(ERR_COUNTS)
    return dict(entry=entry, need=need, mu=(C.c_void_p * m)(*[0x1000] * m), cv=(C.c_void_p * m)(*[0x1000] * m), n_path=ERR_N,
                forwards=np.array([1.0, 1.05]), n_expiries=m, strikes=np.linspace(0.8, 1.2, k), types=np.array([1, 0, 0, 1, 1, 0], dtype=np.int8),
                shifts=np.zeros(k), points=np.linspace(-0.3, 0.3, k), offsets=np.array([0, ERR_COUNTS[0], k], dtype=np.uintp),
                gammas=np.array([0.5]), variances=np.array([0.02, 0.04]), n_z=1, recenter=1, out0=np.zeros(64 * k), out1=np.zeros(64 * k),
                out2=np.zeros(64 * k), out3=np.zeros(64), workspace=C.c_void_p(0x1000), workspace_bytes=8, stream=None)


def call(fn, entry: str, change, need: int) -> int:
    a = base_arguments(entry, need)
    if change is not None:
        change(a)
    assert len(fn.argtypes) == len(SIGNATURES[entry]), entry
    args = []
    for key, ctype in zip(SIGNATURES[entry], fn.argtypes):
        v = a[key]
        args.append(C.cast(v.ctypes.data_as(C.c_void_p), ctype) if isinstance(v, np.ndarray) else v)
    return int(fn(*args))


def run_refusals(X, E) -> list:
    """[[entry, case, status]]; nothing is launched: every call's workspace is too small for it"""
    table = []
    for entry in SIGNATURES:
        fn = getattr(X if entry == "svmc_tilted_cond_payoff_chain" else E, entry)
        need = _size(size_fn(X, E, SIZE_OF[entry]), ERR_N, len(ERR_COUNTS), sum(ERR_COUNTS), 1)
        if call(fn, entry, None, need) != ERR_WORKSPACE:
            raise RuntimeError(f"{entry}: the good call is not refused for its workspace")
        for name, change in defects(entry):
            rc = call(fn, entry, change, need)
            if rc == OK or (rc == ERR_WORKSPACE) != (name == "workspace_one_byte_short"):
                raise RuntimeError(f"{entry} / {name}: status {rc} -- the case does not belong in this table")
            table.append([entry, name, rc])
    return table


def run_host(X, E) -> dict:
    return {"sizes": run_sizes(X, E), "refusals": run_refusals(X, E)}


if __name__ == "__main__":
    from stochvolmodels_amd import _lib
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "host":
        target = sys.argv[2] if len(sys.argv) > 2 else HOST_FIXTURE
        rec = run_host(_lib.load_ext(), _lib.load_est())
        with open(target, "w") as fh:
            json.dump(rec, fh, separators=(",", ":"))
            fh.write("\n")
        print(f"{len(rec['refusals'])} refusals, {np.array(rec['sizes']).size} sizes -> {target} ({os.path.getsize(target)} bytes)")
    elif mode == "gpu":
        target = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
        libs = (_lib.load(), _lib.load_ext(), _lib.load_est())
        inputs = make_inputs()
        recorded, broken = run(libs, inputs)
        np.savez_compressed(target, **{"in__" + k: v for k, v in inputs.items()}, **recorded)
        print(f"{len(recorded)} outputs -> {target} ({os.path.getsize(target)} bytes)")
        if broken:
            sys.exit("non-finite values where the docstring allows none: " + ", ".join(broken))
        rec = np.load(target, allow_pickle=False)
        again, _ = run(libs, {k[4:]: rec[k] for k in rec.files if k.startswith("in__")})
        wrong = [k for k in again if not np.array_equal(again[k], rec[k])]
        if wrong or set(again) != {k for k in rec.files if k.startswith("out__")}:
            sys.exit("the file does not replay on the build that wrote it: " + ", ".join(wrong[:6]))
        print("replayed: every output equal to the bit")
    else:
        sys.exit(__doc__)
