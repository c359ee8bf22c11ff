"""
Record tests/golden/quote_tails.npz: what the four payoff tails that work on a chain's quote table -- svmc_greeks_payoff_chain,
svmc_cmc_payoff_chain, svmc_cmc_greeks_chain, svmc_cmc_sens_chain -- answer on synthetic device arrays, bit for bit; what the five
workspace size functions return on a grid; and the status code and svmc_last_error text with which the four tails and the four
fused drivers (svmc_{logsv,heston}_chain_price_{cmc_sens,greeks}) refuse a chain with ONE fault.  This project's own output,
recorded on a GPU box:

    python tests/golden/make_golden_quote_tails.py          # writes the fixture

Recorded on commit 9dbc6b8 ("Hold the volatility-path kernel and its reducers to exact references"), the parent of the change
that gave the four tails one quote check, one table image builder and one workspace layout each; tests/test_gpu_quote_tails.py
replays the file on every later build.

The inputs are stored in the file.  n_path = 2 x 256 + 37 (three path blocks, the last partial: the in-order column sums have more
than one row); five expiries of 1, 0, 9, 8 and 0 strikes (an empty expiry in the middle and at the end, a ragged group at both
group widths, 8 and 4, and a full group of 8), calls and puts mixed within an expiry; P = 2.  Three variants:
  planted        one cv == 0, one cv < 0, one NaN mu and one +inf mu per row (log-return rows: one NaN and one -inf -- a path at
                 +inf is an infinite payoff there, not a dropped path);
  path0_dropped  path 0 of every row is NaN besides: the intrinsic shift and the (0, 0) pair shift;
  no_kept_path   expiry 2 keeps no path besides: the 0 / 0 rows.
In every variant every recorded price, error and sensitivity is finite, except, in no_kept_path, the quotes of expiry 2.
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
FIXTURE = os.path.join(HERE, "quote_tails.npz")

N_PATH, COUNTS, P = 2 * 256 + 37, (1, 0, 9, 8, 0), 2
M, K = len(COUNTS), sum(COUNTS)
VARIANTS = ("planted", "path0_dropped", "no_kept_path")
EMPTY_EXPIRY = 2                                   # the expiry of no_kept_path that keeps no path (quotes 1 .. 9)
CMC_STATS, CMC_GREEKS_STATS, CMC_GREEKS_ROWS, SENS_ROWS, GREEKS_BASE_ROWS = 5, 6, 10, 3, 5
ERR_WORKSPACE = 5
DP = C.POINTER(C.c_double)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------
def make_inputs() -> dict:
    """{name: array} of the chain and, per variant, the rows of the four tails"""
    rng = np.random.default_rng(20261020)
    forwards = np.array([1.0, 1.02, 0.98, 1.05, 1.01])
    offsets = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.uintp)
    strikes = np.concatenate([forwards[i] * np.linspace(0.8, 1.2, c) if c > 1 else forwards[i] * np.full(c, 0.95)
                              for i, c in enumerate(COUNTS)])
    types = (np.arange(K) % 2 == 0).astype(np.int8)             # put, call, put, ... : both codes in every expiry of two or more
    a = dict(forwards=forwards, discfactors=np.array([0.99, 0.98, 0.97, 0.96, 0.95]), offsets=offsets, strikes=strikes, types=types,
             steps=np.array([0.01, 0.05]))
    scale = np.sqrt(np.arange(1, M + 1))[:, None]
    mu = -0.01 * scale ** 2 + 0.15 * scale * rng.standard_normal((M, N_PATH))
    cv = (0.004 + 0.02 * rng.random((M, N_PATH))) * scale ** 2
    x = -0.02 * scale ** 2 + 0.2 * scale * rng.standard_normal((M, N_PATH))
    bump = np.arange(1, P + 1)[:, None, None]
    dmu, dx = 0.004 * bump * rng.standard_normal((P, M, N_PATH)), 0.003 * bump * rng.standard_normal((P, M, N_PATH))
    for v, variant in enumerate(VARIANTS):
        rows = dict(mu=mu.copy(), cv=cv.copy(), up_mu=mu + dmu, up_cv=cv * (1 + 0.02 * bump), dn_mu=mu - dmu, dn_cv=cv * (1 - 0.02 * bump),
                    x=x.copy(), x_up=x + dx, x_dn=x - dx)
        for name in ("cv", "up_cv"):
            rows[name][..., 5] = 0.0
        for name in ("cv", "dn_cv"):
            rows[name][..., 17] = -0.01
        for name in ("mu", "up_mu", "x", "x_up"):
            rows[name][..., 300] = np.nan
        for name in ("mu", "dn_mu"):
            rows[name][..., N_PATH - 1] = np.inf
        rows["x_dn"][..., N_PATH - 1] = -np.inf
        if v >= 1:
            for name in ("mu", "up_mu", "x", "x_up"):
                rows[name][..., 0] = np.nan
        if v >= 2:
            for name in ("cv", "up_cv", "dn_cv"):
                rows[name][..., EMPTY_EXPIRY, :] = -1.0
            for name in ("x", "x_up", "x_dn"):
                rows[name][..., EMPTY_EXPIRY, :] = np.nan
        # the Greeks tail's spot sums [1 + 2P][m][2] = [sum F exp(x), count] over the paths with a finite exp(x), job-major
        jobs = [rows["x"]] + [rows[k][p] for p in range(P) for k in ("x_up", "x_dn")]
        with np.errstate(all="ignore"):
            spot = np.array([[[(forwards[i] * np.exp(r[np.isfinite(np.exp(r))])).sum(), np.isfinite(np.exp(r)).sum()] for i, r in enumerate(job)]
                             for job in jobs], dtype=np.float64)
        rows["spot_sums"] = spot
        for name, arr in rows.items():
            a[f"{variant}__{name}"] = np.ascontiguousarray(arr, dtype=np.float64)
    return a


# ---- device memory through the library's own allocator --------------------------------------------------------------------------
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

    def put(self, a: np.ndarray) -> int:
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = self.alloc(a.nbytes)
        self.check(self.L.svmc_memcpy_h2d(p, a.ctypes.data, a.nbytes, None))
        self.check(self.L.svmc_stream_synchronize(None))
        return p

    def rows(self, a: np.ndarray):
        """the rows of a [..., n] array on the device as a C array of pointers, in C order"""
        a = np.ascontiguousarray(a, dtype=np.float64)
        base, n = self.put(a), a.shape[-1]
        count = a.size // n
        return (C.c_void_p * max(count, 1))(*[base + 8 * n * r for r in range(count)])

    def free(self):
        for p in self.owned:
            self.check(self.L.svmc_free(p))
        self.owned = []


def _size(L, name, *args) -> int:
    from stochvolmodels_amd import _lib
    out = C.c_size_t(0)
    _lib.check(getattr(L, name)(*args, C.byref(out)))
    return out.value


def _p(a, ctype=C.c_double):
    return a.ctypes.data_as(C.POINTER(ctype))


# ---- the four tails on one variant ---------------------------------------------------------------------------------------------
def run_tails(L, a: dict, variant: str) -> dict:
    """{variant__entry__rR__output: array} of the four entry points on the variant's rows (recenter 0 and 1 where the tail has it)"""
    from stochvolmodels_amd import _lib
    g = lambda name: a[f"{variant}__{name}"]                 # noqa: E731
    dev, out = Device(L), {}
    chain = (_p(a["forwards"]), _p(a["discfactors"]), M, _p(a["strikes"]), _p(a["types"], C.c_int8), _p(a["offsets"], C.c_size_t))
    try:
        mu, cv = dev.rows(g("mu")), dev.rows(g("cv"))
        ups, dns = (dev.rows(g("up_mu")), dev.rows(g("up_cv"))), (dev.rows(g("dn_mu")), dev.rows(g("dn_cv")))
        x, x_up, x_dn, spot = dev.rows(g("x")), dev.rows(g("x_up")), dev.rows(g("x_dn")), dev.put(g("spot_sums"))
        for recenter in (0, 1):
            tag = f"{variant}__{{}}__r{recenter}__{{}}"
            nb = _size(L, "svmc_cmc_payoff_workspace_bytes", N_PATH, M, K)
            prices, stderrs, stats = np.empty(K), np.empty(K), np.empty((M, CMC_STATS))
            _lib.check(L.svmc_cmc_payoff_chain(mu, cv, N_PATH, *chain, recenter, _p(prices), _p(stderrs), _p(stats), dev.alloc(nb), nb, None))
            out.update({tag.format("cmc_payoff", "prices"): prices, tag.format("cmc_payoff", "stderrs"): stderrs,
                        tag.format("cmc_payoff", "stats"): stats})
            nb = _size(L, "svmc_cmc_greeks_workspace_bytes", N_PATH, M, K)
            greeks, stats = np.empty((CMC_GREEKS_ROWS, K)), np.empty((M, CMC_GREEKS_STATS))
            _lib.check(L.svmc_cmc_greeks_chain(mu, cv, N_PATH, *chain, recenter, _p(greeks), _p(stats), dev.alloc(nb), nb, None))
            out.update({tag.format("cmc_greeks", "greeks"): greeks, tag.format("cmc_greeks", "stats"): stats})
            nb = _size(L, "svmc_cmc_sens_workspace_bytes", N_PATH, M, K, P)
            sens = np.empty((P, SENS_ROWS, K))
            _lib.check(L.svmc_cmc_sens_chain(ups[0], ups[1], dns[0], dns[1], N_PATH, *chain, P, _p(a["steps"]), recenter, _p(sens),
                                             dev.alloc(nb), nb, None))
            out[tag.format("cmc_sens", "sens")] = sens
        nb = _size(L, "svmc_greeks_payoff_workspace_bytes", N_PATH, M, K, P)
        base, sens = np.empty((GREEKS_BASE_ROWS, K)), np.empty((P, SENS_ROWS, K))
        _lib.check(L.svmc_greeks_payoff_chain(x, x_up, x_dn, N_PATH, *chain, P, _p(a["steps"]), spot, _p(base), _p(sens), dev.alloc(nb), nb, None))
        out.update({f"{variant}__greeks_payoff__base": base, f"{variant}__greeks_payoff__sens": sens})
    finally:
        dev.free()
    return out


def values_of(name: str, arr: np.ndarray):
    """the prices, errors and sensitivities of a recorded output as [..., K] (counts and statistics: none)"""
    if name.endswith("__stats"):
        return None
    if name.endswith("__sens"):
        return arr[:, :2, :]
    if name.endswith("__base"):
        return arr[:4, :]
    return arr


def self_check(out: dict) -> list:
    """the outputs that break the rule of the module's docstring"""
    bad = []
    lo, hi = sum(COUNTS[:EMPTY_EXPIRY]), sum(COUNTS[:EMPTY_EXPIRY + 1])
    for name, arr in out.items():
        v = values_of(name, arr)
        if v is None:
            continue
        finite = np.isfinite(v)
        if name.startswith("no_kept_path"):
            finite = finite.copy()
            finite[..., lo:hi] = True
        if not finite.all():
            bad.append(name)
    return bad


# ---- the five size functions on the grid ---------------------------------------------------------------------------------------
SIZE_N, SIZE_MK, SIZE_P = (1, 256, 257, 300000), ((1, 0), (1, 1), (3, 17), (16, 208)), (1, 6, 31)


def run_sizes(L) -> np.ndarray:
    """[n][(m, K)][P][5]: cmc payoff, cmc greeks, cmc sens, greeks payoff, and cmc many at (1 + 2P jobs, m slices)"""
    out = np.zeros((len(SIZE_N), len(SIZE_MK), len(SIZE_P), 5), dtype=np.uint64)
    for i, n in enumerate(SIZE_N):
        for j, (m, k) in enumerate(SIZE_MK):
            for q, p in enumerate(SIZE_P):
                out[i, j, q] = (_size(L, "svmc_cmc_payoff_workspace_bytes", n, m, k), _size(L, "svmc_cmc_greeks_workspace_bytes", n, m, k),
                                _size(L, "svmc_cmc_sens_workspace_bytes", n, m, k, p), _size(L, "svmc_greeks_payoff_workspace_bytes", n, m, k, p),
                                _size(L, "svmc_cmc_many_workspace_bytes", 1 + 2 * p, m))
    return out


# ---- single-fault cases ------------------------------------------------------------------------------------------------------
ERR_N, ERR_M, ERR_K, ERR_P, MAX_M = 64, 2, 6, 1, 17
QUOTES = ("forwards", "discfactors", "n_expiries", "strikes", "types", "offsets")
SIGNATURES = {
    "svmc_cmc_payoff_chain": ("rows", "rows", "n_path") + QUOTES + ("recenter", "out", "out", "out", "workspace", "workspace_bytes", "stream"),
    "svmc_cmc_greeks_chain": ("rows", "rows", "n_path") + QUOTES + ("recenter", "out", "out", "workspace", "workspace_bytes", "stream"),
    "svmc_cmc_sens_chain": ("rows", "rows", "rows", "rows", "n_path") + QUOTES + ("n_params", "steps", "recenter", "out", "workspace",
                                                                                  "workspace_bytes", "stream"),
    "svmc_greeks_payoff_chain": ("rows", "rows", "rows", "n_path") + QUOTES + ("n_params", "steps", "workspace", "out", "out", "workspace",
                                                                               "workspace_bytes", "stream"),
    "svmc_logsv_chain_price_cmc_sens": ("session", "ttms") + QUOTES + ("n_params", "params", "steps", "mode", "nb_steps_per_year", "recenter",
                                                                       "seed", "call_id", "out", "out", "out"),
    "svmc_heston_chain_price_cmc_sens": ("session", "ttms") + QUOTES + ("n_params", "params", "steps", "nb_steps_per_year", "recenter", "seed",
                                                                        "call_id", "out", "out", "out"),
    "svmc_logsv_chain_price_greeks": ("session", "ttms") + QUOTES + ("n_params", "params", "steps", "mode", "nb_steps_per_year", "seed",
                                                                     "call_id", "out", "out", "out", "out"),
    "svmc_heston_chain_price_greeks": ("session", "ttms") + QUOTES + ("n_params", "params", "steps", "mode", "nb_steps_per_year", "seed",
                                                                      "call_id", "out", "out", "out", "out"),
}
TAILS = tuple(n for n in SIGNATURES if "chain_price" not in n)
FUSED = tuple(n for n in SIGNATURES if n not in TAILS)
STEPPED = ("svmc_cmc_sens_chain", "svmc_greeks_payoff_chain")
EVERY = tuple(SIGNATURES)
# (the conditional payoff tail and its derivative tail take any discount factor: a non-finite one gives non-finite prices)
DF_CHECKED = tuple(n for n in SIGNATURES if n not in ("svmc_cmc_payoff_chain", "svmc_cmc_greeks_chain"))
# the strike count at which each tail answers "too many strikes" (the sensitivity tail counts 2 P K, here P = 1)
TOO_MANY = {"svmc_cmc_payoff_chain": 1 << 30, "svmc_cmc_greeks_chain": 1 << 30, "svmc_cmc_sens_chain": 1 << 29, "svmc_greeks_payoff_chain": 1 << 24}


def _null(key):
    return lambda a: a.__setitem__(key, None)


def _set(key, value):
    return lambda a: a.__setitem__(key, value)


def _put(key, index, value):
    return lambda a: a[key].__setitem__(index, value)


def _too_many(a):
    k = TOO_MANY[a["entry"]]
    a.update(n_expiries=1, offsets=np.array([0, k], dtype=np.uintp), strikes=np.zeros(k), types=np.zeros(k, dtype=np.int8))


# (name, the entry points it is recorded for, what it does to a good call's arguments): one per check of the quotes ...
DEFECTS = [
    ("null_forwards", EVERY, _null("forwards")),
    ("null_discfactors", EVERY, _null("discfactors")),
    ("null_strikes", EVERY, _null("strikes")),
    ("null_types", EVERY, _null("types")),
    ("null_offsets", EVERY, _null("offsets")),
    ("n_path_0", TAILS, _set("n_path", 0)),
    ("n_expiries_0", EVERY, _set("n_expiries", 0)),
    ("decreasing_offsets", EVERY, _put("offsets", slice(0, 3), (0, 4, 3))),
    ("forward_nan", EVERY, _put("forwards", 1, np.nan)),
    ("forward_inf", EVERY, _put("forwards", 1, np.inf)),
    ("forward_0", EVERY, _put("forwards", 0, 0.0)),
    ("forward_negative", EVERY, _put("forwards", 1, -1.0)),
    ("discfactor_nan", DF_CHECKED, _put("discfactors", 0, np.nan)),
    ("discfactor_inf", DF_CHECKED, _put("discfactors", 1, np.inf)),
    ("payoff_code_7", EVERY, _put("types", 2, 7)),
    ("payoff_code_2", EVERY, _put("types", 5, 2)),
    ("strike_nan", EVERY, _put("strikes", 0, np.nan)),
    ("strike_inf", EVERY, _put("strikes", 5, np.inf)),
    ("too_many_strikes", TAILS, _too_many),
    # ... and per check of the steps
    ("n_params_-1", STEPPED, _set("n_params", -1)),
    ("n_params_0", ("svmc_cmc_sens_chain",), _set("n_params", 0)),
    ("n_params_32", STEPPED, _set("n_params", 32)),
    ("null_steps", STEPPED, _null("steps")),
    ("step_0", STEPPED, _put("steps", 0, 0.0)),
    ("step_negative", STEPPED, _put("steps", 0, -0.01)),
    ("step_nan", STEPPED, _put("steps", 0, np.nan)),
    ("step_inf", STEPPED, _put("steps", 0, np.inf)),
]


def cases():
    for entry in SIGNATURES:
        for name, entries, change in DEFECTS:
            if entry in entries:
                yield entry, name, change


def base_arguments(entry: str, session, dummy) -> dict:
    """a good call of `entry` but for the workspace of 0 bytes of the four tails, which a chain without a fault would be refused for
    (it is never launched); fresh arrays, so that a defect may write into them"""
    jobs = 1 + 2 * ERR_P
    a = dict(entry=entry, session=session, rows=(C.c_void_p * (32 * MAX_M))(*[dummy] * (32 * MAX_M)), n_path=ERR_N,
             ttms=0.1 * np.arange(1, MAX_M + 1), forwards=np.linspace(1.0, 1.1, MAX_M), discfactors=np.ones(MAX_M), n_expiries=ERR_M,
             strikes=np.linspace(0.8, 1.2, ERR_K + 1), types=np.array([1, 0, 0, 1, 1, 0, 0], dtype=np.int8),
             offsets=np.array([0, 3] + [ERR_K] * (MAX_M - 1), dtype=np.uintp), n_params=ERR_P, steps=np.full(32, 0.01), recenter=1,
             out=np.zeros(64 * (ERR_K + 1) * MAX_M), workspace=dummy, workspace_bytes=0, stream=None, mode=1, nb_steps_per_year=120, seed=7,
             call_id=0)
    if "logsv" in entry:
        a["params"] = np.tile(np.array([0.8, 1.0, 3.0, 3.0, 0.15, 1.8] + [1.0] * MAX_M), (jobs, 1))
    else:
        a["params"] = np.tile(np.array([0.04, 0.04, 3.0, -0.5, 0.4]), (jobs, 1))
        a["mode"] = 0                                            # (the Heston Greeks driver's scheme code)
    return a


def call(L, entry: str, change, session, dummy):
    a = base_arguments(entry, session, dummy)
    change(a)
    fn = getattr(L, entry)
    assert len(fn.argtypes) == len(SIGNATURES[entry]), entry
    args = []
    for key, ctype in zip(SIGNATURES[entry], fn.argtypes):
        v = a[key]
        args.append(C.cast(v.ctypes.data_as(C.c_void_p), ctype) if isinstance(v, np.ndarray) else v)
    rc = fn(*args)
    return int(rc), L.svmc_last_error().decode("utf-8", "replace")


def run_errors(L) -> list:
    """[[entry point, case, status, message]]; every case is refused before anything is launched"""
    from stochvolmodels_amd import _lib
    session, dev = C.c_void_p(), Device(L)
    _lib.check(L.svmc_session_create(C.byref(session), ERR_N, ERR_M, ERR_K))
    try:
        dummy = dev.alloc(8)
        table = []
        for entry, name, change in cases():
            rc, message = call(L, entry, change, session, dummy)
            if rc == 0 or (rc == ERR_WORKSPACE and "workspace too small" in message):
                raise RuntimeError(f"{entry} / {name} passed the checks ({rc}, {message!r}): it does not belong in this table")
            table.append([entry, name, rc, message])
        return table
    finally:
        dev.free()
        _lib.check(L.svmc_session_destroy(session))


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run(L, a: dict):
    """everything the fixture records besides the inputs: the outputs as uint64 views, the size grid, the error table as JSON"""
    out = {}
    for variant in VARIANTS:
        out.update(run_tails(L, a, variant))
    bad = self_check(out)
    rec = {"out__" + k: bits(v) for k, v in out.items()}
    rec["sizes"] = run_sizes(L)
    rec["errors"] = np.array(json.dumps(run_errors(L)))
    return rec, bad


if __name__ == "__main__":
    from stochvolmodels_amd import _lib
    target = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    inputs = make_inputs()
    recorded, broken = run(_lib.load(), inputs)
    np.savez_compressed(target, **{"in__" + k: v for k, v in inputs.items()}, **recorded)
    print(f"{len(recorded) - 2} outputs, {len(json.loads(str(recorded['errors'])))} error cases -> {target} ({os.path.getsize(target)} bytes)")
    if broken:
        sys.exit("non-finite values where the docstring allows none: " + ", ".join(broken))
