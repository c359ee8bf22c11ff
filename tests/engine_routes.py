"""Shared by tests/golden/make_golden_engine_calls.py, tests/test_engine_calls_host.py and tests/test_gpu_engine_routes_bits.py: one
list of HipEngine routes on one small chain, run two ways.

Host (record_host): every route on a HipEngine made with __new__ over a library stand-in that records each C call -- scalars by
value, pointer arguments by the contents they point at, read to the length include/svmc.h (svmc_ext.h, svmc_est.h) documents for
that argument, device addresses as the stand-in engine hands them out -- and fills every output to its documented length, so that
what a route returns pins where its output pointers pointed and how it cut the rows.  Refusals are recorded as (type, text, the C
calls made before).

GPU (run_gpu): the same routes in the same order on ONE engine of N_PATH paths (later routes read the rows earlier ones left), then
the public pricer functions over them; every numeric leaf of every result, and per route the kernel names the engine's timer
reports.
"""
import ctypes as C
import hashlib
import json
import types

import numpy as np

N_PATH, SPY, SEED, CALL_ID = 1000, 12, 7, 3          # 1000: a multiple of neither 64 nor 256
J, P, G = 3, 2, 2                                    # jobs, parameter sets / bumped parameters, gammas
GAMMAS = [-0.5, 1.0]
LOGSV = (0.8, 1.0, 3.0, 3.0, 0.15, 1.8)              # v0 theta kappa1 kappa2 beta volvol
HESTON = (0.04, 0.05, 3.0, -0.5, 0.4)                # v0 theta kappa rho volvol
HAWKES = np.array([0.0, 0.45, 0.06, 0.03, -0.06, -0.03, 6.55, 6.55, 22.29, 76.0, -67.58, 8.5, 8.5, 29.0, 104.55, -109.6])
STEPS = [1e-3, 2e-3]


def chain(m=3):
    """3 expiries with strikes of shape (2, 2), (3,) and (1,): all offsets and shapes distinct; m=1: the same chain cut to one"""
    c = types.SimpleNamespace(m=m)
    c.ttms = np.array([1.0 / 12.0, 0.25, 0.5])[:m]
    c.forwards = np.array([1.0, 1.01, 1.02])[:m]
    c.disc = np.array([0.999, 0.99, 0.98])[:m]
    c.strikes = [np.array([[0.9, 1.0], [1.05, 1.1]]), np.array([0.95, 1.0, 1.1]), np.array([1.02])][:m]
    c.codes = [np.array([1, 1, 0, 0], dtype=np.int8), np.array([1, 0, 0], dtype=np.int8), np.array([0], dtype=np.int8)][:m]
    c.types = [np.where(k == 0, "C", "P").reshape(s.shape) for k, s in zip(c.codes, c.strikes)]
    c.K = sum(k.size for k in c.strikes)
    c.etas = np.array([1.0, 0.9, 1.1])[:m]
    return c


def logsv_rows(c, n):
    return np.array([[v * (1.0 + 0.01 * j) for v in LOGSV] + list(c.etas) for j in range(n)])


def heston_rows(n):
    return np.array([[v * (1.0 + 0.01 * j) for v in HESTON] for j in range(n)])


def hawkes_rows(n):
    return np.array([HAWKES * (1.0 + 0.01 * j) for j in range(n)])


def host_row(k, positive=False):
    """a deterministic row of N_PATH values: log-returns, or (positive) conditional variances"""
    t = np.arange(N_PATH, dtype=np.float64)
    return 0.01 + 0.005 * np.cos(0.37 * (k + 1) * t) ** 2 if positive else 0.05 * np.sin(0.61 * (k + 1) * t) - 0.01


def grid(c):
    nbs, dts, t0 = [], [], 0.0
    for t in c.ttms:
        nb = int((float(t) - t0) * SPY) + 1
        nbs.append(nb)
        dts.append((float(t) - t0) / nb)
        t0 = float(t)
    return nbs, dts


SEEDS, IDS = [11, 12, 13], [0, 1, 2]


def _marshalled(c):
    from stochvolmodels_amd.engine import marshalled_chain
    return marshalled_chain(c.ttms, c.forwards, c.disc, c.strikes, c.codes)


def _tilted(c):
    from stochvolmodels_amd.engine import tilted_chain_arrays
    return tilted_chain_arrays(c.forwards, c.strikes, c.codes, GAMMAS, ttms=c.ttms)


def _rows(m, job):
    return list(range(job * m, (job + 1) * m))


def _sens_host_rows(m):
    """(mu_up, cv_up, mu_dn, cv_dn), each [P][m] host arrays"""
    return tuple([[host_row(17 * a + 5 * p + i, positive=a % 2 == 1) for i in range(m)] for p in range(P)] for a in range(4))


def _sens_rows(m, which):
    """the snapshot rows conditional_sens' host_rows branch uploads to: blocks mu_up, cv_up, mu_dn, cv_dn of P m rows each"""
    a = 0 if which == "up" else 2
    return [([(a * P + p) * m + i for i in range(m)], [((a + 1) * P + p) * m + i for i in range(m)]) for p in range(P)]


def _greeks_host_rows(m):
    return ([host_row(i) for i in range(m)], [[host_row(3 + 7 * p + i) for i in range(m)] for p in range(P)],
            [[host_row(5 + 11 * p + i) for i in range(m)] for p in range(P)])


def sens_table(rows):
    """[1 + 2P][W]: the base row, then per step an up and a dn row bumping parameter 1 + p"""
    out = [rows[0]]
    for p, h in enumerate(STEPS):
        for s in (+1.0, -1.0):
            r = rows[0].copy()
            r[1 + p] += s * h
            out.append(r)
    return np.array(out)


# (name, W of the route's parameter rows, route(engine, chain)); the order is the GPU order: a route may read what an earlier one left
ROUTES = [
    ("logsv_fused", 0, lambda e, c: e.price_logsv_chain_fused(_marshalled(c), *LOGSV, c.etas, True, SPY, 1, SEED, CALL_ID)),
    ("heston_fused", 0, lambda e, c: e.price_heston_chain_fused(_marshalled(c), *HESTON, 0, SPY, 1, SEED, CALL_ID)),
    ("heston_fused_qe", 0, lambda e, c: e.price_heston_chain_fused(_marshalled(c), *HESTON, 1, SPY, 1, SEED, CALL_ID)),
    ("hawkesjd_fused", 16, lambda e, c: e.price_hawkesjd_chain_fused(_marshalled(c), HAWKES, SPY, 1, SEED, CALL_ID)),
    ("logsv_cmc_fused", 0, lambda e, c: e.price_logsv_chain_cmc_fused(_marshalled(c), *LOGSV, c.etas, True, SPY, True, SEED, CALL_ID)),
    ("heston_cmc_fused", 0, lambda e, c: e.price_heston_chain_cmc_fused(_marshalled(c), *HESTON, SPY, False, SEED, CALL_ID)),
    ("hawkesjd_cmc_fused", 16, lambda e, c: e.price_hawkesjd_chain_cmc_fused(_marshalled(c), HAWKES, SPY, True, SEED, CALL_ID)),
    ("logsv_cmc_greeks_fused", 0,
     lambda e, c: e.price_logsv_chain_cmc_greeks_fused(_marshalled(c), *LOGSV, c.etas, True, SPY, True, SEED, CALL_ID)),
    ("heston_cmc_greeks_fused", 0, lambda e, c: e.price_heston_chain_cmc_greeks_fused(_marshalled(c), *HESTON, SPY, True, SEED, CALL_ID)),
    ("hawkesjd_cmc_greeks_fused", 16,
     lambda e, c: e.price_hawkesjd_chain_cmc_greeks_fused(_marshalled(c), HAWKES, SPY, False, SEED, CALL_ID)),
    ("many_fused_logsv", -1, lambda e, c: e.price_chain_many_fused(_marshalled(c), "logsv", logsv_rows(c, J), SEEDS, IDS, 1, SPY, 1)),
    ("many_fused_heston", 5, lambda e, c: e.price_chain_many_fused(_marshalled(c), "heston", heston_rows(J), SEEDS, IDS, 1, SPY, 1)),
    ("many_fused_hawkesjd", 16, lambda e, c: e.price_chain_many_fused(_marshalled(c), "hawkesjd", hawkes_rows(J), SEEDS, IDS, 0, SPY, 1)),
    ("cmc_many_fused_logsv", -1,
     lambda e, c: e.price_chain_cmc_many_fused(_marshalled(c), "logsv", logsv_rows(c, J), SEEDS, IDS, 1, SPY, True)),
    ("cmc_many_fused_heston", 5,
     lambda e, c: e.price_chain_cmc_many_fused(_marshalled(c), "heston", heston_rows(J), SEEDS, IDS, 0, SPY, False)),
    ("cmc_sens_fused_logsv", -1,
     lambda e, c: e.price_chain_cmc_sens_fused(_marshalled(c), "logsv", sens_table(logsv_rows(c, 1)), STEPS, 1, SPY, True, SEED, CALL_ID)),
    ("cmc_sens_fused_heston", 5,
     lambda e, c: e.price_chain_cmc_sens_fused(_marshalled(c), "heston", sens_table(heston_rows(1)), STEPS, 0, SPY, True, SEED, CALL_ID)),
    ("cmc_sets_fused_logsv_ivols", -1,
     lambda e, c: e.price_chain_cmc_sets_fused(_marshalled(c), "logsv", logsv_rows(c, P), 1, SPY, True, SEED, CALL_ID, want_ivols=True)),
    ("cmc_sets_fused_logsv", -1,
     lambda e, c: e.price_chain_cmc_sets_fused(_marshalled(c), "logsv", logsv_rows(c, P), 1, SPY, True, SEED, CALL_ID, want_ivols=False)),
    ("cmc_sets_fused_heston_ivols", 5,
     lambda e, c: e.price_chain_cmc_sets_fused(_marshalled(c), "heston", heston_rows(P), 0, SPY, False, SEED, CALL_ID, want_ivols=True)),
    ("cmc_sets_fused_heston", 5,
     lambda e, c: e.price_chain_cmc_sets_fused(_marshalled(c), "heston", heston_rows(P), 0, SPY, False, SEED, CALL_ID, want_ivols=False)),
    ("greeks_fused_logsv", -1,
     lambda e, c: e.price_chain_greeks_fused(_marshalled(c), "logsv", sens_table(logsv_rows(c, 1)), STEPS, 1, SPY, SEED, CALL_ID)),
    ("greeks_fused_heston", 5,
     lambda e, c: e.price_chain_greeks_fused(_marshalled(c), "heston", sens_table(heston_rows(1)), STEPS, 1, SPY, SEED, CALL_ID)),
    ("tilted_fused", 16, lambda e, c: e.price_hawkesjd_chain_tilted_fused(_tilted(c), HAWKES, SPY, SEED, CALL_ID, GAMMAS, True)),
    ("tilted_many_fused", 16,
     lambda e, c: e.price_hawkesjd_chain_tilted_many_fused(_tilted(c), hawkes_rows(J), SPY, SEEDS, IDS,
                                                           np.array([GAMMAS, [0.0, 0.5], [1.0, -1.0]]), False)),
    ("step_cond_rows", 16, lambda e, c: e.step_hawkesjd_chain_cond_rows(_tilted(c), HAWKES, SPY, SEED, CALL_ID)),
    ("conditional_payoffs", 0,
     lambda e, c: e.conditional_payoffs(c.forwards, c.disc, c.strikes, c.codes, True, mu_rows=_rows(c.m, 0), cv_rows=_rows(c.m, 1))),
    ("conditional_greeks", 0,
     lambda e, c: e.conditional_greeks(c.forwards, c.disc, c.strikes, c.codes, False, mu_rows=_rows(c.m, 0), cv_rows=_rows(c.m, 1))),
    ("tilted_conditional_payoffs", 0,
     lambda e, c: e.tilted_conditional_payoffs(c.forwards, c.strikes, c.codes, GAMMAS, True, mu_rows=_rows(c.m, 0), cv_rows=_rows(c.m, 1))),
    ("tilted_conditional_greeks", 0,
     lambda e, c: e.tilted_conditional_greeks(c.forwards, c.strikes, c.codes, GAMMAS, False, mu_rows=_rows(c.m, 0), cv_rows=_rows(c.m, 1))),
    ("conditional_densities", 0,
     lambda e, c: e.conditional_densities([np.linspace(-0.2, 0.2, 3 + i) for i in range(c.m)], GAMMAS, mu_rows=_rows(c.m, 0),
                                          cv_rows=_rows(c.m, 1))),
    ("il_payoffs_row", 0, lambda e, c: e.il_payoffs([1.0, 1.1], 1.0, 0.8, 1.25, 1000.0, snap_row=0, return_pieces=True)),
    ("tilted_cond", 16, lambda e, c: e.price_hawkesjd_chain_tilted_cond(_tilted(c), HAWKES, SPY, SEED, CALL_ID, GAMMAS, True)),
    ("tilted_cond_greeks", 16, lambda e, c: e.price_hawkesjd_chain_tilted_cond_greeks(_tilted(c), HAWKES, SPY, SEED, CALL_ID, GAMMAS, False)),
    ("jump_rows", 16, lambda e, c: e.step_hawkesjd_jump_rows(_tilted(c), HAWKES, SPY, SEED, CALL_ID)),
    ("jump_sets_payoffs", 0,
     lambda e, c: e.jump_sets_payoffs(c.forwards, c.strikes, c.codes, [[0.01 * (q + 1) * (i + 1) for i in range(c.m)] for q in range(G)],
                                      GAMMAS, True, a_rows=_rows(c.m, 0))),
    ("chain_cmc_many_logsv", -1, lambda e, c: e.chain_cmc_many("logsv", *grid(c), logsv_rows(c, J), SEEDS, IDS, 1, mu_row=2)),
    ("chain_cmc_many_heston", 5, lambda e, c: e.chain_cmc_many("heston", *grid(c), heston_rows(J), SEEDS, IDS)),
    ("conditional_sens_host_rows", 0,
     lambda e, c: e.conditional_sens(c.forwards, c.disc, c.strikes, c.codes, STEPS, True, host_rows=_sens_host_rows(c.m))),
    ("conditional_sens_rows", 0,
     lambda e, c: e.conditional_sens(c.forwards, c.disc, c.strikes, c.codes, STEPS, False, up_rows=_sens_rows(c.m, "up"),
                                     dn_rows=_sens_rows(c.m, "dn"))),
    ("greeks_payoffs_host_rows", 0,
     lambda e, c: e.greeks_payoffs(c.forwards, c.disc, c.strikes, c.codes, STEPS, host_rows=_greeks_host_rows(c.m))),
    ("greeks_payoffs_rows", 0,
     lambda e, c: e.greeks_payoffs(c.forwards, c.disc, c.strikes, c.codes, STEPS, base_rows=_rows(c.m, 0),
                                   up_rows=[_rows(c.m, 1 + 2 * p) for p in range(P)], dn_rows=[_rows(c.m, 2 + 2 * p) for p in range(P)])),
    ("il_payoffs_state", 0, lambda e, c: e.il_payoffs(1.05, 1.0, [0.8, 0.9], 1.25)),
]
ONE_EXPIRY = ROUTES[:13]                             # the nine fused routes (and Heston's second scheme) and the three many-job ones

# the lengths of the pointer arguments of every C entry point the routes reach, in argument order (">": an output, filled); names of
# the expressions: m expiries, K strikes, X density points, J jobs, P sets or steps, G gammas, W doubles per parameter row, N cases
_Q = "K K m+1"
LENGTHS = {
    "svmc_logsv_chain_price": f"m m m m {_Q} >K >K",
    "svmc_heston_chain_price": f"m m m {_Q} >K >K",
    "svmc_hawkesjd_chain_price": f"m m m {_Q} 16 >K >K",
    "svmc_logsv_chain_price_cmc": f"m m m m {_Q} >K >K >5*m",
    "svmc_heston_chain_price_cmc": f"m m m {_Q} >K >K >5*m",
    "svmc_hawkesjd_chain_price_cmc": f"m m m {_Q} 16 >K >K >5*m",
    "svmc_logsv_chain_price_cmc_greeks": f"m m m m {_Q} >10*K >6*m",
    "svmc_heston_chain_price_cmc_greeks": f"m m m {_Q} >10*K >6*m",
    "svmc_hawkesjd_chain_price_cmc_greeks": f"m m m {_Q} 16 >10*K >6*m",
    "svmc_hawkesjd_chain_price_tilted": f"m m {_Q} 16 G >G*K >G*K >G*m*8",
    "svmc_hawkesjd_chain_price_tilted_many": f"m m {_Q} J*16 J J J*G >J*G*K >J*G*K >J*G*m*8",
    "svmc_cmc_payoff_chain": f"m m {_Q} >K >K >5*m",
    "svmc_cmc_greeks_chain": f"m m {_Q} >10*K >6*m",
    "svmc_cmc_sens_chain": f"m m {_Q} P >P*3*K",
    "svmc_greeks_payoff_chain": f"m m {_Q} P >5*K >P*3*K",
    "svmc_il_payoff": "N*5 >N*10",
    "svmc_hawkesjd_chain_cond": "m m 16 >m",
    "svmc_tilted_cond_payoff_chain": f"m K {_Q} G >G*K >G*K >G*m*8",
    "svmc_tilted_cond_greeks_chain": f"m {_Q} G >G*8*K >G*m*4",
    "svmc_cond_density_chain": "X m+1 G >G*X >G*X >G*m*5",
    "svmc_jump_sets_payoff_chain": f"m K {_Q} G*m G >G*K >G*K >G*m*8 >m",
}
for _model in ("logsv", "heston", "hawkesjd"):
    LENGTHS[f"svmc_{_model}_chain_price_many"] = f"m m m {_Q} J*W J J >J*K >J*K"
for _model in ("logsv", "heston"):
    LENGTHS[f"svmc_{_model}_chain_price_cmc_many"] = f"m m m {_Q} J*W J J >J*K >J*K >J*m*5"
    LENGTHS[f"svmc_{_model}_chain_price_cmc_sens"] = f"m m m {_Q} (1+2*P)*W P >10*K >6*m >P*3*K"
    LENGTHS[f"svmc_{_model}_chain_price_cmc_sets"] = f"m m m {_Q} P*W >P*K >P*K >P*m*5 >P*K"        # the last one may be NULL
    LENGTHS[f"svmc_{_model}_chain_price_greeks"] = f"m m m {_Q} (1+2*P)*W P >K >K >5*K >P*3*K"
    LENGTHS[f"svmc_{_model}_chain_cmc_many"] = "m m J*W J J"


class RecordingLib:
    """libsvmc (and both side libraries) stand-in: every call succeeds, is recorded in a form that can be written down, and has its
    outputs filled"""

    def __init__(self, dims):
        self.calls, self.dims, self.keep, self.handles = [], dims, [], 0

    def _byref(self, obj):
        if isinstance(obj, C.c_size_t):
            obj.value = 4100                                   # not a multiple of 8: the size in doubles is rounded up
        elif isinstance(obj, C.c_void_p):
            self.handles += 1
            obj.value = 0xA000 + 0x100 * self.handles
        elif isinstance(obj, C.c_float):
            obj.value = 1.5
        else:
            obj.value = 1
        return "byref " + type(obj).__name__

    def __getattr__(self, name):
        def call(*args):
            lengths = iter(LENGTHS.get(name, "").split())
            rec, n_out = [name], 0
            for a in args:
                if isinstance(a, C._Pointer):
                    spec = next(lengths)
                    n = int(eval(spec.lstrip(">"), {}, self.dims))
                    if spec.startswith(">"):
                        n_out += 1
                        for i in range(n):
                            a[i] = 100.0 * n_out + 0.25 * i
                        rec.append({"out": n})
                    else:
                        rec.append({"at": [a[i] for i in range(n)]})
                elif isinstance(a, C.Array):
                    rec.append({"array": list(a)})
                elif type(a).__name__ == "CArgObject":
                    rec.append(self._byref(a._obj))
                elif isinstance(a, C._SimpleCData):
                    rec.append({type(a).__name__: a.value})
                elif a is None or type(a) in (int, float, bool, str):
                    rec.append(a)
                elif isinstance(a, (np.integer, np.floating)):
                    rec.append({type(a).__name__: a.item()})
                else:
                    raise TypeError(f"{name}: an argument of type {type(a).__name__}")
            if name == "svmc_memcpy_h2d":                      # (device, host address, bytes, stream): the host side by its contents
                rec[2] = {"sha256": hashlib.sha256(C.string_at(args[1], args[2])).hexdigest()}
            elif name == "svmc_memcpy_d2h":                    # (host, device, bytes, stream): filled
                host = args[0].value if hasattr(args[0], "value") else args[0]
                np.ctypeslib.as_array(C.cast(host, C.POINTER(C.c_double)), shape=(args[2] // 8,))[:] = 7.0 + 0.5 * np.arange(args[2] // 8)
                rec[1] = "host"
            elif name == "svmc_host_alloc":
                self.keep.append(np.zeros(args[1] // 8))
                args[0]._obj.value = self.keep[-1].ctypes.data
            self.calls.append(rec)
            return 0
        return call


def stub_engine(lib, timing):
    from stochvolmodels_amd import engine
    eng = engine.HipEngine.__new__(engine.HipEngine)
    buf = lambda base: types.SimpleNamespace(ptr=base, n=1 << 40, offset=lambda k: base + 8 * int(k))      # noqa: E731
    eng.lib, eng.n_path, eng.path_offset, eng.stream, eng.device, eng.closed = lib, N_PATH, 0, 9, 0, False
    eng.x, eng.vol, eng.qvar, eng._cv, eng.ws, eng.ws_bytes = buf(1 << 20), buf(2 << 20), buf(3 << 20), buf(4 << 20), buf(5 << 20), 4096
    eng._snap, eng._snap_rows = buf(1 << 32), 1 << 30
    eng._sums, eng._pinned, eng._pinned_doubles = {}, None, 0
    eng._prof = [] if timing else None
    eng._fused, eng._fused_size, eng._fused_graphs, eng._fused_timing = None, (0, 0), True, False
    tags = {}

    def alloc_sums(n, tag="sums"):
        base = tags.setdefault(tag, (1 << 40) + (len(tags) << 24))
        lib.calls.append(["alloc_sums", int(n), tag, base])
        return base, None
    eng.alloc_sums = alloc_sums
    eng.reserve_snapshots = lambda rows: lib.calls.append(["reserve_snapshots", int(rows)])
    return eng


def plain(obj):
    """a route's result as JSON can hold it: arrays as {"shape", "v"}, tuples as lists, slices as [start, stop]"""
    if isinstance(obj, np.ndarray):
        return {"shape": list(obj.shape), "v": obj.ravel().tolist()}
    if isinstance(obj, dict):
        return {str(k): plain(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [plain(v) for v in obj]
    if isinstance(obj, slice):
        return [obj.start, obj.stop]
    if isinstance(obj, (np.integer, np.floating)):
        return obj.item()
    return obj


def _dims(c, width):
    return dict(m=c.m, K=c.K, X=sum(3 + i for i in range(c.m)), J=J, P=P, G=G, W=6 + c.m if width < 0 else width, N=2)


class _SideLibraries:
    """while inside: _lib.load_ext() and _lib.load_est() hand out `lib`"""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        from stochvolmodels_amd import _lib
        self.saved = (_lib.load_ext, _lib.load_est)
        _lib.load_ext = _lib.load_est = lambda: self.lib

    def __exit__(self, *exc):
        from stochvolmodels_amd import _lib
        _lib.load_ext, _lib.load_est = self.saved


def host_route(route, c, width, timing):
    """{"calls", "result", "timed"} of one route on a fresh stand-in engine, or {"calls", "error": [type, text]}"""
    lib = RecordingLib(_dims(c, width))
    eng = stub_engine(lib, timing)
    with _SideLibraries(lib):
        try:
            out = {"result": plain(route(eng, c))}
        except Exception as e:                       # noqa: BLE001  (a refusal is a result)
            out = {"error": [type(e).__name__, str(e)]}
    out["calls"] = lib.calls
    if timing:
        out["timed"] = [p[0] for p in eng._prof]
    return out


def refusals():
    """(name, route(engine, chain)) of every request this layer refuses"""
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp, logsv_pricer as lp
    out = []
    for model in ("sabr", "hawkesjd"):
        out += [
            (f"many_fused_{model}", lambda e, c, M=model: e.price_chain_many_fused(_marshalled(c), M if M == "sabr" else "rough", heston_rows(J),
                                                                                   SEEDS, IDS, 1, SPY, 1)),
            (f"chain_cmc_many_{model}", lambda e, c, M=model: e.chain_cmc_many(M, *grid(c), heston_rows(J), SEEDS, IDS)),
            (f"cmc_many_fused_{model}", lambda e, c, M=model: e.price_chain_cmc_many_fused(_marshalled(c), M, heston_rows(J), SEEDS, IDS, 1,
                                                                                          SPY, True)),
            (f"cmc_sens_fused_{model}", lambda e, c, M=model: e.price_chain_cmc_sens_fused(_marshalled(c), M, sens_table(heston_rows(1)),
                                                                                          STEPS, 1, SPY, True, SEED, CALL_ID)),
            (f"cmc_sets_fused_{model}", lambda e, c, M=model: e.price_chain_cmc_sets_fused(_marshalled(c), M, heston_rows(P), 1, SPY, True,
                                                                                          SEED, CALL_ID)),
            (f"greeks_fused_{model}", lambda e, c, M=model: e.price_chain_greeks_fused(_marshalled(c), M, sens_table(heston_rows(1)), STEPS,
                                                                                      1, SPY, SEED, CALL_ID)),
        ]
    bad_etas = np.ones(4)
    out += [
        ("etas_logsv_fused", lambda e, c: e.price_logsv_chain_fused(_marshalled(c), *LOGSV, bad_etas, True, SPY, 1, SEED, CALL_ID)),
        ("etas_logsv_cmc_fused", lambda e, c: e.price_logsv_chain_cmc_fused(_marshalled(c), *LOGSV, bad_etas, True, SPY, True, SEED, CALL_ID)),
        ("etas_logsv_cmc_greeks_fused",
         lambda e, c: e.price_logsv_chain_cmc_greeks_fused(_marshalled(c), *LOGSV, bad_etas, True, SPY, True, SEED, CALL_ID)),
        ("etas_logsv_pricer", lambda e, c: lp.logsv_mc_chain_greeks_conditional(
            c.ttms, c.forwards, c.disc, c.strikes, c.types, *LOGSV, bad_etas, nb_path=N_PATH, nb_steps_per_year=SPY, seed=SEED,
            wrt=("theta",))),
        ("table_height_cmc_sens", lambda e, c: e.price_chain_cmc_sens_fused(_marshalled(c), "logsv", sens_table(logsv_rows(c, 1))[:-1],
                                                                            STEPS, 1, SPY, True, SEED, CALL_ID)),
        ("table_height_greeks", lambda e, c: e.price_chain_greeks_fused(_marshalled(c), "heston", sens_table(heston_rows(1))[:-1], STEPS,
                                                                        1, SPY, SEED, CALL_ID)),
        ("sets_width", lambda e, c: e.price_chain_cmc_sets_fused(_marshalled(c), "logsv", heston_rows(P), 1, SPY, True, SEED, CALL_ID)),
        ("seeds_many_fused", lambda e, c: e.price_chain_many_fused(_marshalled(c), "heston", heston_rows(J), SEEDS[:2], IDS, 1, SPY, 1)),
        ("ids_cmc_many_fused", lambda e, c: e.price_chain_cmc_many_fused(_marshalled(c), "heston", heston_rows(J), SEEDS, IDS[:2], 1, SPY,
                                                                        True)),
        ("seeds_chain_cmc_many", lambda e, c: e.chain_cmc_many("heston", *grid(c), heston_rows(J), SEEDS + [5], IDS)),
        ("seeds_tilted_many", lambda e, c: e.price_hawkesjd_chain_tilted_many_fused(_tilted(c), hawkes_rows(J), SPY, SEEDS[:2], IDS,
                                                                                    np.array([GAMMAS] * J), False)),
        ("gammas_tilted_many", lambda e, c: e.price_hawkesjd_chain_tilted_many_fused(_tilted(c), hawkes_rows(J), SPY, SEEDS, IDS,
                                                                                     np.array([GAMMAS] * 2), False)),
        ("spy_step_cond_rows", lambda e, c: e.step_hawkesjd_chain_cond_rows(_tilted(c), HAWKES, 0, SEED, CALL_ID)),
        ("spy_jump_rows", lambda e, c: e.step_hawkesjd_jump_rows(_tilted(c), HAWKES, -12, SEED, CALL_ID)),
        ("spy_jump_step_grid", lambda e, c: hp.jump_step_grid(c.ttms, 0)),
        ("spy_one_expiry_grid", lambda e, c: lp.one_expiry_grid(0.25, 0)),
        ("sens_host_rows_shape", lambda e, c: e.conditional_sens(c.forwards, c.disc, c.strikes, c.codes, STEPS, True,
                                                                 host_rows=_sens_host_rows(c.m)[:3] + ([[np.zeros(5)] * c.m] * P,))),
        ("greeks_host_rows_count", lambda e, c: e.greeks_payoffs(c.forwards, c.disc, c.strikes, c.codes, STEPS,
                                                                 host_rows=(_greeks_host_rows(c.m)[0][:-1],) + _greeks_host_rows(c.m)[1:])),
    ]
    return out


def record_host():
    """the whole host recording: {"three": {route: ...}, "one": {...}, "untimed": {...}, "refusals": {...}}"""
    three, one = chain(3), chain(1)
    rec = {"three": {n: host_route(r, three, w, True) for n, w, r in ROUTES},
           "one": {n: host_route(r, one, w, True) for n, w, r in ONE_EXPIRY},
           "untimed": {n: host_route(r, three, w, False) for n, w, r in ONE_EXPIRY},
           "refusals": {n: host_route(r, three, 5, False) for n, r in refusals()}}
    return json.loads(json.dumps(rec))               # as it reads back from the file


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------------
def leaves(obj, path=""):
    """(path, array) of every numeric leaf of a route's result"""
    if isinstance(obj, dict):
        for k, v in obj.items():
            yield from leaves(v, f"{path}/{k}")
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from leaves(v, f"{path}/{i}")
    elif isinstance(obj, slice):
        yield path, np.array([obj.start, obj.stop])
    elif obj is not None:
        yield path, np.asarray(obj)


def pricer_routes(c):
    """(name, call()) of the public pricer functions over the routes, on the chain c with strings for option types"""
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp, heston_pricer as he, logsv_pricer as lp
    kw = dict(ttms=c.ttms, forwards=c.forwards, discfactors=c.disc, strikes_ttms=c.strikes, optiontypes_ttms=c.types)
    mc = dict(nb_path=N_PATH, nb_steps_per_year=SPY)
    lg = dict(zip(("v0", "theta", "kappa1", "kappa2", "beta", "volvol"), LOGSV), vol_backbone_etas=c.etas)
    hs = dict(zip(("v0", "theta", "kappa", "rho", "volvol"), HESTON))
    hw = dict(zip(hp.PARAM_NAMES, HAWKES.tolist()))
    lps = [sv.LogSvParams(sigma0=0.8 + 0.01 * j, theta=1.0, kappa1=3.0, kappa2=3.0, beta=0.15, volvol=1.8) for j in range(J)]
    hps = [he.HestonParams(v0=0.04 + 0.001 * j, theta=0.05, kappa=3.0, rho=-0.5, volvol=0.4) for j in range(J)]
    wps = [hp.HawkesJDParams(sigma=0.45 + 0.01 * j) for j in range(J)]
    return [
        ("logsv_mc_chain_pricer", lambda: lp.logsv_mc_chain_pricer(**kw, **lg, **mc, seed=SEED)),
        ("logsv_mc_chain_pricer_conditional", lambda: lp.logsv_mc_chain_pricer_conditional(**kw, **lg, **mc, seed=SEED, return_stats=True)),
        ("logsv_mc_chain_greeks_conditional", lambda: lp.logsv_mc_chain_greeks_conditional(**kw, **lg, **mc, seed=SEED, return_stats=True)),
        ("logsv_mc_chain_greeks_conditional_wrt",
         lambda: lp.logsv_mc_chain_greeks_conditional(**kw, **lg, **mc, seed=SEED, wrt=("theta", "volvol"))),
        ("logsv_mc_chain_greeks", lambda: lp.logsv_mc_chain_greeks(lps[0], **kw, wrt=("theta", "volvol"), **mc, seed=SEED)),
        ("logsv_mc_chain_pricer_many", lambda: lp.logsv_mc_chain_pricer_many(lps, **kw, **mc, seeds=SEEDS)),
        ("logsv_mc_chain_pricer_conditional_many",
         lambda: lp.logsv_mc_chain_pricer_conditional_many(lps, **kw, **mc, seeds=SEEDS, return_stats=True)),
        ("logsv_mc_chain_pricer_conditional_sets",
         lambda: lp.logsv_mc_chain_pricer_conditional_sets(lps[:P], **kw, **mc, seed=SEED, return_ivols=True, return_stats=True)),
        ("heston_mc_chain_pricer", lambda: he.heston_mc_chain_pricer(**kw, **hs, **mc, seed=SEED)),
        ("heston_mc_chain_pricer_qe", lambda: he.heston_mc_chain_pricer(**kw, **hs, **mc, seed=SEED, scheme="qe")),
        ("heston_mc_chain_pricer_conditional", lambda: he.heston_mc_chain_pricer_conditional(**kw, **hs, **mc, seed=SEED, return_stats=True)),
        ("heston_mc_chain_greeks_conditional", lambda: he.heston_mc_chain_greeks_conditional(**kw, **hs, **mc, seed=SEED, return_stats=True)),
        ("heston_mc_chain_greeks_conditional_wrt",
         lambda: he.heston_mc_chain_greeks_conditional(**kw, **hs, **mc, seed=SEED, wrt=("theta", "volvol"))),
        ("heston_mc_chain_greeks", lambda: he.heston_mc_chain_greeks(hps[0], **kw, wrt=("theta", "volvol"), **mc, seed=SEED)),
        ("heston_mc_chain_pricer_many", lambda: he.heston_mc_chain_pricer_many(hps, **kw, **mc, seeds=SEEDS)),
        ("heston_mc_chain_pricer_conditional_many",
         lambda: he.heston_mc_chain_pricer_conditional_many(hps, **kw, **mc, seeds=SEEDS, return_stats=True)),
        ("heston_mc_chain_pricer_conditional_sets",
         lambda: he.heston_mc_chain_pricer_conditional_sets(hps[:P], **kw, **mc, seed=SEED, return_ivols=False, return_stats=True)),
        ("hawkesjd_mc_chain_pricer", lambda: hp.hawkesjd_mc_chain_pricer(**kw, **hw, **mc, seed=SEED)),
        ("hawkesjd_mc_chain_pricer_conditional", lambda: hp.hawkesjd_mc_chain_pricer_conditional(**kw, **hw, **mc, seed=SEED, return_stats=True)),
        ("hawkesjd_mc_chain_greeks_conditional", lambda: hp.hawkesjd_mc_chain_greeks_conditional(**kw, **hw, **mc, seed=SEED, return_stats=True)),
        ("hawkesjd_with_risk_premia_gammas", lambda: hp.hawkesjd_mc_chain_pricer_with_risk_premia_gammas(
            **kw, **hw, **mc, seed=SEED, risk_premia_gammas=GAMMAS, recenter_forward=True, return_forwards=True)),
        ("hawkesjd_with_risk_premia", lambda: hp.hawkesjd_mc_chain_pricer_with_risk_premia(
            **kw, **hw, **mc, seed=SEED, risk_premia_gamma=1.0, return_forwards=True)),
        ("hawkesjd_conditional_with_risk_premia_gammas", lambda: hp.hawkesjd_mc_chain_pricer_conditional_with_risk_premia_gammas(
            **kw, **hw, **mc, seed=SEED, risk_premia_gammas=GAMMAS, recenter_forward=True, return_forwards=True)),
        ("hawkesjd_conditional_with_risk_premia", lambda: hp.hawkesjd_mc_chain_pricer_conditional_with_risk_premia(
            **kw, **hw, **mc, seed=SEED, risk_premia_gamma=-0.5, return_forwards=True)),
        ("hawkesjd_greeks_conditional_with_risk_premia_gammas", lambda: hp.hawkesjd_mc_chain_greeks_conditional_with_risk_premia_gammas(
            **kw, **hw, **mc, seed=SEED, risk_premia_gammas=GAMMAS, return_stats=True)),
        ("hawkesjd_greeks_conditional_with_risk_premia", lambda: hp.hawkesjd_mc_chain_greeks_conditional_with_risk_premia(
            **kw, **hw, **mc, seed=SEED, risk_premia_gamma=1.0, recenter_forward=True, return_stats=True)),
        ("hawkesjd_mc_chain_pricer_many", lambda: hp.hawkesjd_mc_chain_pricer_many(wps, **kw, **mc, seeds=SEEDS)),
        ("hawkesjd_with_risk_premia_gammas_many", lambda: hp.hawkesjd_mc_chain_pricer_with_risk_premia_gammas_many(
            wps, **kw, **mc, seeds=SEEDS, risk_premia_gammas=GAMMAS, return_forwards=True)),
        ("hawkesjd_conditional_sets", lambda: hp.hawkesjd_mc_chain_pricer_conditional_sets(
            [0.3, 0.45], GAMMAS, **kw, **{k: v for k, v in hw.items() if k != "sigma"}, **mc, seed=SEED, return_forwards=True)),
    ]


def empty_expiry_chain():
    c = chain(3)
    c.strikes[1], c.codes[1], c.types[1] = np.zeros(0), np.zeros(0, dtype=np.int8), np.array([], dtype="<U1")
    c.K = sum(k.size for k in c.strikes)
    return c


def run_gpu():
    """({route + path: array}, {route: sorted kernel names | [exception type, text]}) of every route on one engine of N_PATH paths"""
    from stochvolmodels_amd.engine import get_engine
    eng = get_engine(N_PATH)
    arrays, notes = {}, {}

    def run(name, call):
        eng.start_kernel_timing()
        try:
            out = call()
        except Exception as e:                       # noqa: BLE001  (recorded: the branch is held to what the parent does)
            eng.stop_kernel_timing()
            notes[name] = [type(e).__name__, str(e)]
            return
        notes[name] = sorted(eng.stop_kernel_timing())
        for path, a in leaves(out):
            arrays[name + path] = a
    three, one, empty = chain(3), chain(1), empty_expiry_chain()
    for name, _, route in ROUTES:
        run("engine/" + name, lambda: route(eng, three))
    for name, _, route in ONE_EXPIRY:
        run("engine1/" + name, lambda: route(eng, one))
    for name, call in pricer_routes(three):
        run("pricer/" + name, call)
    run("empty/logsv_fused", lambda: ROUTES[0][2](eng, empty))
    run("empty/hawkesjd_cmc_fused", lambda: ROUTES[6][2](eng, empty))
    return arrays, notes
