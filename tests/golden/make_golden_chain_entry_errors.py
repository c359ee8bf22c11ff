"""
Record tests/golden/chain_entry_errors.json: the status code and svmc_last_error text with which each of the eight on-device-RNG
chain entry points of svmc_chain.hip -- svmc_{logsv,heston,hawkesjd}_chain_price, svmc_hawkesjd_chain_price_tilted and their four
_many siblings -- refuses a bad argument, one defect at a time and two at once (which of two failing checks answers pins the
ORDER of the checks).  This project's own output, recorded on a GPU box:

    python tests/golden/make_golden_chain_entry_errors.py          # writes the fixture

Recorded on commit eee3073 ("Price many independent Hawkes MC chains in one stepping launch"), the parent of the change that
gave the entry points their shared host helpers; tests/test_gpu_chain_entry_errors.py replays the table on every later build.

Every case fails in the host-side checks, before anything is launched: a session of 64 paths, 2 expiries and 6 strikes is
created (that needs the device) and no kernel ever runs on it.  A defect is listed for an entry point only where that entry
point checks it; a case that came back SVMC_OK would have launched, so run() refuses to record one.
"""
from __future__ import annotations

import ctypes as C
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(HERE, "chain_entry_errors.json")

N_PATH, M, K = 64, 2, 6
MAX_M, MAX_JOBS, MAX_GAMMAS = 17, 65, 17          # one past the library's limits: every array is long enough for a bad count
LOG_RETURN, Q_VAR = 1, 2

# the arguments of each entry point, in the order of include/svmc.h
CHAIN = ("session", "ttms", "forwards", "discfactors")
QUOTES = ("n_expiries", "strikes", "types", "offsets")
SIGNATURES = {
    "svmc_logsv_chain_price": CHAIN + ("etas",) + QUOTES + ("v0", "theta", "kappa1", "kappa2", "beta", "volvol", "is_spot_measure",
                                                            "nb_steps_per_year", "variable_type", "seed", "call_id", "prices", "stderrs"),
    "svmc_heston_chain_price": CHAIN + QUOTES + ("v0", "theta", "kappa", "rho", "volvol", "scheme", "nb_steps_per_year",
                                                 "variable_type", "seed", "call_id", "prices", "stderrs"),
    "svmc_hawkesjd_chain_price": CHAIN + QUOTES + ("params", "nb_steps_per_year", "variable_type", "seed", "call_id", "prices",
                                                   "stderrs"),
    "svmc_hawkesjd_chain_price_tilted": CHAIN[:3] + QUOTES + ("params", "nb_steps_per_year", "seed", "call_id", "gammas", "n_gammas",
                                                              "recenter", "prices", "stderrs", "stats"),
    "svmc_logsv_chain_price_many": CHAIN + QUOTES + ("n_jobs", "params", "seeds", "call_ids", "is_spot_measure", "nb_steps_per_year",
                                                     "variable_type", "prices", "stderrs"),
    "svmc_heston_chain_price_many": CHAIN + QUOTES + ("n_jobs", "params", "seeds", "call_ids", "scheme", "nb_steps_per_year",
                                                      "variable_type", "prices", "stderrs"),
    "svmc_hawkesjd_chain_price_many": CHAIN + QUOTES + ("n_jobs", "params", "seeds", "call_ids", "nb_steps_per_year", "variable_type",
                                                        "prices", "stderrs"),
    "svmc_hawkesjd_chain_price_tilted_many": CHAIN[:3] + QUOTES + ("n_jobs", "params", "seeds", "call_ids", "nb_steps_per_year",
                                                                   "gammas", "n_gammas", "recenter", "prices", "stderrs", "stats"),
}
HAWKES = tuple(n for n in SIGNATURES if "hawkesjd" in n)
TILTED = tuple(n for n in SIGNATURES if "tilted" in n)
MANY = tuple(n for n in SIGNATURES if n.endswith("_many"))
SINGLE = tuple(n for n in SIGNATURES if n not in MANY)
EVERY = tuple(SIGNATURES)


def base_arguments(entry: str, session) -> dict:
    """a good call of `entry` (it is never made): fresh arrays, so that a defect may write into them"""
    from stochvolmodels_amd.pricers.hawkes_jd_pricer import HawkesJDParams, _model_block
    n_jobs = 2
    a = dict(session=session, ttms=0.1 * np.arange(1, MAX_M + 1), forwards=np.linspace(1.0, 1.1, MAX_M), discfactors=np.ones(MAX_M),
             etas=np.ones(MAX_M), n_expiries=M, strikes=np.linspace(0.8, 1.2, K + 1), types=np.array([1, 0, 0, 1, 1, 0, 0], dtype=np.int8),
             offsets=np.array([0, 3] + [K] * (MAX_M - 1), dtype=np.uintp), v0=0.8, theta=1.0, kappa1=3.0, kappa2=3.0, beta=0.15,
             volvol=1.8, kappa=3.0, rho=-0.5, is_spot_measure=1, scheme=0, nb_steps_per_year=120, variable_type=LOG_RETURN, seed=7,
             call_id=0, n_jobs=n_jobs, seeds=np.arange(1, MAX_JOBS + 1, dtype=np.uint64), call_ids=np.zeros(MAX_JOBS, dtype=np.uint32),
             gammas=np.zeros(MAX_JOBS * MAX_GAMMAS), n_gammas=2, recenter=0, prices=np.zeros(MAX_JOBS * MAX_GAMMAS * (K + 1)),
             stderrs=np.zeros(MAX_JOBS * MAX_GAMMAS * (K + 1)), stats=np.zeros(MAX_JOBS * MAX_GAMMAS * MAX_M * 8))
    if entry in HAWKES:
        a["params"] = np.tile(_model_block(HawkesJDParams()), (MAX_JOBS, 1))
    elif "logsv" in entry:
        a["params"] = np.tile(np.array([0.8, 1.0, 3.0, 3.0, 0.15, 1.8] + [1.0] * MAX_M), (MAX_JOBS, 1))
    else:
        a["params"] = np.tile(np.array([0.04, 0.04, 3.0, -0.5, 0.4]), (MAX_JOBS, 1))
    return a


def _null(key):
    return lambda a: a.__setitem__(key, None)


def _set(key, value):
    return lambda a: a.__setitem__(key, value)


def _put(key, index, value):
    return lambda a: a[key] is not None and a[key].__setitem__(index, value)     # (a pair may have nulled the array)


# (name, the entry points that check it, what it does to the arguments); "sharded" swaps in the session with a reducer attached
DEFECTS = [
    ("null_session", EVERY, _null("session")),
    ("null_ttms", EVERY, _null("ttms")),
    ("null_prices", EVERY, _null("prices")),
    ("null_stderrs", EVERY, _null("stderrs")),
    ("null_params", HAWKES + MANY, _null("params")),
    ("null_seeds", MANY, _null("seeds")),
    ("null_call_ids", MANY, _null("call_ids")),
    ("null_stats", TILTED, _null("stats")),
    ("null_gammas", TILTED, _null("gammas")),
    ("n_expiries_0", EVERY, _set("n_expiries", 0)),
    ("n_expiries_3", EVERY, _set("n_expiries", 3)),                     # above the session's 2, within the launch's 16
    ("n_expiries_17", EVERY, _set("n_expiries", 17)),
    ("n_jobs_0", MANY, _set("n_jobs", 0)),
    ("n_jobs_65", MANY, _set("n_jobs", 65)),
    ("nb_steps_per_year_0", EVERY, _set("nb_steps_per_year", 0)),
    ("call_id_2_24", SINGLE, _set("call_id", 1 << 24)),
    ("call_ids_2_24", MANY, _put("call_ids", 1, 1 << 24)),
    ("q_var", tuple(n for n in HAWKES if n not in TILTED), _set("variable_type", Q_VAR)),
    ("sigma_variable", tuple(n for n in EVERY if n not in TILTED), _set("variable_type", 3)),
    ("unknown_variable", tuple(n for n in EVERY if n not in TILTED), _set("variable_type", 9)),
    ("unknown_scheme", tuple(n for n in EVERY if "heston" in n), _set("scheme", 5)),
    ("nonfinite_param", HAWKES, _put("params", (0, 0), np.nan)),
    ("nonfinite_gamma", TILTED, _put("gammas", 1, np.inf)),
    ("nonfinite_forward", TILTED, _put("forwards", 1, np.nan)),
    ("nonfinite_strike", TILTED, _put("strikes", 4, np.inf)),
    ("decreasing_offsets", TILTED, _put("offsets", slice(0, 3), (0, 4, 3))),
    ("decreasing_ttms", EVERY, _put("ttms", 1, 0.05)),
    ("payoff_code_7", EVERY, _put("types", 2, 7)),
    ("inverse_payoff", TILTED, _put("types", 2, 2)),                     # a code the plain calls take and the tilted ones refuse
    ("n_gammas_0", TILTED, _set("n_gammas", 0)),
    ("n_gammas_17", TILTED, _set("n_gammas", 17)),
    ("strikes_exceed_session", EVERY, _put("offsets", slice(2, None), K + 1)),
    ("sharded", TILTED + MANY, "sharded"),
]


def cases():
    """(entry point, case name, [defects]) of the whole table: every applicable defect alone, then every pair of them"""
    for entry in SIGNATURES:
        own = [d for d in DEFECTS if entry in d[1]]
        for d in own:
            yield entry, d[0], [d]
        for d1, d2 in itertools.combinations(own, 2):
            yield entry, d1[0] + "+" + d2[0], [d1, d2]


def _pointer(v):
    return None if v is None else v.ctypes.data_as(C.c_void_p)


def call(L, entry: str, defects, session, sharded_session):
    """(status, message) of `entry` called with the defects applied to a good call's arguments"""
    a = base_arguments(entry, session)
    for _, _, change in defects:
        if change == "sharded":
            if a["session"] is not None:
                a["session"] = sharded_session
        else:
            change(a)
    fn = getattr(L, entry)
    assert len(fn.argtypes) == len(SIGNATURES[entry]), entry
    args = []
    for key, ctype in zip(SIGNATURES[entry], fn.argtypes):
        v = a[key]
        args.append(C.cast(_pointer(v), ctype) if isinstance(v, np.ndarray) else v)
    rc = fn(*args)
    return int(rc), L.svmc_last_error().decode("utf-8", "replace")


def run():
    """the table [[entry point, case, status, message]], from the library the package loads"""
    from stochvolmodels_amd import _lib
    L = _lib.load()
    plain, sharded = C.c_void_p(), C.c_void_p()
    _lib.check(L.svmc_session_create(C.byref(plain), N_PATH, M, K))
    _lib.check(L.svmc_session_create(C.byref(sharded), N_PATH, M, K))
    reducer = _lib.ALL_REDUCE_FN(lambda user, buf, n, stream: 0)          # never called: every case fails before the first launch
    _lib.check(L.svmc_session_set_reducer(sharded, reducer, None, 0, 2, 2 * N_PATH, 0))
    try:
        table = []
        for entry, name, defects in cases():
            rc, message = call(L, entry, defects, plain, sharded)
            if rc == 0:
                raise RuntimeError(f"{entry} / {name} was accepted: the case would launch, so it does not belong in this table")
            table.append([entry, name, rc, message])
        return table
    finally:
        _lib.check(L.svmc_session_destroy(plain))
        _lib.check(L.svmc_session_destroy(sharded))


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    rows = run()
    with open(out, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} cases -> {out}")
