"""
Host side of the Monte Carlo chain Greeks (include/svmc.h): what is refused before any device work, the
bump sizes, the job table of the one stepping launch, and the shaping of the results.  No library call is made here.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import dist as svdist
from .engine import GREEKS_BASE_FIELDS, GREEKS_MAX_PARAMS, GREEKS_SENS_FIELDS, tilted_type_codes
from .mc_chain import chain_shaped, variable_type_code

LOGSV_GREEK_PARAMS = ("sigma0", "theta", "kappa1", "kappa2", "beta", "volvol")      # the columns of a LogSV job row, in order
HESTON_GREEK_PARAMS = ("v0", "theta", "kappa", "rho", "volvol")                     # ... of a Heston job row
# where a bumped value must stay: a volatility, a variance or a vol-of-vol is not negative, a correlation lies inside (-1, 1)
_NON_NEGATIVE = {"logsv": ("sigma0", "theta", "volvol"), "heston": ("v0", "theta", "volvol")}


def check_greeks_request(who: str, variable_type, comm, devices, optiontypes_ttms, is_spot_measure: bool = True) -> list:
    """the requests the Greeks calls refuse, before any device work: 'IC' / 'IP' (ValueError("not implemented")), another
    variable than LOG_RETURN, the inverse measure, sharded paths.  Returns the per-expiry type codes."""
    codes = [tilted_type_codes(t) for t in optiontypes_ttms]                # ValueError("not implemented")
    if variable_type_code(variable_type) != 1:
        raise NotImplementedError(f"{who}: variable_type={variable_type}: the Greeks are those of options on the log-return")
    if not is_spot_measure:
        raise NotImplementedError(f"{who}: is_spot_measure=False: the Greeks cover the spot measure")
    if devices is not None or (comm or svdist.get_default_comm()).world > 1:
        raise NotImplementedError(f"{who}: sharded paths (comm.world > 1, devices=) are not covered")
    return codes


def greeks_bumps(model: str, values: Dict[str, float], wrt: Optional[Sequence[str]] = None, rel_bump: float = 1e-3,
                 bumps: Optional[Dict[str, float]] = None) -> Tuple[Tuple[str, ...], np.ndarray]:
    """(names, h) of the requested sensitivities: wrt defaults to every parameter of the model, h_p = rel_bump |theta_p| unless
    bumps[name] gives it.  ValueError, naming the parameter: an unknown or repeated name, a bump that is not positive and finite,
    a zero parameter without an explicit bump, a bump that takes theta_p +- h_p out of the parameter's domain.  Nothing is made
    one-sided."""
    all_names = {"logsv": LOGSV_GREEK_PARAMS, "heston": HESTON_GREEK_PARAMS}[model]
    names = tuple(all_names if wrt is None else ((wrt,) if isinstance(wrt, str) else wrt))
    bumps = dict(bumps or {})
    for name in list(names) + list(bumps):
        if name not in all_names:
            raise ValueError(f"{name!r} is not a parameter of the {model} model: {', '.join(all_names)}")
    if len(set(names)) != len(names):
        raise ValueError(f"a parameter is named twice in wrt={names}")
    if len(names) > GREEKS_MAX_PARAMS:
        raise ValueError(f"at most {GREEKS_MAX_PARAMS} sensitivities per call")
    if not (np.isfinite(rel_bump) and rel_bump > 0.0):
        raise ValueError("rel_bump must be positive and finite")
    h = np.empty(len(names))
    for j, name in enumerate(names):
        v = float(values[name])
        if name in bumps:
            h[j] = float(bumps[name])
            if not (np.isfinite(h[j]) and h[j] > 0.0):
                raise ValueError(f"the bump of {name} must be positive and finite, got {bumps[name]!r}")
        elif v == 0.0:
            raise ValueError(f"{name} is zero: a relative bump has no size there; give bumps={{{name!r}: h}}")
        else:
            h[j] = float(rel_bump) * abs(v)
        if name in _NON_NEGATIVE[model] and v - h[j] < 0.0:
            raise ValueError(f"the bump {h[j]:g} of {name} = {v:g} leaves its domain: {name} - h < 0")
        if name == "rho" and not (-1.0 < v - h[j] and v + h[j] < 1.0):
            raise ValueError(f"the bump {h[j]:g} of rho = {v:g} leaves its domain: |rho +- h| >= 1")
    return names, h


def greeks_job_table(model: str, base_row: np.ndarray, names: Sequence[str], h: np.ndarray) -> np.ndarray:
    """the [1 + 2P][len(base_row)] parameter rows of the one stepping launch: the base row untouched, then per requested
    parameter the row at theta_p + h_p (up) and the row at theta_p - h_p (dn).  All rows share one seed and one call id."""
    all_names = {"logsv": LOGSV_GREEK_PARAMS, "heston": HESTON_GREEK_PARAMS}[model]
    base_row = np.asarray(base_row, dtype=np.float64).ravel()
    rows = np.tile(base_row, (1 + 2 * len(names), 1))
    for j, name in enumerate(names):
        col = all_names.index(name)
        rows[1 + 2 * j, col] = base_row[col] + h[j]
        rows[2 + 2 * j, col] = base_row[col] - h[j]
    return rows


def greeks_shaped(prices, stderrs, base: np.ndarray, sens: np.ndarray, names: Sequence[str], slices, strikes_ttms) -> dict:
    """the flat results of a call -- prices / stderrs per expiry, base [5][K], sens [P][3][K] -- as the dict of chain-shaped lists
    the pricers return: price, stderr, delta, delta_stderr, dual_delta, dual_delta_stderr, n_itm, and per name sens, sens_stderr,
    n_pairs (the counts as integer arrays)"""
    cut = lambda row: chain_shaped([row[sl] for sl in slices], strikes_ttms)         # noqa: E731
    as_int = lambda parts: [p.astype(np.int64) for p in parts]                       # noqa: E731
    out = {"price": chain_shaped(prices, strikes_ttms), "stderr": chain_shaped(stderrs, strikes_ttms)}
    for r, field in enumerate(GREEKS_BASE_FIELDS):
        out[field] = as_int(cut(base[r])) if field == "n_itm" else cut(base[r])
    out["sens"] = {name: cut(sens[j, 0]) for j, name in enumerate(names)}
    out["sens_stderr"] = {name: cut(sens[j, 1]) for j, name in enumerate(names)}
    out["n_pairs"] = {name: as_int(cut(sens[j, 2])) for j, name in enumerate(names)}
    return out
