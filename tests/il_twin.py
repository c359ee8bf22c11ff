"""
The Monte Carlo impermanent-loss estimator of include/svmc.h (svmc_il_payoff) in NumPy long double: what
tests/test_gpu_il_mc.py holds the device to and what tests/golden/make_golden_il_payoff.py records from the CPU twin's paths.
The keep rule and the indicators are decided in double, as the device decides them.  Not a test module.
"""
import numpy as np

L_ = np.longdouble
FIELDS = ("value", "stderr", "square_root", "linear", "put", "call", "digital_put", "digital_call")


def host_spots(x, p1):
    """(keep mask, the recentred spots of the kept paths in double): the decisions' inputs"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(x)
        keep = np.isfinite(x) & np.isfinite(e)
        m = e[keep].sum() / max(int(keep.sum()), 1)
        return keep, p1 * e[keep] - (p1 * m - p1)


def brute(x, p1, p0, pa, pb, notional=1e6):
    """-> ({field: long double}, n_kept, n_dropped) of one case"""
    keep, s64 = host_spots(x, p1)
    n = int(keep.sum())
    below, above = s64 < pa, s64 > pb
    with np.errstate(all="ignore"):
        e = np.exp(np.asarray(x, dtype=np.float64)[keep].astype(L_))
        p1, p0, pa, pb, notional = (L_(v) for v in (p1, p0, pa, pb, notional))
        m = e.sum() / L_(max(n, 1))
        spot = p1 * e - (p1 * m - p1)
        inside = ~(below | above)
        pieces = dict(square_root=np.where(inside, np.sqrt(np.where(inside, spot, L_(1))), L_(0)),
                      linear=np.sqrt(p0) * (spot / p0 + 1),
                      put=np.where(below, pa - spot, L_(0)), call=np.where(above, spot - pb, L_(0)),
                      digital_put=below.astype(L_), digital_call=above.astype(L_))
        pay = (-2 * pieces["square_root"] + pieces["linear"] + pieces["put"] / np.sqrt(pa) - pieces["call"] / np.sqrt(pb)
               - 2 * np.sqrt(pa) * pieces["digital_put"] - 2 * np.sqrt(pb) * pieces["digital_call"])
        scale = notional / (2 * np.sqrt(p0) - p0 / np.sqrt(pb) - np.sqrt(pa))
        if n == 0:
            out = {k: L_(np.nan) for k in FIELDS}
        else:
            mean = pay.sum() / n
            var = ((pay - mean) ** 2).sum() / n
            out = dict(value=-scale * mean, stderr=scale * np.sqrt(var / n))
            out.update({k: v.sum() / n for k, v in pieces.items()})
    return out, n, int(np.size(x)) - n


def nearest_boundary(x, p1, pa, pb):
    """the smallest relative distance of a host spot from pa or pb: a one-ulp difference in exp must not flip an indicator"""
    _, s = host_spots(x, p1)
    if s.size == 0:
        return np.inf
    return float(min(np.min(np.abs(s - pa)) / pa, np.min(np.abs(s - pb)) / pb))
