"""
CPU twin of the Monte Carlo chain Greeks (include/svmc.h): the estimators restated in numpy.longdouble on host
arrays, the keep rule and the in-the-money indicator decided in DOUBLE as the device decides them, and Black-76's closed forms.
Not imported by the product.

Per expiry with forward F and discount factor DF, job j with terminal log-returns x and spot sums [sum F exp(x), count] over the
paths where F exp(x) is not NaN:
    M = (sum / count) / F, the double those two divisions give;   e = (exp(x) - M) + 1;   spot = F e;   s = +1 call, -1 put
    price      = DF mean(s (spot - K) 1{s (spot - K) > 0})                     (the plain estimator, homogeneous form)
    delta      = DF mean(g),  g = s e 1{s (spot - K) > 0};  error DF popdev(g) / sqrt(n)
    dual_delta = -s DF n_itm / n;  error DF sqrt(q (1 - q) / n), q = n_itm / n
    sens_p     = DF mean_pairs(d) / (2 h_p),  d = pay(x_up) - pay(x_dn), a pair kept iff neither spot is NaN;
                 error DF popdev_pairs(dt) / sqrt(n) / (2 h_p),  dt = d - s (q_up (spot_up - F) - q_dn (spot_dn - F)),
                 q_up, q_dn = n_itm / n of the up and of the dn job
The base job's means run over ALL n paths (a NaN spot is out of the money).  dt carries the delta-method term of the two
recentring means: M_up and M_dn are sample means, a payoff moves by -s F 1{in the money} per unit of its M, and popdev(d) alone
misses that coupling (in the money it overstates the error of the difference several times over).
"""
import numpy as np
from scipy.special import ndtr

L_ = np.longdouble


def spot_sums(x, forward):
    """[sum F exp(x), count] over the paths where F exp(x) is not NaN, in double (the device forms them in its own order)"""
    with np.errstate(all="ignore"):
        sp = forward * np.exp(np.asarray(x, dtype=np.float64))
    ok = ~np.isnan(sp)
    return np.array([sp[ok].sum(), float(ok.sum())])


def _job(x, forward, sums):
    """(spot in double, e in long double) of a job recentred by the mean its spot sums give"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        m64 = (sums[0] / sums[1]) / forward
        spot64 = forward * ((np.exp(x) - m64) + 1.0)
        e = (np.exp(x.astype(L_)) - L_(m64)) + L_(1)         # M is the double the two divisions give: an input of the estimator
    return spot64, e


def _popdev(v, mean):
    return np.sqrt(np.mean((v - mean) ** 2)) if v.size else L_(np.nan)


def greeks(x, forward, discfactor, strikes, types, x_up=(), x_dn=(), steps=(), sums=None):
    """the estimators above for one expiry; sums: [1 + 2P][2], the jobs' spot sums as the device holds them (None: formed here).
    Returns a dict of long-double arrays [K] (counts as int arrays): price, stderr, delta, delta_stderr, dual_delta,
    dual_delta_stderr, n_itm, and lists over the P parameters of sens, sens_stderr, n_pairs."""
    P = len(steps)
    jobs = [x] + [r for p in range(P) for r in (x_up[p], x_dn[p])]
    if sums is None:
        sums = [spot_sums(r, forward) for r in jobs]
    n = np.asarray(x).size
    F, DF = L_(forward), L_(discfactor)
    K = np.asarray(strikes, dtype=np.float64).ravel()
    s = np.where(np.asarray(types).ravel() == "C", 1.0, -1.0)
    out = {k: [] for k in ("price", "stderr", "delta", "delta_stderr", "dual_delta", "dual_delta_stderr", "n_itm")}
    out.update(sens=[[] for _ in range(P)], sens_stderr=[[] for _ in range(P)], n_pairs=[[] for _ in range(P)])
    with np.errstate(all="ignore"):
        spot64, e = _job(x, forward, sums[0])
        pairs = []
        for p in range(P):
            su64, eu = _job(x_up[p], forward, sums[1 + 2 * p])
            sd64, ed = _job(x_dn[p], forward, sums[2 + 2 * p])
            pairs.append((~np.isnan(su64) & ~np.isnan(sd64), F * eu, F * ed, su64, sd64))
        for k, sk in zip(K, s):
            itm = sk * (spot64 - k) > 0.0                     # decided in double; strict: a tie is out of the money
            g = np.where(itm, L_(sk) * e, L_(0))
            pay = np.where(itm, L_(sk) * (F * e - L_(k)), L_(0))
            gm = g.mean()
            q = L_(int(itm.sum())) / L_(n)
            out["price"].append(DF * pay.mean())
            out["stderr"].append(DF * _popdev(pay, pay.mean()) / np.sqrt(L_(n)))
            out["delta"].append(DF * gm)
            out["delta_stderr"].append(DF * _popdev(g, gm) / np.sqrt(L_(n)))
            out["dual_delta"].append(-L_(sk) * DF * q)
            out["dual_delta_stderr"].append(DF * np.sqrt(q * (1 - q) / L_(n)))
            out["n_itm"].append(int(itm.sum()))
            for p, (keep, su, sd, su64, sd64) in enumerate(pairs):
                # the coefficients' q are the doubles the device stores: in-the-money counts decided in double, over n
                qu = float(int((sk * (su64 - k) > 0.0).sum())) / float(n)
                qd = float(int((sk * (sd64 - k) > 0.0).sum())) / float(n)
                d = (np.maximum(L_(sk) * (su - L_(k)), L_(0)) - np.maximum(L_(sk) * (sd - L_(k)), L_(0)))[keep]
                dt = d - (L_(sk * qu) * (su - F) - L_(sk * qd) * (sd - F))[keep]
                dm = d.mean() if d.size else L_(np.nan)
                two_h = L_(2) * L_(steps[p])
                out["sens"][p].append(DF * dm / two_h)
                out["sens_stderr"][p].append(DF * _popdev(dt, dt.mean() if dt.size else L_(np.nan)) / np.sqrt(L_(n)) / two_h)
                out["n_pairs"][p].append(int(keep.sum()))
    for key in ("price", "stderr", "delta", "delta_stderr", "dual_delta", "dual_delta_stderr"):
        out[key] = np.array(out[key], dtype=L_)
    out["n_itm"] = np.array(out["n_itm"], dtype=np.int64)
    for key in ("sens", "sens_stderr"):
        out[key] = [np.array(v, dtype=L_) for v in out[key]]
    out["n_pairs"] = [np.array(v, dtype=np.int64) for v in out["n_pairs"]]
    return out


def black76(forward, strikes, ttm, vol, discfactor, types):
    """Black-76 per strike: (price, forward delta, dual delta, vega)"""
    K = np.asarray(strikes, dtype=np.float64)
    s = np.where(np.asarray(types) == "C", 1.0, -1.0)
    sd = vol * np.sqrt(ttm)
    d1 = np.log(forward / K) / sd + 0.5 * sd
    d2 = d1 - sd
    price = discfactor * s * (forward * ndtr(s * d1) - K * ndtr(s * d2))
    delta = discfactor * s * ndtr(s * d1)
    dual = -discfactor * s * ndtr(s * d2)
    vega = discfactor * forward * np.exp(-0.5 * d1 * d1) / np.sqrt(2.0 * np.pi) * np.sqrt(ttm)
    return price, delta, dual, vega


def gaussian_rows(z, ttm, vol):
    """terminal log-returns of a constant-volatility model on the normals z: x = -vol^2 T / 2 + vol sqrt(T) z"""
    return -0.5 * vol * vol * ttm + vol * np.sqrt(ttm) * z
