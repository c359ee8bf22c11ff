"""
Generate tests/golden/mc_steps.npz: the terminal states of the Monte Carlo step recursions in extended precision, the truth that
tests/test_mc_steps_host.py holds the fp64 CPU oracles to and tests/test_gpu_mc_steps.py the stepping kernels.  CPU only, by hand:

    python tests/golden/make_golden_mc_steps.py

Everything is evaluated in mpmath at PREC = 256 bits from the double parameters, start states and random inputs (converted
exactly).  What is evaluated is the REFERENCE's recursion as the reference writes it -- not the kernels' regrouping (accumulator
form, Newton reciprocal, log-volatility in units of ln 2 / 256, split exponential):

    LogSV          pricers/logsv_pricer.py:1032-1045 (L = ln sigma0 once, then x, L, sigma = exp(L), qvar per step)
    Heston Euler   pricers/heston_pricer.py:368-379  (floor max(v, 1e-4))
    Heston QE      Andersen's QE-M as DESIGN.md and the header of oracle/svmc_oracle.c state it (psi_c = 1.5, gamma1 = gamma2 = 1/2,
                   the martingale correction K0* where it exists and the plain K0 where it does not)
    rough LogSV    pricers/rough_logsv/split_simulation.py:86-128, :228-246, :249-278, :281-352 (RK4 half drift, exact lognormal step
                   of the weighted sum, RK4 half drift, the `volw_h > 0` guard, log-spot and quadratic variance)
    Hawkes         pricers/hawkes_jd_pricer.py:715-776 (U = -ln u / dt, J = shift +- mean E, E = -ln u')

The random inputs are the product's own stream (version RNG_STREAM_VERSION, recorded): the oracle's fill_normals on streams 0
(LogSV, Heston Euler), 4 (QE) and 3 (rough), and hawkes_twin.stream_words for streams 5 (the QE uniform (r + 1/2) 2^-32), 6 and 7
(Hawkes).  A kernel that draws on the device sees these bits (tests/test_gpu_parity.py::test_normals_match_oracle_stream,
tests/test_gpu_device_math.py::test_normal_icdf32_is_the_twin_bit_for_bit); a supplied-randoms kernel gets the arrays uploaded.

A case is (generator, parameter set, step count, step_offset); the forms of a generator (supplied randoms, few-waves device draw,
full-launch device draw) share its truth.  Step counts 1, 2, 3, 7, 64 at step_offset 0 and 1 on N = 130 paths (two waves and two
lanes), and one 1024-step case on 64 paths per generator; rough LogSV 1, 2, 5, 40; Hawkes 1, 2, 3, 7, 64, 451.

File layout (flat, to keep the archive's member count small):
    meta          JSON: rng_stream_version, prec, and `cases`: per case id, gen, set, params, n, steps, dt, offset, seed, start,
                  nq (number of quantities: x, volatility-like state(s), qvar), scales [nq] (the error measure's floor under
                  |truth|), off (offset of the case's nq x n block in hi / lo_rel), foff (offset of its n flags in `fragile`),
                  checksum (sha256 of the case's random inputs as the oracle / twin returns them), oracle_err [nq] and, where a
                  NumPy restatement exists, numpy_err [nq]
    hi, lo_rel    the truth as the double pair hi + lo: hi the nearest double, lo = truth - hi = lo_rel |hi|.  lo_rel (|.| <= 2^-53)
                  is stored in float32 -- hi + lo then carries 77 bits of the truth, and a pair of full doubles per value would put
                  the file past the size of the largest committed fixture
    fragile       per path: a discrete decision of the scheme came within FRAGILE_REL = 1e-9 relative of its threshold at some
                  step of the truth (QE: psi against psi_c, u against p, the two existence tests of K0*; Heston Euler: v against
                  its floor; rough: volw_h against 0, relative to sum |w_i v_i|; Hawkes: -ln u against lambda dt).  Such paths
                  are left out of every comparison; at most 1 % of a case's paths may be fragile (asserted here)
    far_start_*   [3][130] the per-path start states of the far-states cases

oracle_err is the yardstick: the fp64 oracle's own error against the truth in the measure |d - truth| / max(|truth|, scale), the
largest over the non-fragile paths.  Scales: 1 for x; sigma0 (LogSV, a volatility), theta (Heston, a variance), sigma0 / sum w
(rough factors), theta_p, theta_m (Hawkes intensities) for the state; theta^2 T (LogSV), theta T (Heston), sigma0^2 T (rough) for
qvar, T = steps dt.

Far states: LogSV one and two steps from per-path start states, the oracle's own states sampled along the "explosive" and
"collapse" runs of tests/stress_extremes.py (sigma over many decades).  A start is kept only if the truth after two steps (both
step offsets) is finite in double (x, sigma, qvar, and sigma^2, which every fp64 evaluation of the step forms) with
|ln sigma| <= 600; 130 are kept per regime, spread evenly over ln sigma as far as the dynamics let a start live: kappa1 theta dt /
sigma and kappa2 sigma dt move ln sigma by more than 600 in one step outside 1e-4 < sigma < 1e4, and the second step narrows that
to about five decades (sigma from 4e-3 to 2e2).
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hawkes_twin as ht  # noqa: E402
from mc_steps_worker import checksum, hawkes_inputs, measure, normals, qe_uniforms  # noqa: E402  (shared with the tests)
from oracle import oracle  # noqa: E402

PREC = 256
mp.mp.prec = PREC
F = mp.mpf
RNG_STREAM_VERSION = 4
FRAGILE_REL = 1e-9
MAX_FRAGILE_SHARE = 0.01
N = 130
STEPS = (1, 2, 3, 7, 64)
LONG_STEPS, LONG_N = 1024, 64
ROUGH_STEPS = (1, 2, 5, 40)
HAWKES_STEPS = (1, 2, 3, 7, 64, 451)
HAWKES_DT = 0.02
MAX_BYTES = 1_000_000                                  # under the largest committed fixture (device_math.npz)
SEEDS = dict(logsv=20261, heston=20262, qe=20263, rough=20264, hawkes=20265, far=20266)

LOGSV_SETS = {"btc": dict(sigma0=0.8376, theta=1.0413, kappa1=3.1844, kappa2=3.058, beta=0.1514, volvol=1.8458),
              "test": dict(sigma0=0.2, theta=0.22, kappa1=3.0, kappa2=12.0, beta=-0.3, volvol=0.4)}
HESTON_SETS = {"base": dict(v0=0.04, theta=0.04, kappa=4.0, rho=-0.5, volvol=0.4),
               "btc": dict(v0=0.8, theta=1.0, kappa=2.0, rho=0.0, volvol=2.0)}
# test_heston_qe_branches_the_parameters_decide: the general kernel and the two kernels compiled without the exponential branch
QE_SETS = {"general": dict(v0=0.02, theta=0.02, kappa=1.0, rho=-0.7, volvol=1.0),
           "quad": dict(v0=0.5, theta=0.6, kappa=3.0, rho=0.0, volvol=1.2),
           "quad_tiny_volvol": dict(v0=0.04, theta=0.05, kappa=2.0, rho=-0.3, volvol=1e-5)}
DT_LOGSV = DT_HESTON = 1.0 / 360.0
DT_QE = 0.5 / 48
# tests/stress_extremes.py: (volvol, beta, steps) at dt 0.02, theta 1, kappa1 = kappa2 = 3, sigma0 0.8, seed 5, 20000 paths
FAR = {"explosive": (8.0, 2.0, 400), "collapse": (6.0, -3.0, 300)}
FAR_DT, FAR_BASE = 0.02, dict(sigma0=0.8, theta=1.0, kappa1=3.0, kappa2=3.0)


def near(a, b, scale=None):
    """the decision `a against b` is fragile"""
    s = abs(b) if scale is None else scale
    return abs(a - b) <= FRAGILE_REL * s


# ---- the recursions in mpmath; each returns {steps: [nq][n] of mpf} and the first fragile step per path (0 = never) -------------
def truth_logsv(start, dt, p, eta, spot, W0, W1, snaps):
    n = W0.shape[1]
    dt, eta = F(dt), F(eta)
    sdt = mp.sqrt(dt)
    theta, k1, k2, beta, volvol = (F(p[k]) for k in ("theta", "kappa1", "kappa2", "beta", "volvol"))
    alpha, adj = (F(-1), F(0)) if spot else (F(1), beta * eta)
    vartheta2, eta2 = beta * beta + volvol * volvol, eta * eta
    out = {s: [[None] * n for _ in range(3)] for s in snaps}
    for j in range(n):
        x, s, q = F(float(start[0][j])), F(float(start[1][j])), F(float(start[2][j]))
        L = mp.log(s)
        for t in range(max(snaps)):
            w0, w1 = sdt * F(float(W0[t, j])), sdt * F(float(W1[t, j]))
            s2dt = eta2 * s * s * dt
            x = x + alpha * F(0.5) * s2dt + eta * s * w0
            L = L + ((k1 * theta / s - k1) + k2 * (theta - s) + adj * s - F(0.5) * vartheta2) * dt + beta * w0 + volvol * w1
            s = mp.exp(L)
            q = q + F(0.5) * (s2dt + eta2 * s * s * dt)
            if t + 1 in out:
                for i, v in enumerate((x, s, q)):
                    out[t + 1][i][j] = v
    return out, np.zeros(n, dtype=np.int64)


def truth_heston(start, dt, p, W0, W1, snaps):
    n = W0.shape[1]
    dt = F(dt)
    sdt = mp.sqrt(dt)
    theta, kappa, rho, volvol = (F(p[k]) for k in ("theta", "kappa", "rho", "volvol"))
    rho_1, floor = mp.sqrt(1 - rho * rho), F(1e-4)
    out = {s: [[None] * n for _ in range(3)] for s in snaps}
    frag = np.zeros(n, dtype=np.int64)
    for j in range(n):
        x, v, q = F(float(start[0][j])), F(float(start[1][j])), F(float(start[2][j]))
        for t in range(max(snaps)):
            w0, w1 = sdt * F(float(W0[t, j])), sdt * F(float(W1[t, j]))
            s = mp.sqrt(v)
            s2dt = v * dt
            x = x - F(0.5) * s2dt + s * w0
            q = q + s2dt
            v = v + kappa * (theta - v) * dt + s * volvol * (rho * w0 + rho_1 * w1)
            if near(v, floor) and not frag[j]:
                frag[j] = t + 1
            v = max(v, floor)
            if t + 1 in out:
                for i, u in enumerate((x, v, q)):
                    out[t + 1][i][j] = u
    return out, frag


def truth_qe(start, dt, p, Z0, Z1, U, snaps):
    n = Z0.shape[1]
    dt = F(dt)
    theta, kappa, rho, volvol = (F(p[k]) for k in ("theta", "kappa", "rho", "volvol"))
    half = F(0.5)
    E = mp.exp(-kappa * dt)
    kre = kappa * rho / volvol - half
    c1 = volvol * volvol * E * (1 - E) / kappa
    c2 = theta * volvol * volvol * (1 - E) * (1 - E) / (2 * kappa)
    K1, K2 = half * dt * kre - rho / volvol, half * dt * kre + rho / volvol
    K3 = K4 = half * dt * (1 - rho * rho)
    A, K0_plain, K13 = K2 + half * K4, -rho * kappa * theta / volvol * dt, K1 + half * K3
    psi_c = F(1.5)
    out = {s: [[None] * n for _ in range(3)] for s in snaps}
    frag = np.zeros(n, dtype=np.int64)
    for j in range(n):
        x, v0, q = F(float(start[0][j])), F(float(start[1][j])), F(float(start[2][j]))
        for t in range(max(snaps)):
            z0, z1, u = F(float(Z0[t, j])), F(float(Z1[t, j])), F(float(U[t, j]))
            m = theta + (v0 - theta) * E
            s2 = v0 * c1 + c2
            psi = s2 / (m * m)
            fr = near(psi, psi_c)
            if psi <= psi_c:
                ip = 2 / psi
                b2 = ip - 1 + mp.sqrt(ip * (ip - 1))
                a = m / (1 + b2)
                b = mp.sqrt(b2)
                den = 1 - 2 * A * a
                fr = fr or near(den, 0, 1)
                v1 = a * (b + z1) * (b + z1)
                K0 = (-A * b2 * a / den + half * mp.log(den) - K13 * v0) if den > 0 else K0_plain
            else:
                pp = (psi - 1) / (psi + 1)
                bt = (1 - pp) / m
                fr = fr or near(u, pp) or near(A, bt)
                v1 = F(0) if u <= pp else mp.log((1 - pp) / (1 - u)) / bt
                K0 = (-mp.log(pp + bt * (1 - pp) / (bt - A)) - K13 * v0) if A < bt else K0_plain
            if fr and not frag[j]:
                frag[j] = t + 1
            x = x + K0 + K1 * v0 + K2 * v1 + mp.sqrt(K3 * v0 + K4 * v1) * z0
            q = q + half * dt * (v0 + v1)
            v0 = v1
            if t + 1 in out:
                for i, w in enumerate((x, v0, q)):
                    out[t + 1][i][j] = w
    return out, frag


def truth_rough(h, nodes, weights, v0f, p, Z0, Z1, snaps):
    """from the origin (0, v0, 0); quantities: log_s, the nf factors, y"""
    n, nf = Z0.shape[1], len(nodes)
    h = F(h)
    nodes, w, v0 = [F(float(a)) for a in nodes], [F(float(a)) for a in weights], [F(float(a)) for a in v0f]
    theta, k1, k2, rho, volvol = (F(p[k]) for k in ("theta", "kappa1", "kappa2", "rho", "volvol"))
    half = F(0.5)
    wsum = mp.fsum(w)
    wlam = [a * b for a, b in zip(w, nodes)]
    w_lam_v0 = mp.fsum(a * b for a, b in zip(wlam, v0))
    volvol_, rho_comp, sqrt_h, w_inv = volvol * wsum, mp.sqrt(1 - rho * rho), mp.sqrt(h), 1 / wsum
    rng = range(nf)

    def dot(a, b):
        return mp.fsum(a[i] * b[i] for i in rng)

    def slope(z):
        zw = dot(w, z)
        c = (k1 + k2 * zw) * (theta - zw)
        return [-nodes[i] * (z[i] - v0[i]) + c for i in rng]

    def rk4(z, hh):
        s1 = slope(z)
        s2 = slope([z[i] + half * hh * s1[i] for i in rng])
        s3 = slope([z[i] + half * hh * s2[i] for i in rng])
        s4 = slope([z[i] + hh * s3[i] for i in rng])
        return [z[i] + (hh / 6) * (s1[i] + 2 * s2[i] + 2 * s3[i] + s4[i]) for i in rng]

    out = {s: [[None] * n for _ in range(nf + 2)] for s in snaps}
    frag = np.zeros(n, dtype=np.int64)
    for j in range(n):
        ls, v, y = F(0), list(v0), F(0)
        for t in range(max(snaps)):
            z0, z1 = F(float(Z0[t, j])), F(float(Z1[t, j]))
            d = rk4(v, half * h)
            yw = dot(w, d)
            Yh = yw * mp.exp(-half * volvol_ ** 2 * h + volvol_ * (z0 * sqrt_h))
            Q = 1 / wsum * (Yh - yw)
            vh = rk4([d[i] + Q for i in rng], half * h)
            volw_h = dot(w, vh)
            if near(volw_h, 0, mp.fsum(abs(w[i] * vh[i]) for i in rng)) and not frag[j]:
                frag[j] = t + 1
            if not volw_h > 0:
                vh = [F(1e-6)] * nf
                volw_h = dot(w, vh)
            vw, w_lam_vol, w_lam_vol_h = dot(w, v), dot(wlam, v), dot(wlam, vh)
            sq_vw, sq_vhw = vw * vw, volw_h * volw_h
            term1 = 1 / volvol * (((volw_h - vw) / h + half * w_lam_vol + half * w_lam_vol_h - w_lam_v0) * w_inv
                                  - k1 * theta + (k1 - k2 * theta) * (half * vw + half * volw_h)
                                  + k2 * (half * sq_vw + half * sq_vhw)) * h
            term2 = half * h * sq_vw + half * h * sq_vhw
            ls = ls - half * term2 + rho * term1 + rho_comp * mp.sqrt(term2) * z1
            y = y + half * h * (vw * vw + volw_h * volw_h)
            v = vh
            if t + 1 in out:
                for i, u in enumerate([ls] + v + [y]):
                    out[t + 1][i][j] = u
    return out, frag


def truth_hawkes(dt, p, d, snaps):
    """d: hawkes_twin.hawkes_draws; start (0, lambda_p, lambda_m); also the number of paths that jumped on each side per snap"""
    n = d["z"].shape[1]
    dt = F(dt)
    P = {k: F(float(v)) for k, v in p.items()}
    sdt = mp.sqrt(dt)
    comp_p = dt * (mp.exp(P["shift_p"]) / (1 - P["mean_p"]) - 1)
    comp_m = dt * (mp.exp(P["shift_m"]) / (1 - P["mean_m"]) - 1)
    drift_dt = (P["mu"] - F(0.5) * P["sigma"] * P["sigma"]) * dt
    out = {s: [[None] * n for _ in range(3)] for s in snaps}
    frag = np.zeros(n, dtype=np.int64)
    first_p, first_m = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    # the unit exponentials the twin holds are -ln of exact uniforms: recover the uniforms' words for an exact -ln in mpmath
    for j in range(n):
        x, lp, lm = F(0), P["lambda_p"], P["lambda_m"]
        for t in range(max(snaps)):
            w0 = sdt * F(float(d["z"][t, j]))
            eu_p, eu_m = -mp.log(F(float(d["u_p"][t, j]))), -mp.log(F(float(d["u_m"][t, j])))
            diffusion = drift_dt - comp_p * lp - comp_m * lm + P["sigma"] * w0
            if (near(lp * dt, eu_p) or near(lm * dt, eu_m)) and not frag[j]:
                frag[j] = t + 1
            jp = (P["shift_p"] + P["mean_p"] * -mp.log(F(float(d["v_p"][t, j])))) if lp > eu_p / dt else F(0)
            jm = (P["shift_m"] - (-P["mean_m"]) * -mp.log(F(float(d["v_m"][t, j])))) if lm > eu_m / dt else F(0)
            if jp != 0 and not first_p[j]:
                first_p[j] = t + 1
            if jm != 0 and not first_m[j]:
                first_m[j] = t + 1
            x = x + diffusion + jp + jm
            load_p = P["beta1_p"] * jp + P["beta2_p"] * jm
            load_m = P["beta1_m"] * jp + P["beta2_m"] * jm
            lp = lp + P["kappa_p"] * (P["theta_p"] - lp) * dt + load_p
            lm = lm + P["kappa_m"] * (P["theta_m"] - lm) * dt + load_m
            if t + 1 in out:
                for i, u in enumerate((x, lp, lm)):
                    out[t + 1][i][j] = u
    return out, frag, first_p, first_m


def hawkes_grid(steps):
    """(ttm, steps per year) that hawkes_twin.time_grid turns into `steps` steps, and the dt it computes"""
    ttm = steps * HAWKES_DT
    spy = (steps - 0.5) / ttm
    nb, dt = ht.time_grid(ttm, spy)
    assert nb == steps
    return ttm, spy, dt


# ---- bookkeeping ----------------------------------------------------------------------------------------------------------------
class Book:
    def __init__(self):
        self.cases, self.hi, self.lo, self.frag = [], [], [], []
        self.off = self.foff = 0

    def add(self, meta, truth, fragile, oracle_state, numpy_state=None):
        """truth [nq][n] of mpf; oracle_state / numpy_state [nq][n] of doubles"""
        nq, n = len(truth), len(truth[0])
        hi = np.array([[float(v) for v in row] for row in truth])
        lo = np.array([[float(v - F(float(h))) for v, h in zip(row, hrow)] for row, hrow in zip(truth, hi)])
        assert np.all(np.isfinite(hi)), meta["id"]
        share = float(np.mean(fragile))
        assert share <= MAX_FRAGILE_SHARE, (meta["id"], share)
        meta = dict(meta, nq=nq, n=n, off=self.off, foff=self.foff, fragile_paths=int(np.sum(fragile)))
        with np.errstate(all="ignore"):
            lo32 = np.where(hi != 0.0, lo / np.abs(hi), 0.0).astype(np.float32)
        assert np.all(lo[hi == 0.0] == 0.0), meta["id"]    # a truth whose nearest double is 0 is 0 (QE's v = 0 branch)
        lo = lo32.astype(np.float64) * np.abs(hi)           # as tests/mc_steps_worker.py Fixture rebuilds it
        meta["oracle_err"] = measure(np.asarray(oracle_state), hi, lo, fragile, meta["scales"])
        if numpy_state is not None:
            meta["numpy_err"] = measure(np.asarray(numpy_state), hi, lo, fragile, meta["scales"])
        self.cases.append(meta)
        self.hi.append(hi.ravel()), self.lo.append(lo32.ravel()), self.frag.append(np.asarray(fragile, dtype=bool))
        self.off += nq * n
        self.foff += n
        print(meta["id"], "fragile", meta["fragile_paths"], "oracle_err", ["%.2e" % e for e in meta["oracle_err"]], flush=True)


def const_start(n, *vals):
    return [np.full(n, v) for v in vals]


def step_plan():
    """(n, offset, snaps) runs: the 130-path cases are prefixes of one 64-step run per offset"""
    return [(N, 0, STEPS), (N, 1, STEPS), (LONG_N, 0, (LONG_STEPS,))]


def build():
    book = Book()

    # LogSV
    seed = SEEDS["logsv"]
    for sname, p in LOGSV_SETS.items():
        for spot in (True, False):
            for eta in (1.0, 0.7):
                for n, off, snaps in step_plan():
                    if max(snaps) == LONG_STEPS and not (sname == "btc" and spot and eta == 1.0):
                        continue
                    W0, W1 = normals(seed, n, max(snaps), off, 0)
                    st = const_start(n, 0.0, p["sigma0"], 0.0)
                    tr, fr = truth_logsv(st, DT_LOGSV, p, eta, spot, W0, W1, snaps)
                    for s in snaps:
                        a = (p["theta"], p["kappa1"], p["kappa2"], p["beta"], p["volvol"], W0[:s], W1[:s])
                        o = oracle.logsv_terminal_w(*st, DT_LOGSV, *a, eta=eta, is_spot_measure=spot)
                        o2 = oracle.np_logsv_terminal_w(*st, DT_LOGSV, *a, eta=eta, is_spot_measure=spot)
                        book.add(dict(id=f"logsv-{sname}-{'spot' if spot else 'inv'}-eta{eta:g}-s{s}-o{off}", gen="logsv", set=sname,
                                      params=p, eta=eta, spot=spot, steps=s, dt=DT_LOGSV, offset=off, seed=seed,
                                      start=[0.0, p["sigma0"], 0.0], scales=[1.0, p["sigma0"], p["theta"] ** 2 * s * DT_LOGSV],
                                      checksum=checksum(W0[:s], W1[:s])), tr[s], (fr > 0) & (fr <= s), o, o2)

    # Heston Euler
    seed = SEEDS["heston"]
    for sname, p in HESTON_SETS.items():
        for n, off, snaps in step_plan():
            if max(snaps) == LONG_STEPS and sname != "btc":
                continue
            W0, W1 = normals(seed, n, max(snaps), off, 0)
            st = const_start(n, 0.0, p["v0"], 0.0)
            tr, fr = truth_heston(st, DT_HESTON, p, W0, W1, snaps)
            for s in snaps:
                a = (p["theta"], p["kappa"], p["rho"], p["volvol"], W0[:s], W1[:s])
                o = oracle.heston_terminal_w(*st, DT_HESTON, *a)
                o2 = oracle.np_heston_terminal_w(*st, DT_HESTON, *a)
                book.add(dict(id=f"heston-{sname}-s{s}-o{off}", gen="heston", set=sname, params=p, steps=s, dt=DT_HESTON, offset=off,
                              seed=seed, start=[0.0, p["v0"], 0.0], scales=[1.0, p["theta"], p["theta"] * s * DT_HESTON],
                              checksum=checksum(W0[:s], W1[:s])), tr[s], (fr > 0) & (fr <= s), o, o2)

    # Heston QE
    seed = SEEDS["qe"]
    for sname, p in QE_SETS.items():
        for n, off, snaps in step_plan():
            if max(snaps) == LONG_STEPS and sname != "general":
                continue
            Z0, Z1 = normals(seed, n, max(snaps), off, 4)
            U = qe_uniforms(seed, n, max(snaps), off)
            st = const_start(n, 0.0, p["v0"], 0.0)
            tr, fr = truth_qe(st, DT_QE, p, Z0, Z1, U, snaps)
            for s in snaps:
                o = oracle.heston_qe_terminal_w(*st, DT_QE, p["theta"], p["kappa"], p["rho"], p["volvol"], Z0[:s], Z1[:s], U[:s])
                book.add(dict(id=f"qe-{sname}-s{s}-o{off}", gen="qe", set=sname, params=p, steps=s, dt=DT_QE, offset=off, seed=seed,
                              start=[0.0, p["v0"], 0.0], scales=[1.0, p["theta"], p["theta"] * s * DT_QE],
                              checksum=checksum(Z0[:s], Z1[:s], U[:s])), tr[s], (fr > 0) & (fr <= s), o)

    # rough LogSV: the three Hurst cases of rough.npz carry the three factor counts the library instantiates (3, 2, 1)
    seed = SEEDS["rough"]
    g = np.load(os.path.join(HERE, "rough.npz"))
    sigma0, theta, kappa1, kappa2, beta, orthog = (float(a) for a in g["params"])
    volvol = float(np.sqrt(beta ** 2 + orthog ** 2))
    rp = dict(theta=theta, kappa1=kappa1, kappa2=kappa2, rho=beta / volvol, volvol=volvol)
    h = 1.0 / 360.0
    for tag in ("h010", "h045", "h050"):
        nodes, weights = g[f"{tag}_nodes"], g[f"{tag}_weights"]
        nf = nodes.size
        v0f = np.full(nf, sigma0 / np.sum(weights))
        for off in (0, 1):
            Z0, Z1 = normals(seed, N, max(ROUGH_STEPS), off, 3)
            tr, fr = truth_rough(h, nodes, weights, v0f, rp, Z0, Z1, ROUGH_STEPS)
            for s in ROUGH_STEPS:
                ls, y = np.zeros(N), np.zeros(N)
                vol = np.ascontiguousarray(np.repeat(v0f[:, None], N, axis=1))
                z0, z1 = np.ascontiguousarray(Z0[:s]), np.ascontiguousarray(Z1[:s])
                oracle.lib().svo_rough_logsv_terminal_w(N, s, h, nf, oracle._p(np.ascontiguousarray(nodes)),
                                                        oracle._p(np.ascontiguousarray(weights)), oracle._p(v0f), theta, kappa1, kappa2,
                                                        rp["rho"], volvol, oracle._p(ls), oracle._p(vol), oracle._p(y), oracle._p(z0),
                                                        oracle._p(z1), N)
                book.add(dict(id=f"rough-{tag}-s{s}-o{off}", gen="rough", set=tag, params=rp, nodes=nodes.tolist(),
                              weights=weights.tolist(), v0=v0f.tolist(), steps=s, dt=h, offset=off, seed=seed,
                              scales=[1.0] + [float(v0f[0])] * nf + [sigma0 ** 2 * s * h], checksum=checksum(z0, z1)),
                         tr[s], (fr > 0) & (fr <= s), np.vstack([ls[None], vol, y[None]]))

    # Hawkes
    seed = SEEDS["hawkes"]
    for sname in ("hawkes_mc", "hawkes_mc_excited"):
        p = dict(zip(ht.PARAM_NAMES, (float(v) for v in np.load(os.path.join(HERE, sname + ".npz"))["params"])))
        for off in (0, 1):
            d = hawkes_inputs(seed, N, max(HAWKES_STEPS), off)
            tr, fr, fp, fm = truth_hawkes(HAWKES_DT, p, d, HAWKES_STEPS)
            for s in HAWKES_STEPS:
                ttm, spy, dt = hawkes_grid(s)
                if dt != HAWKES_DT:                        # ttm / steps did not round back: this count's own truth at its own dt
                    trs, frs, fps, fms = truth_hawkes(dt, p, {k: v[:s] for k, v in d.items()}, (s,))
                else:
                    trs, frs, fps, fms = tr, fr, fp, fm
                share_p, share_m = np.mean((fps > 0) & (fps <= s)), np.mean((fms > 0) & (fms <= s))
                assert share_p >= 0.05 and share_m >= 0.05, (sname, s, off, share_p, share_m)
                o = ht.simulate_terminal(ttm, np.zeros(N), np.full(N, p["lambda_p"]), np.full(N, p["lambda_m"]), p, seed, 0, 0, off,
                                         spy)
                assert o[3] == s
                book.add(dict(id=f"hawkes-{sname}-s{s}-o{off}", gen="hawkes", set=sname, params=p, steps=s, dt=dt, ttm=ttm, spy=spy,
                              offset=off, seed=seed, start=[0.0, p["lambda_p"], p["lambda_m"]],
                              scales=[1.0, p["theta_p"], p["theta_m"]], jumped=[float(share_p), float(share_m)],
                              checksum=checksum(*[d[k][:s] for k in ("z", "u_p", "u_m", "v_p", "v_m")])),
                         trs[s], (frs > 0) & (frs <= s), np.stack(o[:3]))

    return book, build_far(book)


def build_far(book):
    """LogSV far states (module docstring)"""
    seed = SEEDS["far"]
    far_start = {}
    for regime, (volvol, beta, nb) in FAR.items():
        p = dict(FAR_BASE, beta=beta, volvol=volvol)
        n_run, pool = 20000, []
        x, s, q = np.zeros(n_run), np.full(n_run, p["sigma0"]), np.zeros(n_run)
        with np.errstate(all="ignore"):
            for t0 in range(0, nb, 10):
                x, s, q = oracle.logsv_terminal_rng(x, s, q, 10, FAR_DT, p["theta"], p["kappa1"], p["kappa2"], beta, volvol, 5,
                                                    step_offset=t0)
                ok = np.isfinite(x) & np.isfinite(q) & np.isfinite(s) & (s > 0)
                pool.append(np.stack([x[ok], s[ok], q[ok]]))
        pool = np.concatenate(pool, axis=1)
        # a start whose drift term kappa1 theta dt / sigma or kappa2 sigma dt alone passes 700 cannot end within |ln sigma| <= 600:
        # not worth a truth evaluation.  Of the rest, 3000 spread evenly over ln sigma.
        with np.errstate(all="ignore"):
            pool = pool[:, (p["kappa1"] * p["theta"] * FAR_DT / pool[1] <= 700.0) & (p["kappa2"] * FAR_DT * pool[1] <= 700.0)]
        pool = pool[:, np.argsort(np.log(pool[1]))]
        ln = np.log(pool[1])
        pool = pool[:, np.unique(np.searchsorted(ln, np.linspace(ln[0], ln[-1], 3000)).clip(0, ln.size - 1))]
        ln = np.log(pool[1])
        print(regime, "pool", pool.shape[1], "ln sigma from", ln[0], "to", ln[-1], flush=True)
        W = {off: normals(seed, N, 2, off, 0) for off in (0, 1)}
        # slot j becomes path j: the unused start nearest its target in ln sigma that survives two steps on path j's normals
        # (towards the ends of the range the nearest survivor is the edge of what the dynamics let live)
        targets = np.linspace(ln[0], ln[-1], N)
        kept, used = [], set()
        for j, tgt in enumerate(targets):
            for c in np.argsort(np.abs(ln - tgt)):
                if int(c) in used:
                    continue
                st = [pool[i, c:c + 1] for i in range(3)]
                good = True
                for off in (0, 1):
                    try:
                        tr, _ = truth_logsv(st, FAR_DT, p, 1.0, True, W[off][0][:, j:j + 1], W[off][1][:, j:j + 1], (1, 2))
                    except OverflowError:                  # exp of a log-volatility past mpmath's own exponent range
                        good = False
                        break
                    vals = [float(tr[k][i][0]) for k in (1, 2) for i in range(3)] + [float(tr[k][1][0] ** 2) for k in (1, 2)]
                    good = good and all(np.isfinite(vals)) and all(abs(mp.log(tr[k][1][0])) <= 600 for k in (1, 2))
                if good:
                    kept.append(int(c)), used.add(int(c))
                    break
            else:
                raise AssertionError((regime, j, "no start survives two steps"))
        st = [pool[i, kept] for i in range(3)]
        far_start[regime] = np.stack(st)
        print(regime, "kept ln sigma from", np.log(st[1]).min(), "to", np.log(st[1]).max(), flush=True)
        for off in (0, 1):
            W0, W1 = W[off]
            tr, fr = truth_logsv(st, FAR_DT, p, 1.0, True, W0, W1, (1, 2))
            for s in (1, 2):
                with np.errstate(all="ignore"):
                    a = (p["theta"], p["kappa1"], p["kappa2"], beta, volvol, W0[:s], W1[:s])
                    o = oracle.logsv_terminal_w(*st, FAR_DT, *a)
                    o2 = oracle.np_logsv_terminal_w(*st, FAR_DT, *a)
                book.add(dict(id=f"far-{regime}-s{s}-o{off}", gen="far", set=regime, params=p, eta=1.0, spot=True, steps=s, dt=FAR_DT,
                              offset=off, seed=seed, start=regime, scales=[1.0, p["sigma0"], p["theta"] ** 2 * s * FAR_DT],
                              checksum=checksum(W0[:s], W1[:s], *st)), tr[s], (fr > 0) & (fr <= s), o, o2)
    return far_start


def main():
    oracle.build()
    book, far_start = build()
    meta = dict(rng_stream_version=RNG_STREAM_VERSION, prec=PREC, fragile_rel=FRAGILE_REL, max_fragile_share=MAX_FRAGILE_SHARE,
                cases=book.cases)
    path = os.path.join(HERE, "mc_steps.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), hi=np.concatenate(book.hi), lo_rel=np.concatenate(book.lo),
                        fragile=np.packbits(np.concatenate(book.frag)), **{f"far_start_{k}": v for k, v in far_start.items()})
    size = os.path.getsize(path)
    print(len(book.cases), "cases,", size, "bytes")
    assert size < MAX_BYTES, size


if __name__ == "__main__":
    main()
