"""
Generate tests/golden/hawkes_transform_odes.npz, the high-precision solutions of the Hawkes jump-diffusion's coefficient ODEs
that tests/test_hawkes_transform_host.py and tests/test_gpu_hawkes_transform.py hold a numpy RK4 and the device kernels
(hawkes_mgf_grid_batch_kernel, hawkes_risk_forwards_kernel) to.  Everything is computed here in mpmath (no GPU):

    python tests/golden/make_golden_hawkes_transform_odes.py [--jobs 16]

The right-hand side is func_rhs of the reference's solve_ode_for_a (pricers/hawkes_jd_pricer.py:582-640), written below in
mpmath from the double parameters:

    z_p = phi - beta1_p a1 - beta1_m a2,            z_m = phi - beta2_p a1 - beta2_m a2
    a0' = kappa_p theta_p a1 + kappa_m theta_m a2 + sigma^2 (phi (phi + 1) / 2 - psi)
    a1' = exp(-shift_p z_p) / (1 + mean_p z_p) - 1 - kappa_p a1 + (exp(shift_p) / (1 - mean_p) - 1) phi
    a2' = exp(-shift_m z_m) / (1 + mean_m z_m) - 1 - kappa_m a2 + (exp(shift_m) / (1 - mean_m) - 1) phi
    log E = a0 + a1 lambda_p + a2 lambda_m                                                           (:545)

The system is not polynomial, but the Taylor coefficients of exp(u(t)) and of 1 / d(t) follow from those of u and d by the
usual recurrences (E_n = (1/n) sum k u_k E_(n-k); R_n = -R_0 sum d_k R_(n-k)), so the solution's own Taylor series at a
point is built term by term and summed over a step as long as its last two terms allow at the solve's tolerance.  Every
point is solved twice, independently (SOLVES: 40 digits, 24 terms, 1e-25; 50 digits, 30 terms, 1e-30: different steps,
orders and precisions); the value kept is the second and `agree` = |a - b| / max(1, |b|), the largest over the three
components and log E, is the error bound of the stored value.  Nothing is written unless agree <= 1e-16 everywhere.

Self-checks before anything is integrated: at 100 random (phi, a) points the mp right-hand side, rounded to double, agrees
to 1e-14 relative with the reference's own func_rhs where the reference's source is present (imported with the numba shim
and read out of solve_ode_for_a through its solve_ivp call; never copied); the first Taylor coefficient of the series equals
the mp right-hand side; and the solver reproduces the closed form of the decoupled set to 1e-16.

  names, params   the parameter sets (SVMC_HAWKESJD_PARAMS order, PARAM_NAMES below): the reference's default set, the
                  hawkes_mc_excited set, and
                    asym        strongly asymmetric cross-excitation (beta1_m = 60 against beta2_p = -9), no _p quantity
                                equal to its _m twin
                    decoupled   all four betas zero: a1' = j_p(phi) - kappa_p a1 + comp_p phi has a constant forcing
                    pure_shift  mean_p = mean_m = 0: the jump transform a bare exponential
                    no_shift    shift_p = shift_m = 0
                    kappa_zero  kappa_m = 0 (with beta1_m = 6, beta2_m = -4)
                    sigma_zero  sigma = 0: h0 = 0
  vol_scaler      set_vol_scaler(sigma, 1/365) of each set
  phi [S][P]      P = 14 points of the set's own pricer grid (get_transform_var_grid at MAX_PHI = 500 points: indices 0, 1, 2,
                  the last and ten spread between) and the six real points phi = -gamma - k, gamma in GAMMAS, k in (0, 1),
                  in the order (gamma, k); psi = 0
  ttms, a [S][T][P][3], log_mgf [S][T][P], agree [S][T][P]   from zero over each whole ttm
  defined [S][T][P]   False where the exact solution has a pole before the ttm (1 + mean z reaches 0: some real points at two
                  years on the strongly excited sets): both solves' steps shrank below 1e-12 there, a and log_mgf are NaN,
                  and the device has to give the point up.  Every grid point, every ttm below two years, and every point of
                  the default, asym and decoupled sets is defined.
  closed_a, closed_log_mgf [T][P]   the decoupled set's closed form
  giveup_*        the give-up case: the largest gamma and the ttm of hawkes_risk_premia.npz's `failed` entries (the reference's
                  own solver fails there), on the default set.  Of the entry's two real points the solution at
                  giveup_phi = -gamma - 1 has a pole before that ttm (both solves must find it; the one at -gamma exists);
                  giveup_a, giveup_log_mgf, giveup_agree [P] are the set's P points at that ttm, the neighbours the device
                  test puts in the same wave.
  chain_*         the a_t0 carry on CHAIN_SET: a at CHAIN_TTMS[0] from zero (rounded to complex128, as the device hands it
                  on), then CHAIN_TTMS[1] more from that rounded state
"""
import argparse
import os
import sys
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import mpmath as mp  # noqa: E402
import numpy as np  # noqa: E402

REFERENCE_SRC = "/root/reference/src"

PARAM_NAMES = ("mu", "sigma", "shift_p", "mean_p", "shift_m", "mean_m", "lambda_p", "theta_p", "kappa_p", "beta1_p", "beta2_p",
               "lambda_m", "theta_m", "kappa_m", "beta1_m", "beta2_m")
DEFAULT = dict(mu=0.0, sigma=0.45, shift_p=0.06, mean_p=0.03, shift_m=-0.06, mean_m=-0.03, lambda_p=6.55, theta_p=6.55,
               kappa_p=22.29, beta1_p=76.0, beta2_p=-67.58, lambda_m=8.50, theta_m=8.50, kappa_m=29.0, beta1_m=104.55,
               beta2_m=-109.6)
TTMS = np.array([1.0 / 365.0, 0.25, 2.0])
GAMMAS = np.array([-2.0, 0.5, 3.0])
MAX_PHI = 500                                          # the pricer's grid length (pricers/hawkes_jd_pricer.py)
PHI_IDX = np.unique(np.concatenate([[0, 1, 2, MAX_PHI - 1], np.linspace(3, MAX_PHI - 2, 10).astype(int)]))
CHAIN_SET = "asym"
CHAIN_TTMS = np.array([0.1, 0.15])
SOLVES = ((40, 24, 1e-25), (50, 30, 1e-30))            # (digits, Taylor terms, step tolerance)
MAX_STEPS = 100_000


def parameter_sets():
    excited = np.load(os.path.join(HERE, "hawkes_mc_excited.npz"))["params"]
    sets = {"default": dict(DEFAULT), "excited": dict(zip(PARAM_NAMES, (float(v) for v in excited)))}
    sets["asym"] = dict(mu=0.0, sigma=0.35, shift_p=0.07, mean_p=0.04, shift_m=-0.04, mean_m=-0.05, lambda_p=12.0, theta_p=5.0,
                        kappa_p=18.0, beta1_p=40.0, beta2_p=-9.0, lambda_m=4.0, theta_m=11.0, kappa_m=35.0, beta1_m=60.0,
                        beta2_m=-50.0)
    sets["decoupled"] = dict(DEFAULT, beta1_p=0.0, beta2_p=0.0, beta1_m=0.0, beta2_m=0.0)
    sets["pure_shift"] = dict(DEFAULT, mean_p=0.0, mean_m=0.0)
    sets["no_shift"] = dict(DEFAULT, shift_p=0.0, shift_m=0.0)
    # without decay the default betas carry every real point to a pole within two years: weaker loads on lambda_m
    sets["kappa_zero"] = dict(DEFAULT, kappa_m=0.0, beta1_m=6.0, beta2_m=-4.0)
    sets["sigma_zero"] = dict(DEFAULT, sigma=0.0)
    return sets


def set_points(p):
    """(vol_scaler, phi [P]) of one set: its pricer grid's points, then the forwards kernel's real ones"""
    from stochvolmodels_amd.pricers.hawkes_jd_pricer import MAX_PHI as PRICER_MAX_PHI, set_vol_scaler
    from stochvolmodels_amd.utils.mgf_pricer import get_transform_var_grid
    assert PRICER_MAX_PHI == MAX_PHI
    vs = float(set_vol_scaler(sigma0=p["sigma"], ttm=float(TTMS.min())))
    grid = get_transform_var_grid(variable_type=1, max_phi=MAX_PHI, vol_scaler=vs)[0]
    real = np.array([complex(-g - k) for g in GAMMAS for k in (0.0, 1.0)])
    return vs, np.concatenate([grid[PHI_IDX], real])


# ---- the right-hand side in mpmath, from the reference's formulas ----------------------------------------------------------
def mp_params(p):
    q = {k: mp.mpf(float(v)) for k, v in p.items()}
    q["comp_p"] = mp.exp(q["shift_p"]) / (1 - q["mean_p"]) - 1                                      # :69
    q["comp_m"] = mp.exp(q["shift_m"]) / (1 - q["mean_m"]) - 1                                      # :70
    return q


def mp_rhs(q, phi, psi, a):
    def e_p(z):
        return mp.exp(-q["shift_p"] * z) / (1 + q["mean_p"] * z)

    def e_m(z):
        return mp.exp(-q["shift_m"] * z) / (1 + q["mean_m"] * z)
    j_p = e_p(phi - q["beta1_p"] * a[1] - q["beta1_m"] * a[2]) - 1
    j_m = e_m(phi - q["beta2_p"] * a[1] - q["beta2_m"] * a[2]) - 1
    return [q["kappa_p"] * q["theta_p"] * a[1] + q["kappa_m"] * q["theta_m"] * a[2]
            + q["sigma"] ** 2 * ((phi + 1) * phi / 2 - psi),
            j_p - q["kappa_p"] * a[1] + q["comp_p"] * phi,
            j_m - q["kappa_m"] * a[2] + q["comp_m"] * phi]


def mp_log_mgf(q, a):
    return a[0] + a[1] * q["lambda_p"] + a[2] * q["lambda_m"]


# ---- the solution's Taylor series at a point -------------------------------------------------------------------------------
class JumpSeries:
    """the Taylor coefficients of exp(-shift z(t)) / (1 + mean z(t)) - 1, extended one order at a time from those of z"""

    def __init__(self, shift, mean):
        self.shift, self.mean = shift, mean
        self.u, self.d, self.E, self.R = [], [], [], []

    def push(self, z_m):
        m = len(self.u)
        self.u.append(-self.shift * z_m)
        self.d.append(self.mean * z_m + (1 if m == 0 else 0))
        if m == 0:
            self.E.append(mp.exp(self.u[0]))
            self.R.append(1 / self.d[0])
        else:
            self.E.append(mp.fsum(k * self.u[k] * self.E[m - k] for k in range(1, m + 1)) / m)
            self.R.append(-self.R[0] * mp.fsum(self.d[k] * self.R[m - k] for k in range(1, m + 1)))
        j = mp.fsum(self.E[k] * self.R[m - k] for k in range(m + 1))
        return j - 1 if m == 0 else j


def taylor(q, phi, psi, y, terms):
    """c[m][i], m = 0 .. terms: the Taylor coefficients of the solution through y"""
    c = [list(y)]
    jp, jm = JumpSeries(q["shift_p"], q["mean_p"]), JumpSeries(q["shift_m"], q["mean_m"])
    h0 = q["sigma"] ** 2 * ((phi + 1) * phi / 2 - psi)
    for m in range(terms):
        a = c[m]
        lead = phi if m == 0 else 0
        j_p = jp.push(lead - q["beta1_p"] * a[1] - q["beta1_m"] * a[2])
        j_m = jm.push(lead - q["beta2_p"] * a[1] - q["beta2_m"] * a[2])
        f = [q["kappa_p"] * q["theta_p"] * a[1] + q["kappa_m"] * q["theta_m"] * a[2] + (h0 if m == 0 else 0),
             j_p - q["kappa_p"] * a[1] + (q["comp_p"] * phi if m == 0 else 0),
             j_m - q["kappa_m"] * a[2] + (q["comp_m"] * phi if m == 0 else 0)]
        c.append([v / (m + 1) for v in f])
    return c


def integrate(q, phi, psi, y0, ttms, terms, tol):
    """the mp states at each of the (increasing, double) times from y0 at 0; None from a time the solve cannot reach"""
    y, t, out, steps = list(y0), mp.mpf(0), [], 0
    for T in ttms:
        T = mp.mpf(float(T))
        while t < T:
            c = taylor(q, phi, psi, y, terms)
            scale = max(1, max(abs(v) for v in y))
            h = T - t
            for m in (terms - 1, terms):
                top = max(abs(v) for v in c[m])
                if top > 0:
                    h = min(h, (tol * scale / top) ** (mp.mpf(1) / m) / 2)             # a factor 2 of margin
            steps += 1
            if steps > MAX_STEPS or not h > mp.mpf(10) ** -12:
                return out + [None] * (len(ttms) - len(out))
            y = [mp.polyval([c[m][i] for m in range(terms, -1, -1)], h) for i in range(3)]
            t = T if h == T - t else t + h
        out.append(list(y))
    return out


def solve_point(args):
    """(a [T][3], log E [T], agree [T]) of one point from y0 (three complex doubles) at the times cumsum'd by the caller"""
    p, phi, ttms, y0 = args
    outs = []
    for dps, terms, tol in SOLVES:
        with mp.workdps(dps):
            q = mp_params(p)
            res = integrate(q, mp.mpc(complex(phi)), mp.mpc(0), [mp.mpc(complex(v)) for v in y0], ttms, terms, mp.mpf(tol))
            outs.append([None if r is None else r + [mp_log_mgf(q, r)] for r in res])
    T = len(ttms)
    a, lm, agree = np.full((T, 3), np.nan + 0j), np.full(T, np.nan + 0j), np.full(T, np.inf)
    with mp.workdps(60):
        for t, (r1, r2) in enumerate(zip(*outs)):
            if r1 is None and r2 is None:                      # a pole before this ttm: not defined
                agree[t] = np.nan
                continue
            if r1 is None or r2 is None:
                continue
            agree[t] = float(max(abs(x - y) / max(mp.mpf(1), abs(y)) for x, y in zip(r1, r2)))
            a[t] = [complex(v) for v in r2[:3]]
            lm[t] = complex(r2[3])
    return a, lm, agree


# ---- the decoupled set's closed form ---------------------------------------------------------------------------------------
def closed_form(p, phi, ttm):
    """[a0, a1, a2, log E] in mp with all four betas zero: a_i' = c_i - kappa_i a_i, c_i = j_i(phi) + comp_i phi constant"""
    q = mp_params(p)
    assert all(q[k] == 0 for k in ("beta1_p", "beta2_p", "beta1_m", "beta2_m"))
    phi, t = mp.mpc(complex(phi)), mp.mpf(float(ttm))
    a, integral = {}, {}
    for s in ("p", "m"):
        c = mp.exp(-q["shift_" + s] * phi) / (1 + q["mean_" + s] * phi) - 1 + q["comp_" + s] * phi
        k = q["kappa_" + s]
        a[s] = c * (-mp.expm1(-k * t) / k if k != 0 else t)
        integral[s] = c * ((t + mp.expm1(-k * t) / k) / k if k != 0 else t * t / 2)
    a0 = (q["sigma"] ** 2 * ((phi + 1) * phi / 2)) * t + q["kappa_p"] * q["theta_p"] * integral["p"] \
        + q["kappa_m"] * q["theta_m"] * integral["m"]
    y = [a0, a["p"], a["m"]]
    return y + [mp_log_mgf(q, y)]


# ---- self-checks -----------------------------------------------------------------------------------------------------------
def reference_rhs(p, phi):
    """the reference's own func_rhs for (p, phi, psi = 0), read out of solve_ode_for_a's solve_ivp call"""
    import stochvolmodels.pricers.hawkes_jd_pricer as hp
    orig, got = hp.solve_ivp, {}

    def capture(fun, **kw):
        got["fun"] = fun
    hp.solve_ivp = capture
    try:
        hp.solve_ode_for_a(ttm=1.0, model_params=hp.HawkesJDParams(**p), phi=phi, psi=0j)
    finally:
        hp.solve_ivp = orig
    return got["fun"]


def self_check(sets):
    rng = np.random.default_rng(20261018)
    names = list(sets)
    have_ref = os.path.isdir(REFERENCE_SRC)
    if have_ref:
        sys.path.insert(0, os.path.join(HERE, "_shims"))
        sys.path.insert(0, REFERENCE_SRC)
    worst_ref = worst_series = 0.0
    for trial in range(100):
        p = sets[names[trial % len(names)]]
        phi = complex(-0.5, rng.uniform(0, 240)) if trial % 3 else complex(rng.uniform(-4, 2), 0.0)
        a = (rng.normal(size=3) + 1j * rng.normal(size=3)) * np.array([3.0, 0.05, 0.05])
        with mp.workdps(40):
            q = mp_params(p)
            am = [mp.mpc(complex(v)) for v in a]
            exact_mp = mp_rhs(q, mp.mpc(phi), mp.mpc(0), am)
            c1 = taylor(q, mp.mpc(phi), mp.mpc(0), am, 1)[1]
            worst_series = max(worst_series, float(max(abs(x - y) for x, y in zip(c1, exact_mp))))
            exact = np.array([complex(v) for v in exact_mp])
        if have_ref:
            r = np.asarray(reference_rhs(p, phi)(0.0, a))
            worst_ref = max(worst_ref, float(np.max(np.abs(r - exact)) / np.max(np.abs(exact))))
    print(f"self-check: mp right-hand side vs the reference's func_rhs {worst_ref:.2e}"
          + ("" if have_ref else " (reference not present: skipped)") + f", series' first term vs mp rhs {worst_series:.2e}",
          flush=True)
    assert worst_ref <= 1e-14 and worst_series <= 1e-35, (worst_ref, worst_series)
    p = sets["decoupled"]
    worst = 0.0
    for phi in set_points(p)[1][[0, 1, 7, 13, 14, 19]]:
        _, _, agree = solve_point((p, phi, TTMS, np.zeros(3)))
        worst = max(worst, float(agree.max()))
        for dps, terms, tol in SOLVES:
            with mp.workdps(dps):
                res = integrate(mp_params(p), mp.mpc(complex(phi)), mp.mpc(0), [mp.mpc(0)] * 3, TTMS, terms, mp.mpf(tol))
                for T, r in zip(TTMS, res):
                    cf = closed_form(p, phi, T)
                    worst = max(worst, float(max(abs(x - y) / max(mp.mpf(1), abs(y))
                                                 for x, y in zip(r + [mp_log_mgf(mp_params(p), r)], cf))))
    print(f"self-check: the solver on the decoupled set vs its closed form {worst:.2e}", flush=True)
    assert worst <= 1e-16, worst


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    sets = parameter_sets()
    self_check(sets)
    names = list(sets)
    S, T = len(names), TTMS.size
    pts = [set_points(sets[n]) for n in names]
    P = pts[0][1].size
    out = dict(names=np.array(names), param_names=np.array(PARAM_NAMES),
               params=np.array([[sets[n][k] for k in PARAM_NAMES] for n in names]), ttms=TTMS, gammas=GAMMAS,
               phi_idx=PHI_IDX, n_grid_points=np.array(PHI_IDX.size), vol_scaler=np.array([v for v, _ in pts]),
               phi=np.stack([ph for _, ph in pts]))
    jobs = [(sets[n], out["phi"][s, i], TTMS, np.zeros(3)) for s, n in enumerate(names) for i in range(P)]
    cs = names.index(CHAIN_SET)
    chain_first = [(sets[CHAIN_SET], out["phi"][cs, i], CHAIN_TTMS[:1], np.zeros(3)) for i in range(P)]
    rp = np.load(os.path.join(HERE, "hawkes_risk_premia.npz"))
    g_at, t_at = np.argwhere(rp["fwd_tight_0_grid_failed"])[-1]
    assert np.array_equal(rp["param_sets"][0], out["params"][names.index("default")])
    out["giveup_gamma"], out["giveup_ttm"] = rp["gammas"][g_at], rp["grid_ttms"][t_at]
    out["giveup_phi"] = np.array(complex(-out["giveup_gamma"] - 1.0))
    giveup = [(sets["default"], ph, [out["giveup_ttm"]], np.zeros(3))
              for ph in [complex(out["giveup_phi"])] + list(out["phi"][names.index("default")])]
    with Pool(args.jobs) as pool:
        res = pool.map(solve_point, jobs, chunksize=1)
        gu = pool.map(solve_point, giveup, chunksize=1)
        first = pool.map(solve_point, chain_first, chunksize=1)
        # the second slice starts from the first's state as rounded to complex128
        second = pool.map(solve_point, [(sets[CHAIN_SET], out["phi"][cs, i], CHAIN_TTMS[1:], first[i][0][0]) for i in range(P)],
                          chunksize=1)
    out["a"] = np.array([r[0] for r in res]).reshape(S, P, T, 3).transpose(0, 2, 1, 3)
    out["log_mgf"] = np.array([r[1] for r in res]).reshape(S, P, T).transpose(0, 2, 1)
    out["agree"] = np.array([r[2] for r in res]).reshape(S, P, T).transpose(0, 2, 1)
    assert np.isnan(gu[0][2][0]), "the give-up point's solution exists"
    out["giveup_a"] = np.array([r[0][0] for r in gu[1:]])
    out["giveup_log_mgf"] = np.array([r[1][0] for r in gu[1:]])
    out["giveup_agree"] = np.array([r[2][0] for r in gu[1:]])
    assert np.max(out["giveup_agree"]) <= 1e-16
    out["chain_set"], out["chain_ttms"] = np.array(cs), CHAIN_TTMS
    out["chain_a_first"] = np.array([r[0][0] for r in first])
    out["chain_a"] = np.array([r[0][0] for r in second])
    out["chain_log_mgf"] = np.array([r[1][0] for r in second])
    out["chain_agree"] = np.array([max(r1[2][0], r2[2][0]) for r1, r2 in zip(first, second)])
    with mp.workdps(50):
        ds = names.index("decoupled")
        cf = [[closed_form(sets["decoupled"], ph, t) for ph in out["phi"][ds]] for t in TTMS]
        out["closed_a"] = np.array([[[complex(v) for v in r[:3]] for r in row] for row in cf])
        out["closed_log_mgf"] = np.array([[complex(r[3]) for r in row] for row in cf])
    out["defined"] = ~np.isnan(out["agree"])
    out["agree"] = np.where(out["defined"], out["agree"], 0.0)
    for s, n in enumerate(names):
        print(f"  {n}: worst agreement {np.max(out['agree'][s]):.2e}, poles before the ttm at "
              f"{[(float(TTMS[t]), complex(out['phi'][s, i])) for t, i in np.argwhere(~out['defined'][s])]}", flush=True)
    print(f"worst agreement {np.max(out['agree']):.2e}, chain {np.max(out['chain_agree']):.2e}", flush=True)
    assert np.max(out["agree"]) <= 1e-16 and np.max(out["chain_agree"]) <= 1e-16
    assert np.all(out["defined"][:, :T - 1]) and np.all(out["defined"][:, :, :PHI_IDX.size])
    assert all(np.all(out["defined"][names.index(n)]) for n in ("default", "asym", "decoupled"))
    path = os.path.join(HERE, "hawkes_transform_odes.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
