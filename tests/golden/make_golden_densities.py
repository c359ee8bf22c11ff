"""
Generate tests/golden/densities.npz, what tests/test_gpu_densities.py and tests/test_densities_host.py hold the density /
digital slice pricers, logsv_pdfs, the space grids and the device histogram to.  Runs on the CPU against the UNMODIFIED
reference (imported under the numba stand-in of tests/golden/_shims, as make_golden.py does):

    python tests/golden/make_golden_densities.py [--jobs 8] [--qvar-tight]

  slice_*   closed-form log-MGFs built here in NumPy (the lognormal transform of the reference's own
            tests/test_mgf_pricer_identities.py:22-32, :111-142, :168-181, :226-268) and the reference's digital_slice_pricer_
            with_mgf_grid / pdf_with_mgf_grid on them: negative and positive contour, the 2 001-point density, the trapezoid
            rule, an even-length grid, a NaN planted in log_mgf, and three transforms for the batch test.  Inputs AND outputs.
  heston_*  the reference's closed-form Heston log-MGF on the 1000-point phi grid and its pdf_with_mgf_grid density.
  host_*    get_init_conditions_a and the four LogSvParams space grids (bit-equal targets).
  pdf_*     logsv_pdfs of the reference with scipy.solve_ivp tightened to rtol 1e-11 / atol 1e-13 (make_golden.py
            g_analytic_tight): LOG_RETURN (TEST and BTC sets, orders 1 and 2, both measures) and SIGMA (both sets, both
            orders), ttm 0.25, get_variable_space_grid(n=200, n_stdevs=4.5).  The grid points are independent, so they are
            solved in chunks over a process pool (compute_logsv_a_mgf_grid on sub-grids, then pdf_with_mgf_grid and the
            division by `scale`: logsv_pricer.py:756-803 restated); the composition is checked bit for bit against
            logsv_pdfs itself at the default tolerance before anything is stored.
            Q_VAR (TEST set, order 2): the 40 000-point psi grid.  The first hundred points are timed at the tight tolerance;
            --qvar-tight solves all of them so, otherwise they are solved at the reference's default tolerance
            (qvar_is_tight says which; the test then compares at 5e-6 of the peak mass, as test_analytic_qvar does).  The
            reference's 40 000-point log-MGF of this one case is stored too (640 kB), so that the 40 000-term inversion can
            be tested on the reference's own transform.
  fig_*     the figure's claim (papers/logsv_model_with_quadratic_drift/article_figures.py:82-146): the CPU twin's terminal
            states of 400 000 paths on the Philox stream of FIG_SEED (oracle.logsv_terminal_rng), their
            compute_histogram_data on the three space grids, and per bin the z-score of the reference's second-order mass
            against that frequency in units of sqrt(p (1 - p) / n), p the reference's mass.  The analytic mass of the bin
            [x_(i-1), x_i] is the mean of the reference's masses at its two edges.  Bins whose expected count n p is below 5
            are left out (fig_*_keep) and may be at most 5 % of a variable's bins: the figure's own grids (n_stdevs 4.5; the
            volatility's starts at 0) do not meet that at 400 000 paths (27 % and 67 % of the bins fall short), so each
            variable's grid is the figure's narrowed to the span of the bins that do hold 5 expected paths, 200 points again
            (fig_*_space; the reference's masses on it, fig_*_mass, are re-inverted from the same tight log-MGFs), and the
            script fails if that does not converge.  All three variables are in; Q_VAR's masses come from whichever solve
            qvar_is_tight names.
  ref_seconds_*  wall-clock of the reference's own logsv_pdfs at its DEFAULT settings (x, sigma, qvar; 200 space points), one
            process, timed here while the pool works on the other cores (run with --jobs one below the core count); ref_cpu
            names the processor.
"""
import argparse
import os
import sys
import time
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "_shims"))
sys.path.insert(0, "/root/reference/src")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import stochvolmodels.pricers.heston_pricer as hp  # noqa: E402
import stochvolmodels.pricers.logsv.affine_expansion as afe  # noqa: E402
import stochvolmodels.pricers.logsv_pricer as lp  # noqa: E402
import stochvolmodels.utils.mgf_pricer as mgfp  # noqa: E402
from stochvolmodels.pricers.logsv.affine_expansion import ExpansionOrder  # noqa: E402
from stochvolmodels.pricers.logsv.logsv_params import LogSvParams  # noqa: E402
from stochvolmodels.utils.config import VariableType  # noqa: E402
from stochvolmodels.utils.funcs import compute_histogram_data  # noqa: E402

BTC = lp.LOGSV_BTC_PARAMS
TEST = LogSvParams(sigma0=0.2, theta=0.22, kappa1=3.0, kappa2=12.0, beta=-0.3, volvol=0.4)
SETS = {"test": TEST, "btc": BTC}
TTM, N_SPACE, N_STDEVS = 0.25, 200, 4.5
FIG_SEED, FIG_PATHS = 20260, 400_000
ORDERS = {1: ExpansionOrder.FIRST, 2: ExpansionOrder.SECOND}
VARS = {"x": VariableType.LOG_RETURN, "qvar": VariableType.Q_VAR, "sigma": VariableType.SIGMA}
_ORIG_SOLVE_IVP = afe.solve_ivp


def _tight(*a, **k):
    k.setdefault("rtol", 1e-11)
    k.setdefault("atol", 1e-13)
    return _ORIG_SOLVE_IVP(*a, **k)


def params_vec(p):
    return np.array([p.sigma0, p.theta, p.kappa1, p.kappa2, p.beta, p.volvol])


def pdf_pieces(p, variable_type, spot):
    """the grids, A(0), shift and scale of logsv_pdfs (logsv_pricer.py:756-795)"""
    vol_scaler = lp.set_vol_scaler(sigma0=p.sigma0, ttm=TTM)
    phi, psi, theta = mgfp.get_transform_var_grid(variable_type=variable_type, is_spot_measure=spot, vol_scaler=vol_scaler)
    if variable_type == VariableType.LOG_RETURN:
        var_grid, shift, scale = phi, 0.0, 1.0
    elif variable_type == VariableType.Q_VAR:
        var_grid, shift, scale = psi, 0.0, 1.0 / TTM
    else:
        var_grid, shift, scale = theta, p.theta, 1.0
    return phi, psi, theta, var_grid, shift, scale


def solve_chunk(job):
    """one chunk of one case's grid through the reference's compute_logsv_a_mgf_grid (a worker process)"""
    tag, vname, order, spot, lo, hi, tight = job
    afe.solve_ivp = _tight if tight else _ORIG_SOLVE_IVP
    p, variable_type = SETS[tag], VARS[vname]
    phi, psi, theta, _, _, _ = pdf_pieces(p, variable_type, spot)
    a_t0 = afe.get_init_conditions_a(phi_grid=phi, psi_grid=psi, theta_grid=theta,
                                     n_terms=afe.get_expansion_n(expansion_order=ORDERS[order]), variable_type=variable_type)
    _, log_mgf = afe.compute_logsv_a_mgf_grid(ttm=TTM, phi_grid=phi[lo:hi], psi_grid=psi[lo:hi], theta_grid=theta[lo:hi],
                                              a_t0=a_t0[lo:hi], is_analytic=False, expansion_order=ORDERS[order],
                                              is_stiff_solver=False, is_spot_measure=spot, **p.to_dict())
    return job, log_mgf


def chunked_log_mgfs(pool, cases, chunk, meanwhile=None):
    """{case: log_mgf over the whole grid}; cases = [(tag, vname, order, spot, tight)]; meanwhile() runs in this process once
    the jobs are with the pool"""
    jobs = []
    for tag, vname, order, spot, tight in cases:
        n = pdf_pieces(SETS[tag], VARS[vname], spot)[3].size
        jobs += [(tag, vname, order, spot, lo, min(lo + chunk, n), tight) for lo in range(0, n, chunk)]
    # longest grids first: the pool's tail is then made of short jobs
    parts = {}
    results = pool.imap_unordered(solve_chunk, jobs, chunksize=1)
    if meanwhile is not None:
        meanwhile()
    for job, lm in results:
        parts.setdefault(job[:4] + (job[6],), {})[job[4]] = lm
    return {case: np.concatenate([parts[case][lo] for lo in sorted(parts[case])]) for case in parts}


def invert(p, variable_type, spot, log_mgf, space):
    """logsv_pricer.py:797-803"""
    _, _, _, var_grid, shift, scale = pdf_pieces(p, variable_type, spot)
    pdf = mgfp.pdf_with_mgf_grid(log_mgf_grid=log_mgf, transform_var_grid=var_grid, space_grid=space, shift=shift, scale=scale)
    return pdf / scale


def space_grid(p, variable_type):
    return p.get_variable_space_grid(variable_type=variable_type, ttm=TTM, n=N_SPACE, n_stdevs=N_STDEVS)


def lognormal(ttm=0.5, vol=0.3, spot=True, n=2001):
    phi = mgfp.get_phi_grid(is_spot_measure=spot, max_phi=n, vol_scaler=vol * np.sqrt(ttm))
    return phi, 0.5 * (vol * vol * ttm) * (phi + phi * phi)


def g_slices(out):
    forward, df = 1.2, 0.97
    phi, lm = lognormal()
    out.update(slice_phi=phi, slice_log_mgf=lm, slice_forward=forward, slice_discfactor=df)
    k4 = np.array([0.9, 1.1, 1.3, 1.5])
    out["slice_dig_strikes"] = k4
    out["slice_dig_calls"] = mgfp.digital_slice_pricer_with_mgf_grid(lm, phi, forward, k4, np.full(4, "C"), df)
    out["slice_dig_puts"] = mgfp.digital_slice_pricer_with_mgf_grid(lm, phi, forward, k4, np.full(4, "P"), df)
    out["slice_dig_calls_trapz"] = mgfp.digital_slice_pricer_with_mgf_grid(lm, phi, forward, k4, np.full(4, "C"), df,
                                                                           is_simpson=False)
    phi_p, lm_p = lognormal(spot=False)
    k3, t3 = np.array([0.9, 1.1, 1.3]), np.array(["P", "C", "C"])
    out.update(slice_pos_phi=phi_p, slice_pos_log_mgf=lm_p, slice_pos_strikes=k3, slice_pos_types=t3)
    out["slice_pos_digitals"] = mgfp.digital_slice_pricer_with_mgf_grid(lm_p, phi_p, forward, k3, t3, df)
    space = np.linspace(-1.5, 1.2, 2001)
    out["slice_space"] = space
    out["slice_pdf"] = mgfp.pdf_with_mgf_grid(lm, phi, space)
    out["slice_pdf_trapz"] = mgfp.pdf_with_mgf_grid(lm, phi, space, is_simpson=False)
    out["slice_pdf_shift_scale"] = mgfp.pdf_with_mgf_grid(lm, phi, space, shift=0.03, scale=1.25)
    phi_e, lm_e = lognormal(n=2000)                                        # even length: the last odd index keeps weight 4
    out.update(slice_even_phi=phi_e, slice_even_log_mgf=lm_e)
    out["slice_even_pdf"] = mgfp.pdf_with_mgf_grid(lm_e, phi_e, space)
    out["slice_even_dig_calls"] = mgfp.digital_slice_pricer_with_mgf_grid(lm_e, phi_e, forward, k4, np.full(4, "C"), df)
    lm_nan = lm.copy()
    lm_nan[[7, 400]] = np.nan + 1j * np.nan
    out["slice_nan_idx"] = np.array([7, 400])
    out["slice_nan_pdf"] = mgfp.pdf_with_mgf_grid(lm_nan, phi, space)
    out["slice_nan_dig_calls"] = mgfp.digital_slice_pricer_with_mgf_grid(lm_nan, phi, forward, k4, np.full(4, "C"), df)
    # three transforms on one grid for the batch test: lognormal at three vols
    vols = np.array([0.2, 0.3, 0.45])
    out["slice_batch_vols"] = vols
    out["slice_batch_pdf"] = np.stack([mgfp.pdf_with_mgf_grid(0.5 * (v * v * 0.5) * (phi + phi * phi), phi, space) for v in vols])
    # Heston: the reference's closed form on the pricer's phi grid
    h = hp.HestonParams(v0=0.04, theta=0.05, kappa=3.0, rho=-0.6, volvol=0.5)
    hphi = mgfp.get_phi_grid(vol_scaler=float(np.minimum(0.3, np.sqrt(h.v0 * 0.5))))
    hlm = hp.compute_heston_mgf_grid(v0=h.v0, theta=h.theta, kappa=h.kappa, volvol=h.volvol, rho=h.rho, ttm=0.5, phi_grid=hphi,
                                     psi_grid=np.zeros_like(hphi))[0]
    hspace = np.linspace(-0.9, 0.6, 200)
    out.update(heston_params=np.array([h.v0, h.theta, h.kappa, h.rho, h.volvol]), heston_ttm=0.5, heston_phi=hphi,
               heston_log_mgf=hlm, heston_space=hspace, heston_pdf=mgfp.pdf_with_mgf_grid(hlm, hphi, hspace),
               heston_dig_strikes=k3, heston_dig_calls=mgfp.digital_slice_pricer_with_mgf_grid(hlm, hphi, 1.0, k3, np.full(3, "C")))


def g_host(out):
    for tag, p in SETS.items():
        out[f"{tag}_params"] = params_vec(p)
        out[f"host_{tag}_x_grid"] = p.get_x_grid(ttm=0.7, n_stdevs=3.0, n=57)
        out[f"host_{tag}_sigma_grid"] = p.get_sigma_grid(ttm=0.7, n_stdevs=3.0, n=57)
        out[f"host_{tag}_qvar_grid"] = p.get_qvar_grid(ttm=0.7, n_stdevs=3.0, n=57)
        out[f"host_{tag}_x_grid_default"] = p.get_x_grid()
        out[f"host_{tag}_sigma_grid_default"] = p.get_sigma_grid()
        out[f"host_{tag}_qvar_grid_default"] = p.get_qvar_grid()
        for vname, vt in VARS.items():
            out[f"space_{tag}_{vname}"] = space_grid(p, vt)
    phi = -0.5 + 1j * np.linspace(0.0, 9.0, 7)
    psi = -0.5 + 1j * np.linspace(0.0, 11.0, 9)
    theta = 0.0 + 1j * np.linspace(0.0, 13.0, 11)
    out.update(host_init_phi=phi, host_init_psi=psi, host_init_theta=theta)
    for vname, vt in VARS.items():
        for n in (3, 5):
            out[f"host_init_{vname}_{n}"] = afe.get_init_conditions_a(phi_grid=phi, psi_grid=psi, theta_grid=theta, n_terms=n,
                                                                      variable_type=vt)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or platform.machine()


def g_reference_timings(out):
    """the reference as shipped (default RK45), one process, one call per variable; run while the pool solves on the other cores"""
    afe.solve_ivp = _ORIG_SOLVE_IVP
    for vname in ("x", "sigma", "qvar"):
        t0 = time.perf_counter()
        pdf = lp.logsv_pdfs(params=TEST, ttm=TTM, space_grid=space_grid(TEST, VARS[vname]), variable_type=VARS[vname])
        out[f"ref_seconds_{vname}"] = time.perf_counter() - t0
        out[f"pdf_default_test_{vname}_2_spot"] = pdf
        print(f"reference logsv_pdfs {vname}: {out[f'ref_seconds_{vname}']:.1f} s", flush=True)
    out["ref_cpu"] = np.array(cpu_model())


def g_figure(out, lms):
    from oracle import oracle
    p = TEST
    nb_steps, dt = oracle.set_time_grid(TTM, 360)
    x, s, q = oracle.logsv_terminal_rng(np.zeros(FIG_PATHS), np.full(FIG_PATHS, p.sigma0), np.zeros(FIG_PATHS), nb_steps, dt,
                                        p.theta, p.kappa1, p.kappa2, p.beta, p.volvol, FIG_SEED)
    out.update(fig_seed=FIG_SEED, fig_paths=FIG_PATHS)
    datas = {"x": x, "qvar": q / TTM, "sigma": s}
    for vname, lm in lms.items():
        # the chosen grid: start from the figure's (n_stdevs 4.5) and narrow it to the span of the bins that are expected to
        # hold 5 paths under the reference's masses, 200 points again, until at most 5 % of the bins fall short
        grid = space_grid(p, VARS[vname])
        for _ in range(6):
            m = invert(p, VARS[vname], True, lm, grid)
            pb = 0.5 * (m[:-1] + m[1:])                                   # the reference's mass of bin [x_(i-1), x_i]
            keep = FIG_PATHS * pb >= 5.0
            left_out = 1.0 - np.count_nonzero(keep) / keep.size
            print(f"figure {vname}: grid [{grid[0]:.4f}, {grid[-1]:.4f}], {left_out:.1%} of the bins expect fewer than 5 paths", flush=True)
            if left_out <= 0.05:
                break
            idx = np.flatnonzero(keep)
            grid = np.linspace(grid[idx[0]], grid[idx[-1] + 1], N_SPACE)
        else:
            raise SystemExit(f"figure fixture {vname}: no grid keeps 95 % of its bins at an expected count of 5")
        hist = compute_histogram_data(data=datas[vname], x_grid=grid).to_numpy()
        se = np.sqrt(np.where(keep, pb * (1.0 - pb), 1.0) / FIG_PATHS)
        z = np.where(keep, (pb - hist[1:]) / se, 0.0)
        out[f"fig_{vname}_space"], out[f"fig_{vname}_mass"] = grid, m
        out[f"fig_{vname}_hist"], out[f"fig_{vname}_keep"], out[f"fig_{vname}_z_ref"] = hist, keep, z
        print(f"figure {vname}: {np.count_nonzero(~keep)} of {keep.size} bins left out, max |z_ref| {np.abs(z).max():.2f}, "
              f"L1(mass, frequency) {np.abs(pb - hist[1:]).sum():.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--qvar-tight", action="store_true")
    ap.add_argument("--skip-timings", action="store_true")
    ap.add_argument("--cache", help="keep the solved log-MGFs in this .npz and reuse them on the next run")
    args = ap.parse_args()
    out = {}
    g_slices(out)
    g_host(out)
    print("slices, host done", flush=True)
    with Pool(args.jobs) as pool:
        # the chunked composition against logsv_pdfs itself, default tolerance
        case = ("test", "x", 2, True, False)
        lm = chunked_log_mgfs(pool, [case], 125)[case]
        direct = lp.logsv_pdfs(params=TEST, ttm=TTM, space_grid=space_grid(TEST, VARS["x"]))
        assert np.array_equal(invert(TEST, VARS["x"], True, lm, space_grid(TEST, VARS["x"])), direct), "composition differs"
        print("chunked composition == logsv_pdfs, bit for bit", flush=True)
        # Q_VAR: the first hundred points, tight, timed
        t0 = time.perf_counter()
        solve_chunk(("test", "qvar", 2, True, 0, 100, True))
        afe.solve_ivp = _ORIG_SOLVE_IVP
        per_point = (time.perf_counter() - t0) / 100
        out["qvar_tight_seconds_first_100"] = per_point * 100
        print(f"Q_VAR tight: {per_point * 1e3:.1f} ms a point over the first hundred -> {per_point * 40000 / args.jobs / 60:.1f} min "
              f"on {args.jobs} processes if the rest cost the same", flush=True)
        cases = [(tag, "sigma", order, True, True) for tag in SETS for order in (1, 2)]
        cases += [(tag, "x", order, spot, True) for tag in SETS for order in (1, 2) for spot in (True, False)]
        cases.append(("test", "qvar", 2, True, bool(args.qvar_tight)))
        out["qvar_is_tight"] = bool(args.qvar_tight)
        t0 = time.perf_counter()
        key = lambda case: "|".join(map(str, case))                      # noqa: E731
        lms, timings = {}, {}
        if args.cache and os.path.exists(args.cache):
            with np.load(args.cache) as c:
                lms = {case: c[key(case)] for case in cases if key(case) in c.files}
        if args.cache and os.path.exists(args.cache + ".timings.npz"):
            with np.load(args.cache + ".timings.npz") as c:
                timings = {k: c[k] for k in c.files}

        def timed():
            if not timings and not args.skip_timings:
                g_reference_timings(timings)
                if args.cache:
                    np.savez(args.cache + ".timings.npz", **timings)

        missing = [case for case in cases if case not in lms]
        if missing:
            lms.update(chunked_log_mgfs(pool, missing, 100, meanwhile=timed))
            if args.cache:
                np.savez(args.cache, **{key(case): lm for case, lm in lms.items()})
        else:
            timed()
        out.update(timings)
        lms = {case: lms[case] for case in cases}
        print(f"all grids solved in {time.perf_counter() - t0:.0f} s", flush=True)
    fig_lms = {}
    for (tag, vname, order, spot, _), lm in lms.items():
        p = SETS[tag]
        pdf = invert(p, VARS[vname], spot, lm, space_grid(p, VARS[vname]))
        out[f"pdf_{tag}_{vname}_{order}_{'spot' if spot else 'inv'}"] = pdf
        if tag == "test" and order == 2 and spot:
            fig_lms[vname] = lm
        if vname == "qvar":
            out["qvar_log_mgf"] = lm
        print(f"pdf {tag} {vname} order {order} {'spot' if spot else 'inv'}: sum {pdf.sum():.9f}", flush=True)
    g_figure(out, fig_lms)
    path = os.path.join(HERE, "densities.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"densities.npz {size / 1024:.1f} KiB")
    assert size < 1024 * 1024, "over the size limit for a committed file"


if __name__ == "__main__":
    main()
