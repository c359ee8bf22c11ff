"""
Times of the exponentially weighted payoff reduction on the GPU -> profiles/hawkes_tilted_bench.json:

  * the two chains -- the paper's slice (one expiry, 20 strikes) and the 49-option BTC chain of tests/golden/hawkes_analytic.npz --
    at 10^5 and 2^20 resident paths under 1, 2 and 5 gammas: svmc_tilted_payoff_chain's launches alone (queued on resident
    snapshots and results, then one synchronise) and HipEngine.tilted_payoffs (host preparation and the download included);
  * (a) on the same box and the same snapshots: svmc_payoff_sums_chain, the plain measure's launch pair, the same way;
  * (b) the script's way on the same box: the download of one expiry's x, then the NumPy loop over the strikes
    (nanmean(exp(gamma x) payoff) / mean(exp(gamma x))) on one host core, for one and for two gammas;
  * the whole pricer call, hawkesjd_mc_chain_pricer_with_risk_premia_gammas, at the reference's 1 800 steps per year.

Host clocks around work that ends in a synchronise; medians of --repeats runs after a warm-up.  The shader clock of the box is
read by the in-kernel probe of a LogSV stepping launch, as the other profiles note it.

    python tools/bench_tilted.py [--repeats 10] [--out profiles/hawkes_tilted_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import stochvolmodels_amd as sv  # noqa: E402
from stochvolmodels_amd import _lib  # noqa: E402
from stochvolmodels_amd.engine import DeviceBuffer, get_engine, payoff_shifts, tilted_type_codes  # noqa: E402
from stochvolmodels_amd.pricers import hawkes_jd_pricer as hp  # noqa: E402

GAMMA_SETS = ([1.0], [1.0, -1.0], [-3.0, -1.0, 0.0, 0.5, 3.0])


def median_ms(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def chains():
    k = np.linspace(0.5, 1.5, 20)
    paper = dict(ttms=np.array([1.0 / 12.0]), forwards=np.array([1.0]), strikes=[k], types=[np.where(k <= 1.0, "P", "C")])
    f = np.load(os.path.join(ROOT, "tests", "golden", "hawkes_analytic.npz"), allow_pickle=False)
    m = f["ttms"].size
    btc = dict(ttms=f["ttms"], forwards=f["forwards"], strikes=[f[f"strikes_{i}"] for i in range(m)],
               types=[f[f"types_{i}"] for i in range(m)])
    return {"paper_slice_20": paper, "btc_chain_49": btc}


def box_clock_mhz():
    """the shader clock during a LogSV stepping launch (svmc_clock_probe_*), None where the probe gives nothing"""
    L = _lib.load()
    P = sv.LOGSV_BTC_PARAMS
    try:
        _lib.check(L.svmc_clock_probe_arm(1))
        n = 1 << 18
        sv.logsv_mc_chain_pricer(ttms=np.array([0.25]), forwards=np.array([1.0]), discfactors=np.array([1.0]),
                                 strikes_ttms=(np.array([1.0]),), optiontypes_ttms=(np.array(["C"]),), v0=P.sigma0, theta=P.theta,
                                 kappa1=P.kappa1, kappa2=P.kappa2, beta=P.beta, volvol=P.volvol, vol_backbone_etas=np.ones(1),
                                 nb_path=n, nb_steps_per_year=3600, seed=1)
        st = (C.c_uint64 * 8)()
        _lib.check(L.svmc_clock_probe_read(st, get_engine(n).stream))
        dt, dr = st[2] - st[0], st[3] - st[1]
        return round(dt / dr * 100.0, 1) if dr > 0 else None
    except Exception:
        return None
    finally:
        L.svmc_clock_probe_arm(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--paths", type=int, nargs="*", default=[100_000, 1 << 20])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hawkes_tilted_bench.json"))
    args = ap.parse_args()
    L = _lib.load()
    dp, pi8, psz = C.POINTER(C.c_double), C.POINTER(C.c_int8), C.POINTER(C.c_size_t)
    out = {"repeats": args.repeats, "kernel_clock_mhz": box_clock_mhz(), "device_runs": [], "script_way_same_box": [], "pricer_calls": []}
    rng = np.random.default_rng(1)
    for n in args.paths:
        eng = get_engine(n)
        for name, ch in chains().items():
            m = ch["ttms"].size
            eng.reserve_snapshots(m)
            for i, t in enumerate(ch["ttms"]):
                eng.upload(eng.snapshot_ptr(i), 0.6 * np.sqrt(t) * rng.standard_normal(n) - 0.18 * t)
            codes = [tilted_type_codes(t) for t in ch["types"]]
            fw = np.ascontiguousarray(ch["forwards"], dtype=np.float64)
            tt = np.ascontiguousarray(ch["ttms"], dtype=np.float64)
            k_all = np.ascontiguousarray(np.concatenate(ch["strikes"]))
            c_all = np.ascontiguousarray(np.concatenate(codes))
            s_all = np.ascontiguousarray(np.concatenate([payoff_shifts(k, c, float(f), 1) for k, c, f in zip(ch["strikes"], codes, fw)]))
            offs = np.concatenate([[0], np.cumsum([k.size for k in ch["strikes"]])]).astype(np.uintp)
            K = k_all.size
            xs = (C.c_void_p * m)(*[eng.snapshot_ptr(i) for i in range(m)])
            spot = DeviceBuffer(2 * m)
            for i in range(m):
                eng.spot_sums(eng.snapshot_ptr(i), float(fw[i]), spot.offset(2 * i))
            res = DeviceBuffer(5 * (2 * K + 8 * m) + 3 * K)

            def plain():
                _lib.check(L.svmc_payoff_sums_chain(xs, None, n, fw.ctypes.data_as(dp), tt.ctypes.data_as(dp), spot.ptr, m,
                                                    k_all.ctypes.data_as(dp), c_all.ctypes.data_as(pi8), s_all.ctypes.data_as(dp),
                                                    offs.ctypes.data_as(psz), 1, res.ptr, eng.ws.ptr, eng.ws_bytes, eng.stream))
                eng.synchronize()

            plain_ms = median_ms(plain, args.repeats)
            for gammas in GAMMA_SETS:
                g = np.array(gammas)
                G = g.size

                def tilted():
                    _lib.check(L.svmc_tilted_payoff_chain(xs, n, fw.ctypes.data_as(dp), m, k_all.ctypes.data_as(dp),
                                                          c_all.ctypes.data_as(pi8), s_all.ctypes.data_as(dp), offs.ctypes.data_as(psz),
                                                          g.ctypes.data_as(dp), G, 1, spot.ptr, res.ptr, res.offset(G * K),
                                                          res.offset(2 * G * K), eng.ws.ptr, eng.ws_bytes, eng.stream))
                    eng.synchronize()

                launches = median_ms(tilted, args.repeats)
                whole = median_ms(lambda: eng.tilted_payoffs(fw, ch["strikes"], codes, g, True, snap_rows=range(m)), args.repeats)
                row = {"chain": name, "n_path": n, "n_gammas": G, "tilted_launches_ms": launches, "engine_tilted_payoffs_ms": whole,
                       "plain_payoff_launches_ms": plain_ms, "tilted_over_plain_per_gamma": launches / plain_ms / G}
                print(json.dumps(row), flush=True)
                out["device_runs"].append(row)
            spot.free()
            res.free()
        # (b) the script's way, on the paper's slice
        ch = chains()["paper_slice_20"]
        eng.reserve_snapshots(1)
        k, types = ch["strikes"][0], ch["types"][0]

        def script(gammas):
            x = eng.download(eng.snapshot_ptr(0), n)
            for gamma in gammas:
                risk = np.exp(gamma * x)
                spots = np.exp(x)
                for strike, ty in zip(k, types):
                    pay = np.maximum(spots - strike, 0.0) if ty == "C" else np.maximum(strike - spots, 0.0)
                    np.nanmean(risk * pay) / np.mean(risk)

        row = {"n_path": n, "download_x_ms": median_ms(lambda: eng.download(eng.snapshot_ptr(0), n), args.repeats),
               "download_and_numpy_one_gamma_ms": median_ms(lambda: script([1.0]), args.repeats),
               "download_and_numpy_two_gammas_ms": median_ms(lambda: script([1.0, -1.0]), args.repeats)}
        print(json.dumps(row), flush=True)
        out["script_way_same_box"].append(row)
        # the whole pricer call at the reference's step count
        kw = hp.HawkesJDParams().to_dict()
        kw.pop("risk_premia_gamma")
        chain = dict(ttms=ch["ttms"], forwards=ch["forwards"], discfactors=np.ones(1), strikes_ttms=ch["strikes"], optiontypes_ttms=ch["types"])
        for gammas in GAMMA_SETS:
            ms = median_ms(lambda: hp.hawkesjd_mc_chain_pricer_with_risk_premia_gammas(risk_premia_gammas=gammas, nb_path=n, seed=1,
                                                                                        **chain, **kw), args.repeats)
            plain_ms = median_ms(lambda: hp.hawkesjd_mc_chain_pricer(nb_path=n, seed=1, **chain, **kw), args.repeats)
            row = {"chain": "paper_slice_20", "n_path": n, "n_gammas": len(gammas), "nb_steps_per_year": hp.NB_STEPS_PER_YEAR,
                   "tilted_pricer_call_ms": ms, "plain_pricer_call_ms": plain_ms}
            print(json.dumps(row), flush=True)
            out["pricer_calls"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
