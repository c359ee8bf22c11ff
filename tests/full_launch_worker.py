"""worker of tests/test_gpu_parity.py::test_full_launch_chain_kernels_equal_slices_and_many_job_batch: the test starts it with
SVMC_FEW_WAVES_MAX_PATHS=0 (read once per process), so every on-device-RNG launch here runs the FULL-LAUNCH kernels.  At 1089 paths
-- one full 1024-thread block, one full wave and one lane: a partial block, a partial wave and idle waves -- it prices a 3-expiry
chain with ragged step counts by whole-chain stepping, slice by slice and as job 0 of a 2-job batch, and compares bit for bit:
prices, standard errors and (the first two) the terminal state.  Prints one JSON line {case: {check: bool}}; exit status 1 if any
check is false."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import stochvolmodels_amd as sv  # noqa: E402
from stochvolmodels_amd.engine import get_engine  # noqa: E402
from stochvolmodels_amd.pricers import heston_pricer as hp  # noqa: E402
from stochvolmodels_amd.pricers import logsv_pricer as lp  # noqa: E402

N = 1089
TTMS = np.array([0.11, 0.3, 0.57])                    # 120 steps per year: 14, 23 and 33 steps
FW = np.array([1.0, 1.02, 0.97])
CHAIN = dict(ttms=TTMS, forwards=FW, discfactors=np.full(3, 0.99), nb_path=N, nb_steps_per_year=120)
# the QE sets of test_heston_qe_branches_the_parameters_decide: the first leaves the quadratic branch (the general kernel), the
# second and third never do and have rho <= 0 (a batch of those two runs the kernels compiled without the exponential branch)
QE_GENERAL = dict(v0=0.02, theta=0.02, kappa=1.0, rho=-0.7, volvol=1.0)
QE_QUAD = dict(v0=0.5, theta=0.6, kappa=3.0, rho=0.0, volvol=1.2)
QE_QUAD_OTHER = dict(v0=0.04, theta=0.05, kappa=2.0, rho=-0.3, volvol=1e-5)


def same(a, b):
    return bool(all(np.array_equal(u, v) for u, v in zip(a, b)) and len(a) == len(b))


def compare(module, single, many):
    """single(): the chain through the single-job pricer; many(): the 2-job batch whose job 0 is that chain"""
    out = {}
    for flag in (True, False):
        module.WHOLE_CHAIN_STEPPING = flag
        try:
            pr, sd = single()
        finally:
            module.WHOLE_CHAIN_STEPPING = True
        out[flag] = (pr, sd, get_engine(N).get_state())
    bpr, bsd = many()[0]
    return {"chain_eq_slices_prices": same(out[True][0], out[False][0]), "chain_eq_slices_stderrs": same(out[True][1], out[False][1]),
            "chain_eq_slices_state": same(out[True][2], out[False][2]), "many_eq_chain_prices": same(bpr, out[True][0]),
            "many_eq_chain_stderrs": same(bsd, out[True][1]),
            "finite": bool(all(np.all(np.isfinite(a)) for a in list(out[True][0]) + list(out[True][1])))}


def logsv_case(spot):
    p = sv.LOGSV_BTC_PARAMS
    other = sv.LogSvParams(sigma0=1.1 * p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2 + 0.2, beta=p.beta, volvol=0.9 * p.volvol)
    ty = np.array(["P", "C", "C"]) if spot else np.array(["IP", "IC", "IC"])
    kw = dict(CHAIN, strikes_ttms=[f * np.array([0.8, 1.0, 1.2]) for f in FW], optiontypes_ttms=[ty] * 3, is_spot_measure=spot)
    return compare(lp,
                   lambda: sv.logsv_mc_chain_pricer(v0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2, beta=p.beta, volvol=p.volvol,
                                                    vol_backbone_etas=np.ones(3), seed=99, **kw),
                   lambda: sv.logsv_mc_chain_pricer_many([p, other], seeds=[99, 7], **kw))


def heston_case(scheme, par, other):
    kw = dict(CHAIN, strikes_ttms=[f * np.array([0.8, 1.0, 1.2]) for f in FW], optiontypes_ttms=[np.array(["IP", "C", "IC"])] * 3, scheme=scheme)
    return compare(hp, lambda: sv.heston_mc_chain_pricer(seed=5, **par, **kw),
                   lambda: sv.heston_mc_chain_pricer_many([sv.HestonParams(**par), sv.HestonParams(**other)], seeds=[5, 6], **kw))


def main():
    assert os.environ.get("SVMC_FEW_WAVES_MAX_PATHS") == "0"
    out = {"logsv_spot_measure": logsv_case(True), "logsv_inverse_measure": logsv_case(False),
           "heston_euler": heston_case("euler", dict(v0=0.05, theta=0.04, kappa=3.0, rho=-0.6, volvol=0.7), QE_QUAD),
           "heston_qe_general": heston_case("qe", QE_GENERAL, QE_QUAD), "heston_qe_quad_only": heston_case("qe", QE_QUAD, QE_QUAD_OTHER)}
    print(json.dumps(out))
    return 0 if all(all(c.values()) for c in out.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
