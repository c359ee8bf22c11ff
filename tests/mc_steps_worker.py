"""Shared by tests/golden/make_golden_mc_steps.py, tests/test_mc_steps_host.py and tests/test_gpu_mc_steps.py: the random inputs of
the cases of tests/golden/mc_steps.npz, the error measure, the asserted bound, and the runner that drives the engine through a
case in one of its forms.

As a program it is the worker of tests/test_gpu_mc_steps.py::test_full_launch_forms: the test starts it with
SVMC_FEW_WAVES_MAX_PATHS=0 (read once per process), so that the on-device-RNG launches of LogSV, Heston Euler and Heston QE run
the FULL-LAUNCH kernels at the fixture's 130 and 64 paths, and it writes the terminal states of every such case to the .npz named
on its command line:  python tests/mc_steps_worker.py OUT.npz"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import hawkes_twin as ht  # noqa: E402
from oracle import oracle  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "mc_steps.npz")
ULP = 2.0 ** -52

# The bound tests/test_gpu_mc_steps.py asserts per case and quantity: gpu_err <= max(MARGIN x oracle_err, FLOOR_ULPS x 2^-52),
# oracle_err the fixture's stored error of the fp64 oracle, per generator.  MARGIN is twice the worst gpu_err / oracle_err seen on
# the first device run among the figures whose oracle_err is at least one ulp, FLOOR_ULPS twice the worst gpu_err (in ulps) among
# the rest, where the oracle happens to round (almost) exactly and a ratio says nothing
# (profiles/mc_step_observed_tolerances.txt has the per-case figures).  tests/test_mc_steps_host.py shows that a step constant
# off by 1e-13 breaks it.
# worst ratios seen: LogSV 4.02, far states 9.21, Heston Euler 5.77, Heston QE 18.97, rough 1.84, Hawkes 1.18; worst ulps where the
# oracle's error is under one ulp: 2.92, 0.91, 2.64, 1.70, 1.27, 1.20
MARGIN = dict(logsv=8.1, far=18.5, heston=11.6, qe=38.0, rough=3.7, hawkes=2.4)
FLOOR_ULPS = dict(logsv=5.9, far=2.0, heston=5.3, qe=3.4, rough=2.6, hawkes=2.4)


def bound(oracle_err, gen):
    return np.maximum(MARGIN[gen] * np.asarray(oracle_err, dtype=np.float64), FLOOR_ULPS[gen] * ULP)


# ---- fixture --------------------------------------------------------------------------------------------------------------------
class Fixture:
    def __init__(self, path=FIXTURE):
        g = np.load(path, allow_pickle=False)
        self.meta = json.loads(str(g["meta"]))
        self.cases = self.meta["cases"]
        self.by_id = {c["id"]: c for c in self.cases}
        self.hi = g["hi"]
        self.lo = g["lo_rel"].astype(np.float64) * np.abs(self.hi)       # the truth is the double pair hi + lo
        self.fragile_bits = np.unpackbits(g["fragile"]).astype(bool)
        self.far_start = {k[len("far_start_"):]: g[k] for k in g.files if k.startswith("far_start_")}

    def truth(self, case):
        """(hi [nq][n], lo [nq][n], fragile [n])"""
        nq, n, off = case["nq"], case["n"], case["off"]
        sl = slice(off, off + nq * n)
        return self.hi[sl].reshape(nq, n), self.lo[sl].reshape(nq, n), self.fragile_bits[case["foff"]:case["foff"] + n]

    def start(self, case):
        """the start state as [3][n] arrays (generators with a state to start from)"""
        if isinstance(case["start"], str):
            return [np.array(a) for a in self.far_start[case["start"]]]
        return [np.full(case["n"], v) for v in case["start"]]

    def error(self, case, state):
        hi, lo, fragile = self.truth(case)
        return measure(np.asarray(state, dtype=np.float64), hi, lo, fragile, case["scales"])


def measure(state, hi, lo, fragile, scales):
    """|d - truth| / max(|truth|, scale) with truth = hi + lo, the largest over the non-fragile paths, per quantity"""
    keep = ~np.asarray(fragile, dtype=bool)
    with np.errstate(all="ignore"):
        diff = np.abs((state - hi) - lo)                  # d - hi is exact for d within a factor two of hi (Sterbenz)
        rel = diff / np.maximum(np.abs(hi), np.asarray(scales, dtype=np.float64)[:, None])
    rel = np.where(np.isnan(rel), np.inf, rel)            # a NaN state is an infinite error, not a skipped path
    return [float(np.max(r[keep])) for r in rel]


# ---- random inputs: the product's own stream through the oracle and the twin ----------------------------------------------------
def checksum(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()[:16]


def normals(seed, n, steps, offset, stream):
    return oracle.fill_normals(seed, n, steps, call_id=0, step_offset=offset, stream=stream)


def qe_uniforms(seed, n, steps, offset):
    """(r[step & 3] + 1/2) 2^-32 of stream 5's call step >> 2 (oracle/svmc_oracle.c svo_draw_qe), through the twin's Philox"""
    c0 = offset >> 2
    w = np.stack(ht.stream_words(seed, 0, 5, 0, n, c0, ((offset + steps - 1) >> 2) - c0 + 1))    # [4][calls][n]
    st = np.arange(offset, offset + steps)
    return ht.uniform_from_words(w[st & 3, (st >> 2) - c0, :])


def hawkes_inputs(seed, n, steps, offset):
    """the twin's draws plus the exact uniforms (v_p, v_m) behind its unit exponentials"""
    d = ht.hawkes_draws(seed, 0, 0, n, offset, steps)
    e = ht.stream_words(seed, 0, ht.HAWKES_JUMP_STREAM, 0, n, offset, steps)
    d["v_p"], d["v_m"] = ht.uniform_from_words(e[0]), ht.uniform_from_words(e[1])
    return d


STREAM = dict(logsv=0, far=0, heston=0, qe=4, rough=3)


def inputs(fx, case):
    """the random arrays of a case and their checksum as the fixture recorded it"""
    gen, n, s, off, seed = case["gen"], case["n"], case["steps"], case["offset"], case["seed"]
    if gen == "hawkes":
        d = hawkes_inputs(seed, n, s, off)
        return d, checksum(*[d[k] for k in ("z", "u_p", "u_m", "v_p", "v_m")])
    arrs = list(normals(seed, n, s, off, STREAM[gen]))
    if gen == "qe":
        arrs.append(qe_uniforms(seed, n, s, off))
    extra = fx.start(case) if gen == "far" else []
    return arrs, checksum(*arrs, *extra)


# ---- the fp64 oracles on a case ---------------------------------------------------------------------------------------------------
def oracle_state(fx, case, arrs, restatement=False, scaled=None):
    """the terminal state [nq][n] from the C oracle (or, restatement=True, the NumPy restatement / hawkes_twin); scaled = (name,
    factor): that one step constant multiplied by factor (the mutation of tests/test_mc_steps_host.py)"""
    gen, p, s, dt = case["gen"], dict(case["params"]), case["steps"], case["dt"]
    eta = case.get("eta", 1.0)
    if scaled is not None:
        name, f = scaled
        if name == "dt":
            dt = dt * f
        elif name == "eta":
            eta = eta * f
        else:
            p[name] = p[name] * f
    with np.errstate(all="ignore"):
        if gen in ("logsv", "far"):
            fn = oracle.np_logsv_terminal_w if restatement else oracle.logsv_terminal_w
            return np.stack(fn(*fx.start(case), dt, p["theta"], p["kappa1"], p["kappa2"], p["beta"], p["volvol"], arrs[0], arrs[1],
                               eta=eta, is_spot_measure=case["spot"]))
        if gen == "heston":
            fn = oracle.np_heston_terminal_w if restatement else oracle.heston_terminal_w
            return np.stack(fn(*fx.start(case), dt, p["theta"], p["kappa"], p["rho"], p["volvol"], arrs[0], arrs[1]))
        if gen == "qe":
            return np.stack(oracle.heston_qe_terminal_w(*fx.start(case), dt, p["theta"], p["kappa"], p["rho"], p["volvol"], *arrs))
        if gen == "rough":
            n, nf = case["n"], len(case["nodes"])
            nodes, weights, v0 = (np.ascontiguousarray(case[k], dtype=np.float64) for k in ("nodes", "weights", "v0"))
            ls, y, vol = np.zeros(n), np.zeros(n), np.ascontiguousarray(np.repeat(v0[:, None], n, axis=1))
            z0, z1 = np.ascontiguousarray(arrs[0]), np.ascontiguousarray(arrs[1])
            P = oracle._p
            oracle.lib().svo_rough_logsv_terminal_w(n, s, dt, nf, P(nodes), P(weights), P(v0), p["theta"], p["kappa1"], p["kappa2"],
                                                    p["rho"], p["volvol"], P(ls), P(vol), P(y), P(z0), P(z1), n)
            return np.vstack([ls[None], vol, y[None]])
        if gen == "hawkes":
            ttm = case["ttm"] * (scaled[1] if scaled is not None and scaled[0] == "dt" else 1.0)
            st = fx.start(case)
            o = ht.simulate_terminal(ttm, st[0], st[1], st[2], p, case["seed"], 0, 0, case["offset"], case["spy"] * case["ttm"] / ttm)
            assert o[3] == s
            return np.stack(o[:3])
    raise ValueError(gen)


# ---- the engine on a case ---------------------------------------------------------------------------------------------------------
FORMS = dict(logsv=("w", "rng"), far=("w", "rng"), heston=("w", "rng"), qe=("w", "rng"), rough=("w", "rng"), hawkes=("rng",))
FULL_LAUNCH_GENS = ("logsv", "far", "heston", "qe")      # the generators few_waves_launch() picks a kernel form for


def device_state(eng, fx, case, form, arrs=None):
    """drive the engine (n = case["n"] paths) through the case: form "w" on uploaded randoms, "rng" on the device draw"""
    gen, p, s, dt, off, seed = case["gen"], case["params"], case["steps"], case["dt"], case["offset"], case["seed"]
    ptrs = eng.upload_randoms(tuple(arrs)) if form == "w" else None
    if gen in ("logsv", "far"):
        eng.set_state(*fx.start(case))
        a = (s, dt, p["theta"], p["kappa1"], p["kappa2"], p["beta"], p["volvol"], case["eta"], case["spot"])
        eng.logsv_w(*a, *ptrs) if form == "w" else eng.logsv_rng(*a, seed, 0, off)
    elif gen == "heston":
        eng.set_state(*fx.start(case))
        a = (s, dt, p["theta"], p["kappa"], p["rho"], p["volvol"])
        eng.heston_w(*a, *ptrs) if form == "w" else eng.heston_rng(*a, 0, seed, 0, off)
    elif gen == "qe":
        eng.set_state(*fx.start(case))
        a = (s, dt, p["theta"], p["kappa"], p["rho"], p["volvol"])
        eng.heston_qe_w(*a, *ptrs) if form == "w" else eng.heston_rng(*a, 1, seed, 0, off)
    elif gen == "rough":
        a = (s, dt, case["nodes"], case["weights"], case["v0"], p["theta"], p["kappa1"], p["kappa2"], p["rho"], p["volvol"])
        if form == "w":
            eng.rough_logsv(*a, z0_ptr=ptrs[0], z1_ptr=ptrs[1], from_origin=True)
        else:
            eng.rough_logsv(*a, seed=seed, call_id=0, step_offset=off, from_origin=True)
        x, _, q = eng.get_state()
        return np.vstack([x[None], eng.get_factors(len(case["nodes"])), q[None]])
    elif gen == "hawkes":
        eng.set_state(*fx.start(case))
        eng.hawkesjd_rng(s, dt, np.array([p[k] for k in ht.PARAM_NAMES]), seed, 0, off)
    else:
        raise ValueError(gen)
    return np.stack(eng.get_state())


def run_forms(fx, cases_forms):
    """{(case id, form): state} for an iterable of (case, form); one engine per path count, closed at the end"""
    from stochvolmodels_amd.engine import HipEngine
    engines, out = {}, {}
    try:
        for case, form in cases_forms:
            eng = engines.get(case["n"])
            if eng is None:
                eng = engines[case["n"]] = HipEngine(case["n"])
            arrs = inputs(fx, case)[0] if form == "w" else None
            out[(case["id"], form)] = device_state(eng, fx, case, form, arrs)
    finally:
        for eng in engines.values():
            eng.close()
    return out


def main():
    assert os.environ.get("SVMC_FEW_WAVES_MAX_PATHS") == "0"
    fx = Fixture()
    states = run_forms(fx, [(c, "rng") for c in fx.cases if c["gen"] in FULL_LAUNCH_GENS])
    np.savez(sys.argv[1], **{cid: st for (cid, _), st in states.items()})
    return 0


if __name__ == "__main__":
    sys.exit(main())
