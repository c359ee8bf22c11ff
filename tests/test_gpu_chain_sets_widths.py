"""
Every width of the multi-set LogSV stepping kernels -- logsv_chain_w_sets_kernel<P> on resident randoms, P = 2..8, and
logsv_chain_rng_sets_kernel<P> on randoms regenerated in registers, P = 1..7, eight sets as two launches of four -- held to the
single-set route BIT FOR BIT, per set: prices, standard errors and implied vols.

The oracle is the single-set route: logsv_mc_chain_pricer_fixed_randoms on the same resident randoms, and on the frozen route
logsv_mc_chain_pricer(seed=...) for prices and standard errors and the single-set call on the frozen object for the implied vols
(the graph's last kernel on those prices).

  * widths 1..9, 15 (a launch of eight and one of seven) and 16, on both routes; set q differs from the others in all six model
    parameters and every second set carries a vol backbone;
  * path counts 1, 63, 64, 65, 255, 256, 257 and 4133 at the widths that select distinct code (1, 4, 5, 6, 7, 8: the single-set
    route, the pipelined loop without and with parking, the two-piece loop, the launch with s0 = 4), 257 and 4133 at the others:
    a single wave, a block less one, an exact block, a block and one, many blocks with a ragged tail;
  * chains (CHAINS; the step counts are asserted with time_grid_steps): one one-step slice; one-step, two-step, odd and even
    slices in that order, so that a slice boundary falls on either half of a Philox pair; 1, 2, 16 and 17 expiries.  Past sixteen
    expiries the resident route prices the sets one after the other through the single-set entry (the same bits) and the frozen
    route refuses (svmc_logsv_chain_price_frozen_sets: "at most 16 expiries");
  * both measures, LOG_RETURN with inverse payoff codes in the chain, Q_VAR;
  * company: set q alone, in slot 0 and slot 6 of a seven-set call and in slot 5 of an eight-set call gives the same bits;
  * sharding, frozen route: the snapshot rows of a 513-path call are the rows of the sessions at path_offset 0, 64 and 194 side by
    side, at width 7 and 8;
  * capture, replay and graphs off at width 5 and 7.

WIDTH_GRID is plain data: tests/test_chain_sets_widths_host.py checks, without a device, that it launches every instantiation
of the two families that tests/golden/libsvmc_kernel_names.json lists.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# ---- plain data (imported by tests/test_chain_sets_widths_host.py) -------------------------------------------------------------
MAX_SETS_PER_LAUNCH = 8
WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16)
EDGE_WIDTHS = (1, 4, 5, 6, 7, 8)                      # the widths that select distinct code
EDGE_PATHS = (1, 63, 64, 65, 255, 256, 257, 4133)     # BLOCK = 256, a wave = 64
BASE_PATHS = (257, 4133)
ROUTES = ("resident", "frozen")
WIDTH_GRID = [(route, w, n) for route in ROUTES for w in WIDTHS for n in (EDGE_PATHS if w in EDGE_WIDTHS else BASE_PATHS)]


def launches_of(route, width):
    """the stepping kernels a call of `width` sets runs, as (family, P): the Python route cuts the list into calls of eight sets;
    one set on resident randoms goes to the single-set (indirect) kernel, eight frozen sets to two launches of <4>"""
    out = []
    for q0 in range(0, width, MAX_SETS_PER_LAUNCH):
        p = min(MAX_SETS_PER_LAUNCH, width - q0)
        if route == "resident":
            out.append(("logsv_chain_w_indirect_kernel", 1) if p == 1 else ("logsv_chain_w_sets_kernel", p))
        else:
            out += [("logsv_chain_rng_sets_kernel", 4)] * 2 if p == 8 else [("logsv_chain_rng_sets_kernel", p)]
    return out


SPY = 360
# ttms and the step counts they give at SPY steps per year (expiry i: int((T_i - T_{i-1}) SPY) + 1 steps)
CHAINS = {
    "one_step": dict(ttms=(0.002,), steps=(1,)),                                        # 0.72 -> 1
    "mixed": dict(ttms=(0.002, 0.006, 0.024, 0.056), steps=(1, 2, 7, 12)),              # 0.72, 1.44, 6.48, 11.52
    "m1": dict(ttms=(0.06,), steps=(22,)),                                              # 21.6
    "m2": dict(ttms=(0.03, 0.1), steps=(11, 26)),                                       # 10.8, 25.2
    "m16": dict(ttms=tuple(0.0075 * k for k in range(1, 17)), steps=(3,) * 16),         # 2.7 each
    "m17": dict(ttms=tuple(0.0075 * k for k in range(1, 18)), steps=(3,) * 17),
}
MAX_CHAIN_SLICES = 16
SEED_FROZEN, SEED_RESIDENT = 77, 5
LOG_RETURN, INVERSE_CODES, Q_VAR = "log_return", "inverse_codes", "q_var"


# ---- the device side ---------------------------------------------------------------------------------------------------------------
def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


class Context:
    """the chains, parameter sets, randoms and single-set results of this file, each made once"""

    def __init__(self, sv):
        self.sv = sv
        self._randoms, self._single, self._chains = {}, {}, {}

    def chain(self, name, variant=LOG_RETURN):
        """the chain's arrays; its step counts are asserted on the product's own grid rule"""
        key = (name, variant)
        if key not in self._chains:
            from stochvolmodels_amd.utils.funcs import time_grid_steps
            c = CHAINS[name]
            ttms = np.array(c["ttms"])
            t0, steps = 0.0, []
            for t in ttms:
                steps.append(time_grid_steps(float(t) - t0, SPY)[0])
                t0 = float(t)
            assert tuple(steps) == c["steps"], (name, steps)
            m = ttms.size
            fw = 1.0 + 0.01 * np.arange(m)
            rel = np.linspace(0.94, 1.06, 5)
            ks = tuple(f * rel for f in fw)
            j = np.arange(rel.size)
            if variant == INVERSE_CODES:
                tys = tuple(np.where(k >= f, np.where(j % 2 == 0, "IC", "C"), np.where(j % 3 == 0, "IP", "P")) for k, f in zip(ks, fw))
            else:
                tys = tuple(np.where(k >= f, "C", "P") for k, f in zip(ks, fw))
            if variant == Q_VAR:
                ks = tuple(np.array([0.5, 1.0, 1.6]) * 0.7 * t for t in ttms)                 # around sigma^2 T
                tys = (np.array(["C", "P", "C"]),) * m
            self._chains[key] = dict(ttms=ttms, forwards=fw, discfactors=np.exp(-0.03 * ttms), strikes_ttms=ks, optiontypes_ttms=tys)
        return self._chains[key]

    def sets(self, name, count=16):
        """set j differs from every other in all six model parameters; the odd ones carry a vol backbone"""
        import pandas as pd
        ttms = np.array(CHAINS[name]["ttms"])
        rng = np.random.default_rng(9)
        out = []
        for j in range(count):
            bb = None if j % 2 == 0 else pd.Series(1.0 + 0.1 * rng.standard_normal(ttms.size), index=ttms)
            out.append(self.sv.LogSvParams(sigma0=0.8 + 0.02 * j, theta=1.0 + 0.01 * j, kappa1=3.0 + 0.1 * j, kappa2=3.0 - 0.1 * j,
                                           beta=0.15 - 0.03 * j, volvol=1.8 - 0.05 * j, vol_backbone=bb))
        return out

    def randoms(self, route, name, n):
        key = (route, name, n)
        if key not in self._randoms:
            ttms = np.array(CHAINS[name]["ttms"])
            if route == "resident":
                W = self.sv.get_randoms_for_chain_valuation(ttms, nb_path=n, nb_steps_per_year=SPY, seed=SEED_RESIDENT)
                self._randoms[key] = self.sv.upload_fixed_randoms(*W)
            else:
                self._randoms[key] = self.sv.draw_fixed_randoms_on_device(ttms, nb_path=n, nb_steps_per_year=SPY, seed=SEED_FROZEN)
            assert tuple(self._randoms[key].nb_steps) == CHAINS[name]["steps"]
        return self._randoms[key]

    @staticmethod
    def vt(sv, variant):
        return sv.VariableType.Q_VAR if variant == Q_VAR else sv.VariableType.LOG_RETURN

    def single(self, route, name, n, p, spot=True, variant=LOG_RETURN):
        """(prices, stderrs, ivols | None) of one set from the single-set route; p: a LogSvParams of self.sets(name)"""
        sv = self.sv
        key = (route, name, n, spot, variant, p.sigma0)
        if key not in self._single:
            chain = self.chain(name, variant)
            res = self.randoms(route, name, n)
            par = dict(v0=p.sigma0, theta=p.theta, kappa1=p.kappa1, kappa2=p.kappa2, beta=p.beta, volvol=p.volvol,
                       vol_backbone_etas=p.get_vol_backbone_etas(ttms=chain["ttms"]), is_spot_measure=spot,
                       variable_type=self.vt(sv, variant))
            iv = variant != Q_VAR
            on_res = sv.logsv_mc_chain_pricer_fixed_randoms(W0s=res, W1s=None, dts=None, return_ivols=iv, **par, **chain)
            if route == "frozen":
                want = sv.logsv_mc_chain_pricer(nb_path=n, nb_steps_per_year=SPY, seed=SEED_FROZEN, **par, **chain)
                for a, b in zip(on_res[0] + on_res[1], want[0] + want[1]):
                    assert same(a, b), "the single-set call on the frozen object is not logsv_mc_chain_pricer(seed=...)"
                on_res = (want[0], want[1]) + tuple(on_res[2:])
            self._single[key] = (on_res[0], on_res[1], on_res[2] if iv else None)
        return self._single[key]

    def batch(self, route, name, n, params_list, spot=True, variant=LOG_RETURN):
        sv = self.sv
        out = sv.logsv_mc_chain_pricer_fixed_randoms_batch(params_list=params_list, W0s=self.randoms(route, name, n),
                                                           is_spot_measure=spot, variable_type=self.vt(sv, variant),
                                                           return_ivols=variant != Q_VAR, **self.chain(name, variant))
        assert len(out) == len(params_list)
        return out

    def check(self, got, want, tag):
        """one set's batch result against its single-set result"""
        parts = 2 if want[2] is None else 3
        assert len(got) == parts
        for part, name in zip(range(parts), ("prices", "stderrs", "ivols")):
            assert len(got[part]) == len(want[part])
            for i, (a, b) in enumerate(zip(got[part], want[part])):
                assert same(a, b), f"{tag}: {name} of expiry {i} differ: {np.asarray(a)} {np.asarray(b)}"

    def batch_against_singles(self, route, name, n, width, spot=True, variant=LOG_RETURN):
        sets = self.sets(name)[:width]
        out = self.batch(route, name, n, sets, spot, variant)
        for q, (p, got) in enumerate(zip(sets, out)):
            self.check(got, self.single(route, name, n, p, spot, variant), f"{route}, {name}, {n} paths, {width} sets, set {q}")
        return out

    def free(self):
        for r in self._randoms.values():
            r.free()
        self._randoms.clear()


@pytest.fixture(scope="module")
def ctx():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd import _lib
    _lib.load()
    c = Context(sv)
    yield c
    c.free()


# ---- widths x path counts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,width,n", WIDTH_GRID)
def test_every_width_gives_the_single_set_bits(ctx, route, width, n):
    """the mixed chain (slices of 1, 2, 7 and 12 steps), spot measure, vol backbones on the odd sets, with implied vols"""
    out = ctx.batch_against_singles(route, "mixed", n, width)
    if n >= 4133:                                          # the quotes are priced: the comparison is not of NaNs
        assert all(np.isfinite(np.concatenate(o[0] + o[1])).all() for o in out)
        assert sum(int(np.isfinite(np.concatenate(o[2])).sum()) for o in out) >= 4 * width


# ---- chains ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("width", (4, 7, 8))
@pytest.mark.parametrize("name", ("one_step", "m1", "m2", "m16"))
def test_chains_of_one_step_and_of_one_two_and_sixteen_expiries(ctx, name, width, route):
    assert len(CHAINS[name]["ttms"]) <= MAX_CHAIN_SLICES
    ctx.batch_against_singles(route, name, 257, width)


@pytest.mark.parametrize("width", (4, 7, 8))
def test_seventeen_expiries_on_resident_randoms_fall_back_to_the_single_set_entry(ctx, width):
    """svmc_logsv_chain_price_fixed_sets: a chain past MAX_CHAIN_SLICES is priced set by set through the single-set entry (a
    stepping launch per expiry) -- per set the same bits"""
    assert len(CHAINS["m17"]["ttms"]) == MAX_CHAIN_SLICES + 1
    ctx.batch_against_singles("resident", "m17", 257, width)


@pytest.mark.parametrize("width", (1, 7, 8))
def test_seventeen_expiries_on_the_frozen_route_are_refused(ctx, width):
    """svmc_logsv_chain_price_frozen_sets takes at most sixteen expiries and says so before any launch (an invalid argument: the
    host mirror raises ValueError with the library's message)"""
    with pytest.raises(ValueError, match="at most 16 expiries"):
        ctx.batch("frozen", "m17", 257, ctx.sets("m17")[:width])


# ---- payoff variants ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("width", (4, 5, 7, 8))
@pytest.mark.parametrize("spot", (True, False), ids=("spot", "inverse"))
@pytest.mark.parametrize("variant", (INVERSE_CODES, Q_VAR))
def test_measures_and_payoff_variants(ctx, variant, spot, width, route):
    ctx.batch_against_singles(route, "mixed", 257, width, spot, variant)


# ---- company --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("spot", (True, False), ids=("spot", "inverse"))
def test_a_set_gives_the_same_bits_in_any_company(ctx, route, spot):
    """set 3 (a backbone) alone, in slot 0 and slot 6 of seven, and in slot 5 of eight (on the frozen route the s0 = 4 launch)"""
    sets = ctx.sets("mixed")
    target, others = sets[3], sets[:3] + sets[4:]
    want = ctx.single(route, "mixed", 4133, target, spot)
    arrangements = {"alone": ([target], 0), "slot 0 of 7": ([target] + others[:6], 0), "slot 6 of 7": (others[:6] + [target], 6),
                    "slot 5 of 8": (others[:5] + [target] + others[5:7], 5)}
    for tag, (plist, slot) in arrangements.items():
        out = ctx.batch(route, "mixed", 4133, plist, spot)
        ctx.check(out[slot], want, f"{route}, {tag}")
        for q, p in enumerate(plist):                        # ... and the company keeps its own bits
            ctx.check(out[q], ctx.single(route, "mixed", 4133, p, spot), f"{route}, {tag}, set {q}")


# ---- sharding -------------------------------------------------------------------------------------------------------------------
SHARD_PATHS, SHARDS = 513, ((0, 64), (64, 130), (194, 319))


@pytest.mark.parametrize("width", (7, 8))
def test_frozen_rows_do_not_depend_on_the_sharding(ctx, width):
    """x and qvar of every (set, expiry) of a 513-path call are those of sessions at path_offset 0, 64 and 194 (64, 130 and 319
    paths) side by side.  A shard is a session over an engine built at its path_offset, as the engine's own chain calls make it
    (HipEngine.fused_chain_session: svmc_session_create_on takes the offset), its launches issued directly."""
    import chain_sets_steps as cs
    from stochvolmodels_amd import _lib
    from stochvolmodels_amd.engine import HipEngine, get_engine, marshalled_chain, option_type_codes
    lib = _lib.load()
    assert sum(n for _, n in SHARDS) == SHARD_PATHS and all(a + n == b for (a, n), (b, _) in zip(SHARDS, SHARDS[1:]))
    chain = ctx.chain("mixed", Q_VAR)
    m = chain["ttms"].size
    sets = ctx.sets("mixed")[:width]
    ctx.batch_against_singles("frozen", "mixed", SHARD_PATHS, width, True, Q_VAR)
    res = ctx.randoms("frozen", "mixed", SHARD_PATHS)
    ctx.batch("frozen", "mixed", SHARD_PATHS, sets, True, Q_VAR)     # (the single-set calls in between used the same rows)
    whole = cs.session_rows(get_engine(SHARD_PATHS), res._session_sets, SHARD_PATHS, *res._session_sets_size, width, m, True)

    rows = np.ones((width, 6 + m))
    for row, p in zip(rows, sets):
        row[:6] = (p.sigma0, p.theta, p.kappa1, p.kappa2, p.beta, p.volvol)
        row[6:] = p.get_vol_backbone_etas(ttms=chain["ttms"])
    ch = marshalled_chain(chain["ttms"], chain["forwards"], chain["discfactors"], [np.ascontiguousarray(k) for k in chain["strikes_ttms"]],
                          [option_type_codes(t) for t in chain["optiontypes_ttms"]])
    nbs = (C.c_int * m)(*res.nb_steps)
    dts = np.array(res.dts)
    dp = C.POINTER(C.c_double)
    parts = []
    for off, n in SHARDS:
        eng = HipEngine(n, path_offset=off)
        try:
            eng.use_graphs(False)                           # the engine's stream is the null stream, which is not captured
            size = (8 * m, 8 * max(ch["total"], 1))
            sess = eng.fused_chain_session(*size)
            out = np.empty((2, width, ch["total"]))
            _lib.check(lib.svmc_logsv_chain_price_frozen_sets(
                sess, ch["ttms"], ch["forwards"], ch["discfactors"], m, ch["strikes"], ch["codes"], ch["offsets"], width,
                rows.ctypes.data_as(dp), 1, 2, nbs, dts.ctypes.data_as(dp), SEED_FROZEN, 0, out[0].ctypes.data_as(dp),
                out[1].ctypes.data_as(dp), None))
            snap, state = cs.session_snapshot_ptr(sess, n, *size)
            assert state == (eng.x.ptr, eng.vol.ptr, eng.qvar.ptr)       # the helper reads the object it thinks it reads
            parts.append(cs.session_rows(eng, sess, n, *size, width, m, True))
        finally:
            eng.close()
    for k, what in enumerate(("x", "qvar")):
        got = np.concatenate([p[k] for p in parts], axis=2)
        assert got.shape == whole[k].shape == (width, m, SHARD_PATHS)
        for q in range(width):
            for i in range(m):
                assert np.array_equal(got[q, i], whole[k][q, i]), f"{what} of set {q}, expiry {i}"
    assert np.all(whole[1][:, -1] > 0.0) and np.all(np.diff(whole[1], axis=1) > 0.0)      # qvar grows from slice to slice


# ---- capture, replay, graphs off --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("width", (5, 7))
def test_capture_replay_and_graphs_off(ctx, route, width):
    from stochvolmodels_amd import _lib
    from stochvolmodels_amd.engine import option_type_codes
    lib = _lib.load()
    name, n = "mixed", 4133
    sets = ctx.sets(name)[:width]
    chain = ctx.chain(name)
    res = ctx.randoms(route, name, n)
    ctx.batch(route, name, n, ctx.sets(name)[8:8 + width - 1])       # another set count was captured in between
    for rep in ("capture", "replay", "replay"):
        out = ctx.batch(route, name, n, sets)
        for q, (p, got) in enumerate(zip(sets, out)):
            ctx.check(got, ctx.single(route, name, n, p), f"{route}, {width} sets, {rep}, set {q}")
    # graphs off: the frozen route issues the same launches directly, the resident route prices set by set
    rows = np.ones((width, 6 + chain["ttms"].size))
    for row, p in zip(rows, sets):
        row[:6] = (p.sigma0, p.theta, p.kappa1, p.kappa2, p.beta, p.volvol)
        row[6:] = p.get_vol_backbone_etas(ttms=chain["ttms"])
    args = (chain["ttms"], chain["forwards"], chain["discfactors"], [np.ascontiguousarray(k) for k in chain["strikes_ttms"]],
            [option_type_codes(t) for t in chain["optiontypes_ttms"]], rows, True, 1)
    try:
        if route == "resident":
            _lib.check(lib.svmc_session_use_graphs(res._session_sets, 0))
        out = res.price_logsv_chain_sets(*args, want_ivols=True, use_graph=False)
    finally:
        if route == "resident":
            _lib.check(lib.svmc_session_use_graphs(res._session_sets, 1))
    for q, (p, got) in enumerate(zip(sets, out)):
        want = ctx.single(route, name, n, p)
        if route == "resident":
            # without a graph the single-set entry inverts the prices with the host routine, not the graph's last kernel (svmc.h,
            # svmc_logsv_chain_price_fixed_iv): the same solver on the host's libm, held to the graph's vols as
            # tests/test_gpu_parity.py::test_implied_vols_from_the_graph holds it
            np.testing.assert_allclose(np.concatenate(got[2]), np.concatenate(want[2]), rtol=1e-12)
            got, want = got[:2], want[:2] + (None,)
        ctx.check(got, want, f"{route}, {width} sets, graphs off, set {q}")
    out = ctx.batch(route, name, n, sets)                              # and on again
    for q, (p, got) in enumerate(zip(sets, out)):
        ctx.check(got, ctx.single(route, name, n, p), f"{route}, {width} sets, graphs on again, set {q}")
