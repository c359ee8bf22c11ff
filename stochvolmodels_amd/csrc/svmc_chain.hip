// svmc_chain.hip -- fused single-GPU chain drivers of the C ABI: one call prices a whole option chain.
//
// Restates, in host C++ over the kernels of svmc_kernels.hip and svmc_heston.hip, the expiry loop of logsv_mc_chain_pricer
// (pricers/logsv_pricer.py:806-867) and heston_mc_chain_pricer (pricers/heston_pricer.py:285-331): state
// x0 = 0, vol0 = v0, qvar0 = 0; per slice nb_steps_i = int((T_i - T_{i-1}) * spy) + 1 (utils/funcs.py:44) and
// dt_i = (T_i - T_{i-1}) / nb_steps_i; the state is carried slice to slice in HBM; payoffs per slice by
// compute_mc_vars_payoff (utils/mc_payoffs.py:10-88).  All launches of a chain are queued back to back on the
// session's stream and the host synchronises once, for the D2H of the 3*sum(K_i) sums.
//
// This is the path a C/C++ host takes (examples/price_chain.c).  The Python host drives the same kernels through
// mc_chain.py because it also has to place the two all-reduces of the multi-GPU case between the phases.
#include <cmath>
#include <cstdlib>
#include <vector>

#include "svmc_internal.h"
#include "svmc_black.h"
#include "svmc_quotes.h"
#include <limits>
#include <cstring>

namespace svmc {

constexpr double IV_VOL_LO = 1e-6, IV_VOL_HI = 10.0;       // the bracket of the implied vols (data/option_chain.py's host mirror)

// A captured chain on fixed randoms (svmc_logsv_chain_price_fixed): everything that shapes the launches -- chain,
// randoms, step counts -- is frozen in `key`; the model constants live in `params_dev`, refreshed from the pinned
// `params_host` by the graph's first node, so one hipGraphLaunch re-prices the chain for a new parameter set.
struct FixedGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    std::vector<unsigned char> key;
    double *params_host = nullptr, *params_dev = nullptr, *sums_host = nullptr;   // pinned / device / pinned
    size_t params_doubles = 0, sums_doubles = 0;
    // implied vols on the device (svmc_logsv_chain_price_fixed_iv): per-quote constants, results device / pinned
    double *quotes_dev = nullptr, *ivols_dev = nullptr, *ivols_host = nullptr;
};

// the buffers of the many-job drivers (svmc_*_chain_price_many), grown on demand and apart from everything the other drivers use
struct ManyBuffers {
    double *snap = nullptr, *spot_ws = nullptr, *spot = nullptr, *sums = nullptr;     // device
    void *ws = nullptr, *table_dev = nullptr;                                          // device
    void *table_host = nullptr;                                                        // pinned
    double *sums_pinned = nullptr;                                                     // pinned
    size_t snap_bytes = 0, spot_ws_bytes = 0, spot_bytes = 0, sums_bytes = 0, ws_bytes = 0, table_bytes = 0, table_host_bytes = 0,
           sums_pinned_bytes = 0;
};

// a captured conditional evaluation of a set count (svmc_*_chain_price_cmc_sets): `g` holds the graph and its key alone
struct CmcSetsGraph {
    FixedGraph g;
    void *ws = nullptr, *pinned = nullptr;                  // device, pinned
    size_t ws_bytes = 0, pinned_bytes = 0;
};

struct Session {
    // multi-GPU (svmc_session_set_comm): this session holds the paths [path_offset, path_offset + n_path) of a job of
    // n_total paths spread over `world` ranks; `comm` is the ncclComm_t the two reductions of a chain go through
    void *comm = nullptr;
    // ... or a caller-supplied all-reduce (svmc_session_set_reducer): another transport than RCCL, or a test harness
    svmc_all_reduce_fn reduce_fn = nullptr;
    void *reduce_user = nullptr;
    bool sharded() const { return comm != nullptr || reduce_fn != nullptr; }
    int rank = 0, world = 1;
    uint64_t n_total = 0, path_offset = 0;
    bool use_graphs = true;
    size_t graph_launches = 0;
    FixedGraph fixed;
    FixedGraph fixed_sets;                  // svmc_logsv_chain_price_fixed_sets: several parameter sets per replay
    FixedGraph frozen[MAX_FUSED_SETS + 1];  // svmc_logsv_chain_price_frozen_sets: one captured chain per set count (an SLSQP
                                            // iterate alternates between its base point, 1 set, and its bumped neighbours)
    size_t n_path = 0;
    int max_expiries = 0;
    size_t max_strikes = 0;
    double *x = nullptr, *vol = nullptr, *qvar = nullptr, *snap = nullptr, *spot = nullptr, *sums = nullptr;
    double *sums_pinned = nullptr;          // page-locked landing buffer of the payoff sums: 3 max_strikes doubles (a copy into
                                            // pageable memory costs 16 us more per chain: tools/ubench/sync_latency.py)
    void *ws = nullptr;
    size_t ws_bytes = 0;
    // the generators' per-wave spot partials [2 max_expiries][wave_rows(n_path)], apart from `ws` (the payoff launch's block
    // partials): on one device the payoff kernel reads them while it writes those (one_device_tail)
    double *spot_ws = nullptr;
    size_t spot_ws_bytes = 0;
    hipStream_t stream = nullptr;
    bool owns_state = true, owns_stream = true;   // false: svmc_session_create_on -- the caller's state arrays / stream
    // svmc_session_time_stepping: HIP events around the stepping launch (+ its spot-sum reduce) of the on-device-RNG chain
    // drivers, on the session's stream -- what a host that times the dominant kernel (bench.py) reads back after the call
    bool time_stepping = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_stepping_ms = -1.0f;
    ManyBuffers many;
    // svmc_hawkesjd_chain_price_tilted: the page-locked landing buffer of its prices, errors and statistics, grown on demand
    double *tilted_pinned = nullptr;
    size_t tilted_pinned_bytes = 0;
    // svmc_*_chain_price_cmc: the fourth state array (cv) and the payoff tail's workspace, grown on demand
    double *cmc_cv = nullptr;
    void *cmc_ws = nullptr, *cmc_pinned = nullptr;          // device, device, pinned (the chain table's image and the results)
    size_t cmc_cv_bytes = 0, cmc_ws_bytes = 0, cmc_pinned_bytes = 0;
    // svmc_*_chain_price_greeks: the Greeks tail's workspace and its page-locked block (the table's image, then the results)
    void *greeks_ws = nullptr, *greeks_pinned = nullptr;   // device, pinned
    size_t greeks_ws_bytes = 0, greeks_pinned_bytes = 0;
    // svmc_*_chain_price_cmc_many / _cmc_sens: the jobs' mu and cv rows, the job table (device, pinned), the sensitivity tail's
    // workspace and its page-locked block (the table's image, then the results), grown on demand
    double *cmany_snap = nullptr;
    void *cmany_table_dev = nullptr, *cmany_table_host = nullptr, *csens_ws = nullptr, *csens_pinned = nullptr;
    size_t cmany_snap_bytes = 0, cmany_table_bytes = 0, cmany_table_host_bytes = 0, csens_ws_bytes = 0, csens_pinned_bytes = 0;
    // svmc_*_chain_price_cmc_sets: one captured evaluation per set count (an SLSQP iterate alternates between its base point and its
    // bumped neighbours), each with a tail workspace -- whose head is the table's image, uploaded once per key -- and a page-locked
    // result block of its own: no other driver writes them.  The stepping buffers (cmany_*) are shared: cmc_sets_drop
    CmcSetsGraph cmc_sets[SVMC_CMC_SETS_MAX + 1];
    // ... and, for a session on the default stream (svmc_session_create_on with a null stream), which cannot be captured, the
    // stream those evaluations run on: they touch no state another stream of the session's caller works on, and every call on
    // the session ends synchronised
    hipStream_t cmc_sets_stream = nullptr;
};

// events around a stepping call of a timed session (no-ops otherwise)
static void stepping_begin(Session *s)
{
    if (s->time_stepping && s->ev0 != nullptr) (void)hipEventRecord(s->ev0, s->stream);
}
static void stepping_end(Session *s)
{
    if (s->time_stepping && s->ev1 != nullptr) (void)hipEventRecord(s->ev1, s->stream);
}
// after the chain's synchronisation
static void stepping_read(Session *s)
{
    s->last_stepping_ms = -1.0f;
    if (s->time_stepping && s->ev0 != nullptr && s->ev1 != nullptr) {
        float ms = -1.0f;
        if (hipEventElapsedTime(&ms, s->ev0, s->ev1) == hipSuccess) s->last_stepping_ms = ms;
    }
}

static void fixed_graph_release(FixedGraph &g)
{
    if (g.exec != nullptr) (void)hipGraphExecDestroy(g.exec);
    if (g.graph != nullptr) (void)hipGraphDestroy(g.graph);
    if (g.params_host != nullptr) (void)hipHostFree(g.params_host);
    if (g.sums_host != nullptr) (void)hipHostFree(g.sums_host);
    if (g.params_dev != nullptr) (void)hipFree(g.params_dev);
    if (g.quotes_dev != nullptr) (void)hipFree(g.quotes_dev);
    if (g.ivols_dev != nullptr) (void)hipFree(g.ivols_dev);
    if (g.ivols_host != nullptr) (void)hipHostFree(g.ivols_host);
    g = FixedGraph();
}

static void session_release(Session *s)
{
    if (s == nullptr) return;
    fixed_graph_release(s->fixed);
    fixed_graph_release(s->fixed_sets);
    for (FixedGraph &g : s->frozen) fixed_graph_release(g);
    if (s->owns_state)
        for (void *p : {static_cast<void *>(s->x), static_cast<void *>(s->vol), static_cast<void *>(s->qvar)})
            if (p != nullptr) (void)hipFree(p);
    for (void *p : {static_cast<void *>(s->snap), static_cast<void *>(s->spot), static_cast<void *>(s->sums), s->ws,
                    static_cast<void *>(s->spot_ws)})
        if (p != nullptr) (void)hipFree(p);
    if (s->sums_pinned != nullptr) (void)hipHostFree(s->sums_pinned);
    if (s->tilted_pinned != nullptr) (void)hipHostFree(s->tilted_pinned);
    if (s->cmc_cv != nullptr) (void)hipFree(s->cmc_cv);
    if (s->cmc_ws != nullptr) (void)hipFree(s->cmc_ws);
    if (s->cmc_pinned != nullptr) (void)hipHostFree(s->cmc_pinned);
    if (s->greeks_ws != nullptr) (void)hipFree(s->greeks_ws);
    if (s->greeks_pinned != nullptr) (void)hipHostFree(s->greeks_pinned);
    for (void *p : {static_cast<void *>(s->cmany_snap), s->cmany_table_dev, s->csens_ws})
        if (p != nullptr) (void)hipFree(p);
    for (void *p : {s->cmany_table_host, s->csens_pinned})
        if (p != nullptr) (void)hipHostFree(p);
    for (CmcSetsGraph &cg : s->cmc_sets) {
        fixed_graph_release(cg.g);
        if (cg.ws != nullptr) (void)hipFree(cg.ws);
        if (cg.pinned != nullptr) (void)hipHostFree(cg.pinned);
    }
    if (s->cmc_sets_stream != nullptr) (void)hipStreamDestroy(s->cmc_sets_stream);
    ManyBuffers &mb = s->many;
    for (void *p : {static_cast<void *>(mb.snap), static_cast<void *>(mb.spot_ws), static_cast<void *>(mb.spot),
                    static_cast<void *>(mb.sums), mb.ws, mb.table_dev})
        if (p != nullptr) (void)hipFree(p);
    for (void *p : {mb.table_host, static_cast<void *>(mb.sums_pinned)})
        if (p != nullptr) (void)hipHostFree(p);
    if (s->ev0 != nullptr) (void)hipEventDestroy(s->ev0);
    if (s->ev1 != nullptr) (void)hipEventDestroy(s->ev1);
    if (s->owns_stream && s->stream != nullptr) (void)hipStreamDestroy(s->stream);
    delete s;
}

// intrinsic value at the forward for LOG_RETURN, zero otherwise (the shift of svmc_payoff_sums)
static double payoff_shift(double strike, int type, double forward, int variable_type)
{
    if (variable_type != SVMC_LOG_RETURN) return 0.0;
    const bool call = (type == SVMC_CALL || type == SVMC_INV_CALL);
    const double intrinsic = call ? std::fmax(forward - strike, 0.0) : std::fmax(strike - forward, 0.0);
    return (type >= SVMC_INV_CALL) ? intrinsic / forward : intrinsic;
}

struct ChainView {
    int m;
    const double *ttms, *forwards, *discfactors, *strikes;
    const int8_t *types;
    const size_t *offsets;   // [m + 1] into strikes/types
};

// the step grid of every expiry of a chain, each slice starting at the previous expiry (utils/funcs.py:44-47)
static void expiry_grids(const ChainView &c, int nb_steps_per_year, std::vector<int> &nbs, std::vector<double> &dts)
{
    nbs.resize(c.m);
    dts.resize(c.m);
    double t0 = 0.0;
    for (int i = 0; i < c.m; ++i) {
        const double ttm = c.ttms[i] - t0;
        nbs[i] = static_cast<int>(ttm * static_cast<double>(nb_steps_per_year)) + 1;
        dts[i] = (nbs[i] == 1) ? ttm : ttm / static_cast<double>(nbs[i]);
        t0 = c.ttms[i];
    }
}

// (needs_discfactors false: the undiscounted pricers, whose view carries no discount factors)
static int check_chain(const char *fn, const Session *s, const ChainView &c, int variable_type, const double *prices,
                       const double *stderrs, bool needs_discfactors = true)
{
    if (s == nullptr) return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": null session");
    if (!c.ttms || !c.forwards || (needs_discfactors && !c.discfactors) || !c.strikes || !c.types || !c.offsets || !prices || !stderrs)
        return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": null pointer");
    if (c.m < 1 || c.m > s->max_expiries) return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": expiries exceed the session");
    if (c.offsets[c.m] > s->max_strikes) return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": strikes exceed the session");
    if (variable_type == SVMC_SIGMA) return fail(SVMC_ERR_UNSUPPORTED_VARIABLE, std::string(fn) + ": VariableType.SIGMA");
    if (variable_type != SVMC_LOG_RETURN && variable_type != SVMC_Q_VAR)
        return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": unknown variable type");
    for (size_t k = 0; k < c.offsets[c.m]; ++k)
        if (c.types[k] < SVMC_CALL || c.types[k] > SVMC_INV_PUT) return fail(SVMC_ERR_UNKNOWN_PAYOFF, "unknown option payoff code");
    double prev = 0.0;
    for (int i = 0; i < c.m; ++i) {
        if (!(c.ttms[i] > prev)) return fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": ttms must be positive and increasing");
        prev = c.ttms[i];
    }
    return SVMC_OK;
}

static void payoff_shifts_of(const ChainView &c, int variable_type, std::vector<double> &shifts)
{
    shifts.resize(c.offsets[c.m]);
    for (int i = 0; i < c.m; ++i)
        for (size_t k = c.offsets[i]; k < c.offsets[i + 1]; ++k)
            shifts[k] = payoff_shift(c.strikes[k], c.types[k], c.forwards[i], variable_type);
}

// the snapshot rows of parameter set q of P: x of expiry i at row q m + i, qvar at row (P + q) m + i (rows of n_path doubles)
struct SnapshotRows {
    std::vector<const double *> x, qvar;
};
static SnapshotRows snapshot_rows(const Session *s, const ChainView &c, int q, int P)
{
    SnapshotRows r{std::vector<const double *>(c.m), std::vector<const double *>(c.m)};
    for (int i = 0; i < c.m; ++i) {
        r.x[i] = s->snap + static_cast<size_t>(q * c.m + i) * s->n_path;
        r.qvar[i] = s->snap + static_cast<size_t>((P + q) * c.m + i) * s->n_path;
    }
    return r;
}

// phase 3 of mc_chain.py, per-strike sums of every slice queued on the session's stream, for parameter set `set` of P: its
// snapshot rows, spot sums and output block -- one launch pair per set with the single-set launch shape, hence the single-set bits
static int enqueue_payoff_sums_of_set(Session *s, const ChainView &c, int variable_type, const std::vector<double> &shifts,
                                      int set, int n_sets)
{
    const size_t K = c.offsets[c.m];
    const SnapshotRows r = snapshot_rows(s, c, set, n_sets);
    return svmc_payoff_sums_chain(r.x.data(), variable_type == SVMC_Q_VAR ? r.qvar.data() : nullptr, s->n_path, c.forwards, c.ttms,
                                  s->spot + 2 * static_cast<size_t>(set) * c.m, c.m, c.strikes, c.types, shifts.data(), c.offsets,
                                  variable_type, s->sums + 3 * K * static_cast<size_t>(set), s->ws, s->ws_bytes, s->stream);
}

// the payoff sums of all n_sets sets: one launch and one column reduce where the chain allows it (the bits of the per-set loop)
static int enqueue_payoff_sums_of_sets(Session *s, const ChainView &c, int variable_type, const std::vector<double> &shifts,
                                       int n_sets)
{
    if (n_sets > 1 && payoff_sets_fit(s->n_path, c.m, c.offsets, c.types, n_sets, s->ws_bytes)) {
        const size_t n = s->n_path;
        const SnapshotRows r = snapshot_rows(s, c, 0, n_sets);
        return payoff_sums_chain_sets(r.x.data(), variable_type == SVMC_Q_VAR ? r.qvar.data() : nullptr, n, c.forwards, c.ttms, s->spot,
                                      c.m, c.strikes, c.types, shifts.data(), c.offsets, variable_type, s->sums, s->ws, s->ws_bytes,
                                      s->stream, n_sets, static_cast<size_t>(c.m) * n, static_cast<size_t>(c.m) * n,
                                      2 * static_cast<size_t>(c.m));
    }
    for (int q = 0; q < n_sets; ++q)
        if (int rc = enqueue_payoff_sums_of_set(s, c, variable_type, shifts, q, n_sets)) return rc;
    return SVMC_OK;
}

// host side of the implied vols for the routes that do not replay a graph (multi-GPU, graphs off): the same solver
static void implied_vols_on_host(const ChainView &c, int variable_type, const double *prices, double *ivols)
{
    for (int i = 0; i < c.m; ++i)
        for (size_t k = c.offsets[i]; k < c.offsets[i + 1]; ++k) {
            // quotes on the log-return only: options on the realised variance have no Black vol on the forward; inverse
            // options (IC / IP) as in chain_implied_vols_kernel: the vanilla inversion of price x forward
            const bool call = c.types[k] == SVMC_CALL || c.types[k] == SVMC_INV_CALL;
            const double px = c.types[k] >= SVMC_INV_CALL ? prices[k] * c.forwards[i] : prices[k];
            ivols[k] = variable_type == SVMC_LOG_RETURN
                           ? black_implied_vol(px, c.strikes[k], call, c.forwards[i], c.ttms[i], c.discfactors[i], IV_VOL_LO, IV_VOL_HI)
                           : std::numeric_limits<double>::quiet_NaN();
        }
}

// the path count of the WHOLE job, which the standard errors divide by
static double paths_of_job(const Session *s)
{
    return static_cast<double>(s->sharded() ? s->n_total : s->n_path);
}

// phase 4 for P parameter sets, blocks of K = offsets[m] quotes: host finalisation of the downloaded sums
// (utils/mc_payoffs.py:85-88), then, when asked for, the implied vols -- the graph's, or the host solver's where it has none
static int finish_sets(const Session *s, const ChainView &c, const double *sums, const std::vector<double> &shifts, int P,
                       int variable_type, double *prices, double *stderrs, double *ivols, const double *ivols_pinned)
{
    const size_t K = c.offsets[c.m];
    const double n_all = paths_of_job(s);
    for (int q = 0; q < P; ++q)
        for (int i = 0; i < c.m; ++i) {
            const size_t k0 = c.offsets[i], k = c.offsets[i + 1] - k0, b = K * q + k0;
            if (int rc = svmc_payoff_finalize(sums + 3 * b, shifts.data() + k0, k, c.discfactors[i], n_all, prices + b, stderrs + b))
                return rc;
        }
    if (ivols == nullptr) return SVMC_OK;
    if (ivols_pinned != nullptr)
        memcpy(ivols, ivols_pinned, K * P * sizeof(double));
    else
        for (int q = 0; q < P; ++q) implied_vols_on_host(c, variable_type, prices + K * q, ivols + K * q);
    return SVMC_OK;
}

// The two cross-rank couplings of compute_mc_vars_payoff, as in-place fp64 sum all-reduces on the session's stream,
// stream-ordered against the kernels on either side (no host synchronisation): phase 2 = [sum F exp(x), count] per
// expiry (utils/mc_payoffs.py:61-63), phase 3' = [sum d, sum d^2, count] per strike (:85-86).  No-ops without a comm.
static int all_reduce(Session *s, double *buf, size_t n)
{
    if (!s->sharded() || n == 0) return SVMC_OK;
    if (s->reduce_fn != nullptr) {
        last_error_ref().clear();
        const int rc = s->reduce_fn(s->reduce_user, buf, n, reinterpret_cast<svmc_stream_t>(s->stream));
        if (rc == SVMC_OK) return SVMC_OK;
        const std::string why = last_error_ref();          // what the callback itself said, if it went through this library
        return fail(rc, "the session's all-reduce callback failed" + (why.empty() ? std::string() : ": " + why));
    }
    return svmc_rccl_all_reduce_sum(s->comm, buf, n, reinterpret_cast<svmc_stream_t>(s->stream));
}

// The tail of an on-device-RNG chain on ONE device (no communicator): the stepping launch left its per-wave spot partials in
// s->spot_ws unreduced; the payoff kernel sums them itself (up to 2048 rows; a reduce launch ahead of it otherwise) and
// chain_finish_kernel, a wave per quote, forms the column sums in reduce_columns_kernel's order (the bits of the five-node tail
// below) and stores them straight into the pinned host buffer.  Whether a chain takes it: one_device_tail().
static bool one_device_tail(const Session *s, const ChainView &c)
{
    static const bool off = getenv("SVMC_CHAIN_TAIL_NODES") != nullptr && atoi(getenv("SVMC_CHAIN_TAIL_NODES")) == 5;   // A/B, tests
    return !off && !s->sharded() && c.m <= MAX_FUSED_SLICES &&
           static_cast<size_t>(wave_rows(s->n_path)) * 2 * static_cast<size_t>(c.m) * sizeof(double) <= s->spot_ws_bytes &&
           payoff_sets_fit(s->n_path, c.m, c.offsets, c.types, 1, s->ws_bytes);
}

static int enqueue_one_device_tail(Session *s, const ChainView &c, int variable_type, const std::vector<double> &shifts, double *sums_out)
{
    const size_t n = s->n_path;
    const SnapshotRows r = snapshot_rows(s, c, 0, 1);
    const bool in_kernel = spot_sums_in_payoff_kernel(n);
    if (!in_kernel)
        if (int rc = reduce_spot_partials(s->spot_ws, n, 2 * c.m, s->spot, s->stream)) return rc;
    return chain_payoff_and_finish(r.x.data(), variable_type == SVMC_Q_VAR ? r.qvar.data() : nullptr, n, c.forwards, c.ttms, s->spot,
                                   in_kernel ? s->spot_ws : nullptr, c.m, c.strikes, c.types, shifts.data(), c.offsets, variable_type,
                                   s->ws, s->ws_bytes, s->stream, sums_out);
}

// partials_pending: the stepping launch(es) left the per-wave spot partials in s->spot_ws unreduced (the on-device-RNG drivers);
// false: s->spot already holds this rank's spot sums (the slice-by-slice fixed-randoms route)
static int reduce_and_finalize(Session *s, const ChainView &c, int variable_type, double *prices, double *stderrs,
                               bool partials_pending)
{
    std::vector<double> shifts;
    payoff_shifts_of(c, variable_type, shifts);
    if (partials_pending && one_device_tail(s, c)) {
        if (int rc = enqueue_one_device_tail(s, c, variable_type, shifts, s->sums_pinned)) return rc;
    } else {
        if (partials_pending)
            if (int rc = reduce_spot_partials(s->spot_ws, s->n_path, 2 * c.m, s->spot, s->stream)) return rc;
        if (int rc = all_reduce(s, s->spot, 2 * static_cast<size_t>(c.m))) return rc;
        if (int rc = enqueue_payoff_sums_of_set(s, c, variable_type, shifts, 0, 1)) return rc;
        if (int rc = all_reduce(s, s->sums, 3 * c.offsets[c.m])) return rc;
        SVMC_HIP_TRY(hipMemcpyAsync(s->sums_pinned, s->sums, 3 * c.offsets[c.m] * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    }
    SVMC_HIP_TRY(hipStreamSynchronize(s->stream));
    stepping_read(s);
    return finish_sets(s, c, s->sums_pinned, shifts, 1, variable_type, prices, stderrs, nullptr, nullptr);
}

// ---- the captured chains (FixedGraph): a key, the buffers it sizes, a graph captured from the driver's `enqueue`

template <class T>
static void key_append(std::vector<unsigned char> &key, const T *p, size_t count)
{
    const unsigned char *b = reinterpret_cast<const unsigned char *>(p);
    key.insert(key.end(), b, b + count * sizeof(T));
}

// the part of a graph's key every driver shares: the chain, P and the results asked for (the discount factors only matter to the
// implied vols); each driver appends what else shapes its launches
static std::vector<unsigned char> chain_key(const ChainView &c, int P, int variable_type, int want_iv)
{
    std::vector<unsigned char> key;
    key_append(key, &c.m, 1);
    key_append(key, &P, 1);
    key_append(key, &variable_type, 1);
    key_append(key, &want_iv, 1);
    key_append(key, c.ttms, c.m);
    key_append(key, c.discfactors, want_iv ? c.m : 0);
    key_append(key, c.forwards, c.m);
    key_append(key, c.offsets, c.m + 1);
    key_append(key, c.strikes, c.offsets[c.m]);
    key_append(key, c.types, c.offsets[c.m]);
    return key;
}

// the parameter block of P sets: [P] initial volatilities, then [m][P] model constants of WIDTH doubles -- for one set the
// [v0][m constants] of the single-set kernels.  Set q is sets + row q = (v0, theta, kappa1, kappa2, beta, volvol), its vol-backbone
// etas are at etas + row q (1 where etas is null).
template <void (*TO_DOUBLES)(double, double, double, double, double, double, double, int, double *), int WIDTH>
static void fill_params(double *block, const ChainView &c, int P, const double *sets, const double *etas, size_t row,
                        const double *dts, int is_spot_measure)
{
    for (int q = 0; q < P; ++q) {
        const double *pr = sets + row * q, *eta = etas ? etas + row * q : nullptr;
        block[q] = pr[0];
        for (int i = 0; i < c.m; ++i)
            TO_DOUBLES(dts[i], pr[1], pr[2], pr[3], pr[4], pr[5], eta ? eta[i] : 1.0, is_spot_measure,
                       block + P + (static_cast<size_t>(i) * P + q) * WIDTH);
    }
}

// (re)allocates g for a new key: the pinned and device parameter blocks (fill_params, constants of params_width doubles), the
// pinned sums of P sets and, with implied vols, the quote table of every set -- part of the key, so uploaded once, outside the graph
static int graph_prepare(FixedGraph &g, const std::vector<unsigned char> &key, const ChainView &c, const std::vector<double> &shifts,
                         int P, int params_width, bool want_iv)
{
    fixed_graph_release(g);
    const size_t K = c.offsets[c.m], n_quotes = K * P;
    g.params_doubles = static_cast<size_t>(P) * (1 + static_cast<size_t>(c.m) * params_width);
    g.sums_doubles = 3 * n_quotes;
    SVMC_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&g.params_host), g.params_doubles * sizeof(double), hipHostMallocDefault));
    SVMC_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&g.sums_host), (g.sums_doubles ? g.sums_doubles : 1) * sizeof(double),
                               hipHostMallocDefault));
    SVMC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&g.params_dev), g.params_doubles * sizeof(double)));
    if (want_iv && n_quotes) {
        std::vector<double> quotes(IV_QUOTE_DOUBLES_HOST * n_quotes);
        for (int q = 0; q < P; ++q)
            for (int i = 0; i < c.m; ++i)
                for (size_t k = c.offsets[i]; k < c.offsets[i + 1]; ++k) {
                    double *qd = quotes.data() + IV_QUOTE_DOUBLES_HOST * (K * q + k);
                    qd[0] = c.strikes[k];
                    qd[1] = static_cast<double>(c.types[k]);
                    qd[2] = shifts[k];
                    qd[3] = c.forwards[i];
                    qd[4] = c.ttms[i];
                    qd[5] = c.discfactors[i];
                }
        SVMC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&g.quotes_dev), quotes.size() * sizeof(double)));
        SVMC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&g.ivols_dev), n_quotes * sizeof(double)));
        SVMC_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&g.ivols_host), n_quotes * sizeof(double), hipHostMallocDefault));
        SVMC_HIP_TRY(hipMemcpy(g.quotes_dev, quotes.data(), quotes.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    g.key = key;
    return SVMC_OK;
}

// captures enqueue() -- a driver's launches on `stream` (the session's, by default), one linear chain of nodes -- into g and
// instantiates it.  Capture mode is always left; g is released on any error.
template <class Enqueue>
static int graph_capture(Session *s, FixedGraph &g, const char *fn, Enqueue enqueue, hipStream_t stream = nullptr)
{
    if (stream == nullptr) stream = s->stream;
    int rc = SVMC_OK;
    hipError_t e = hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed);
    if (e == hipSuccess) {
        rc = enqueue();
        e = hipStreamEndCapture(stream, &g.graph);
        if (rc == SVMC_OK && e == hipSuccess) e = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
    }
    if (rc == SVMC_OK && e == hipSuccess) return SVMC_OK;
    fixed_graph_release(g);
    return rc != SVMC_OK ? rc : fail(SVMC_ERR_HIP, std::string(fn) + ": graph capture: " + hipGetErrorString(e));
}

// the last step of a captured chain, its results home: with implied vols the last kernel writes both the sums and the vols into
// the pinned host buffers (two copy nodes fewer per replay); without, the sums' copy
static int enqueue_results_home(Session *s, const FixedGraph &g)
{
    if (g.ivols_dev != nullptr)
        return chain_implied_vols(s->sums, g.quotes_dev, g.sums_doubles / 3, paths_of_job(s), IV_VOL_LO, IV_VOL_HI, g.ivols_host,
                                  g.sums_host, s->stream);
    if (g.sums_doubles)
        SVMC_HIP_TRY(hipMemcpyAsync(g.sums_host, s->sums, g.sums_doubles * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    return SVMC_OK;
}

// the key of a chain on fixed randoms (svmc_logsv_chain_price_fixed_iv, _fixed_sets)
static std::vector<unsigned char> fixed_key(const ChainView &c, int P, int variable_type, int want_iv, size_t ldw,
                                            const double *const *W0s, const double *const *W1s, const int *nb_steps)
{
    std::vector<unsigned char> key = chain_key(c, P, variable_type, want_iv);
    key_append(key, &ldw, 1);
    key_append(key, W0s, c.m);
    key_append(key, W1s, c.m);
    key_append(key, nb_steps, c.m);
    return key;
}

// The stepping half of every single-chain driver on device randoms: the chain's checks, the entry point's own ahead of the step
// count's (check()) and after it (prepare(): also its set-up before the launch), the step grids and the model's stepping call step(nbs,
// dts, qsnap, spot, ws, ws_bytes).  One launch may leave (may_pend) its spot partials unreduced in s->spot_ws for the tail: `pending`.
struct Stepped { int rc; bool pending; };
static int no_check() { return SVMC_OK; }
template <class Step, class Check = int (*)(), class Prepare = int (*)()>
static Stepped single_step(const char *fn, Session *s, const ChainView &c, int nb_steps_per_year, int variable_type, const double *prices,
                           const double *stderrs, bool needs_discfactors, bool may_pend, Step &&step, Check &&check = no_check,
                           Prepare &&prepare = no_check)
{
    if (int rc = check_chain(fn, s, c, variable_type, prices, stderrs, needs_discfactors)) return {rc, false};
    if (int rc = check()) return {rc, false};
    if (nb_steps_per_year <= 0) return {fail(SVMC_ERR_INVALID_ARGUMENT, std::string(fn) + ": nb_steps_per_year must be positive"), false};
    if (int rc = prepare()) return {rc, false};
    std::vector<int> nbs;       // (the start state of every path travels to the first launch as three constants: no fill launch)
    std::vector<double> dts;
    expiry_grids(c, nb_steps_per_year, nbs, dts);
    double *qsnap = (variable_type == SVMC_Q_VAR) ? s->snap + static_cast<size_t>(c.m) * s->n_path : nullptr;
    const bool pending = may_pend && c.m <= MAX_FUSED_SLICES;
    stepping_begin(s);
    const int rc = step(nbs.data(), dts.data(), qsnap, pending ? nullptr : s->spot, pending ? s->spot_ws : s->ws,
                        pending ? s->spot_ws_bytes : s->ws_bytes);
    if (rc == SVMC_OK) stepping_end(s);
    return {rc, pending};
}

// *p at least `need` bytes (its contents are not kept); every call that grows one ends synchronised, so nothing still reads the old
static hipError_t grow(void **p, size_t &cap, size_t need, bool pinned)
{
    if (*p != nullptr && need <= cap) return hipSuccess;
    if (*p != nullptr) (void)(pinned ? hipHostFree(*p) : hipFree(*p));
    *p = nullptr;
    cap = 0;
    const hipError_t e = pinned ? hipHostMalloc(p, need, hipHostMallocDefault) : hipMalloc(p, need);
    if (e == hipSuccess) cap = need;
    return e;
}

// what the tilted calls check beyond the chain's own checks, for n_gamma_values gammas (n_gammas per job)
static int check_tilted(const char *fn, const ChainView &c, const double *gammas, size_t n_gamma_values, int n_gammas, const double *stats)
{
    SVMC_REQUIRE(gammas != nullptr && stats != nullptr, std::string(fn) + ": null pointer");
    SVMC_REQUIRE(n_gammas >= 1 && n_gammas <= SVMC_TILTED_MAX_GAMMAS, std::string(fn) + ": n_gammas outside 1 .. SVMC_TILTED_MAX_GAMMAS");
    for (size_t g = 0; g < n_gamma_values; ++g) SVMC_REQUIRE(std::isfinite(gammas[g]), std::string(fn) + ": a gamma is not finite");
    for (int i = 0; i < c.m; ++i) {
        SVMC_REQUIRE(std::isfinite(c.forwards[i]), std::string(fn) + ": a forward is not finite");
        SVMC_REQUIRE(c.offsets[i] <= c.offsets[i + 1], std::string(fn) + ": strike offsets must not decrease");
    }
    for (size_t k = 0; k < c.offsets[c.m]; ++k) {
        if (c.types[k] != SVMC_CALL && c.types[k] != SVMC_PUT) return fail(SVMC_ERR_UNKNOWN_PAYOFF, "unknown option payoff code");
        SVMC_REQUIRE(std::isfinite(c.strikes[k]), std::string(fn) + ": a strike is not finite");
    }
    return SVMC_OK;
}

// the page-locked landing block of the tilted calls in s->tilted_pinned: per job [prices G K | stderrs G K | stats G m 8]; after
// the synchronisation copy_home puts job j's pieces into the caller's [J][G K], [J][G K] and [J][G m 8] arrays
struct TiltedBlock {
    double *base;
    size_t GK, n_stats;
    double *prices(size_t j) const { return base + j * (2 * GK + n_stats); }
    double *stderrs(size_t j) const { return prices(j) + GK; }
    double *stats(size_t j) const { return stderrs(j) + GK; }
    void copy_home(size_t j, double *prices_host, double *stderrs_host, double *stats_host) const
    {
        memcpy(prices_host + j * GK, prices(j), GK * sizeof(double));
        memcpy(stderrs_host + j * GK, stderrs(j), GK * sizeof(double));
        memcpy(stats_host + j * n_stats, stats(j), n_stats * sizeof(double));
    }
};
static int tilted_block(Session *s, const ChainView &c, int n_gammas, int n_jobs, TiltedBlock &b)
{
    b.GK = static_cast<size_t>(n_gammas) * c.offsets[c.m];
    b.n_stats = static_cast<size_t>(n_gammas) * c.m * SVMC_TILTED_STATS_DOUBLES;
    SVMC_HIP_TRY(grow(reinterpret_cast<void **>(&s->tilted_pinned), s->tilted_pinned_bytes,
                      static_cast<size_t>(n_jobs) * (2 * b.GK + b.n_stats) * sizeof(double), true));
    b.base = s->tilted_pinned;
    return SVMC_OK;
}

// ---- conditional Monte Carlo (include/svmc.h; kernels and the payoff tail: svmc_cmc.hip).  The chain's checks and step grids are
// single_step's; mu rides in the session's x, cv in an array of its own, expiry i's snapshots in rows i and m + i of s->snap.
template <class Step>
static int chain_price_cmc(const char *fn, Session *s, const ChainView &c, int nb_steps_per_year, int recenter, double *prices_host,
                           double *stderrs_host, double *greeks_host, double *stats_host, Step &&step)
{
    // greeks_host (svmc_*_chain_price_cmc_greeks) [SVMC_CMC_GREEKS_ROWS][K]: the tail with the derivatives; prices_host and
    // stderrs_host are then its first two rows
    double *mu_snap = nullptr, *cv_snap = nullptr;
    const bool deriv = greeks_host != nullptr;
    const Stepped st = single_step(fn, s, c, nb_steps_per_year, SVMC_LOG_RETURN, prices_host, stderrs_host, true, false,
                                   [&](const int *nbs, const double *dts, double *, double *, void *, size_t) {
                                       return step(nbs, dts, mu_snap, cv_snap);
                                   },
                                   [&]() {
                                       SVMC_REQUIRE(!s->sharded(), std::string(fn) + ": the conditional estimator is not sharded");
                                       for (size_t k = 0; k < c.offsets[c.m]; ++k)
                                           if (c.types[k] != SVMC_CALL && c.types[k] != SVMC_PUT)
                                               return fail(SVMC_ERR_UNKNOWN_PAYOFF, "unknown option payoff code");
                                       return SVMC_OK;
                                   },
                                   [&]() {
                                       SVMC_HIP_TRY(grow(reinterpret_cast<void **>(&s->cmc_cv), s->cmc_cv_bytes, s->n_path * sizeof(double), false));
                                       const size_t K = c.offsets[c.m];
                                       SVMC_HIP_TRY(grow(&s->cmc_ws, s->cmc_ws_bytes, cmc_workspace_bytes_of(s->n_path, c.m, K, deriv), false));
                                       SVMC_HIP_TRY(grow(&s->cmc_pinned, s->cmc_pinned_bytes, cmc_pinned_bytes_of(c.m, K, deriv), true));
                                       mu_snap = s->snap;
                                       cv_snap = s->snap + static_cast<size_t>(c.m) * s->n_path;
                                       return SVMC_OK;
                                   });
    if (st.rc) return st.rc;
    std::vector<const double *> mus(c.m), cvs(c.m);
    for (int i = 0; i < c.m; ++i) {
        mus[i] = mu_snap + static_cast<size_t>(i) * s->n_path;
        cvs[i] = cv_snap + static_cast<size_t>(i) * s->n_path;
    }
    const int rc = cmc_tail(fn, mus.data(), cvs.data(), s->n_path, c.forwards, c.discfactors, c.m, c.strikes, c.types, c.offsets, recenter,
                            prices_host, stderrs_host, greeks_host, stats_host, s->cmc_ws, s->cmc_ws_bytes, s->stream, s->cmc_pinned,
                            s->cmc_pinned_bytes);
    if (rc == SVMC_OK) stepping_read(s);
    return rc;
}

}  // namespace svmc

using namespace svmc;

extern "C" {

static int session_create(const char *fn, svmc_session_t *session, size_t n_path, int max_expiries, size_t max_strikes_total,
                          double *x, double *vol, double *qvar, bool borrow_stream, hipStream_t stream_in);

int svmc_session_create(svmc_session_t *session, size_t n_path, int max_expiries, size_t max_strikes_total)
{
    return session_create("svmc_session_create", session, n_path, max_expiries, max_strikes_total, nullptr, nullptr, nullptr, false,
                          nullptr);
}

int svmc_session_create_on(svmc_session_t *session, size_t n_path, int max_expiries, size_t max_strikes_total, double *x,
                           double *vol, double *qvar, uint64_t path_offset, svmc_stream_t stream)
{
    SVMC_REQUIRE(x != nullptr && vol != nullptr && qvar != nullptr, "svmc_session_create_on: null state array");
    if (int rc = session_create("svmc_session_create_on", session, n_path, max_expiries, max_strikes_total, x, vol, qvar, true,
                                as_stream(stream)))
        return rc;
    reinterpret_cast<Session *>(*session)->path_offset = path_offset;
    return SVMC_OK;
}

static int session_create(const char *fn, svmc_session_t *session, size_t n_path, int max_expiries, size_t max_strikes_total,
                          double *x, double *vol, double *qvar, bool borrow_stream, hipStream_t stream_in)
{
    SVMC_REQUIRE(session != nullptr, std::string(fn) + ": null output");
    SVMC_REQUIRE(n_path > 0 && max_expiries > 0 && max_strikes_total > 0, std::string(fn) + ": sizes must be positive");
    Session *s = new Session;
    s->n_path = n_path;
    s->max_expiries = max_expiries;
    s->max_strikes = max_strikes_total;
    s->owns_state = x == nullptr;
    s->owns_stream = !borrow_stream;
    s->x = x;
    s->vol = vol;
    s->qvar = qvar;
    s->stream = stream_in;
    size_t ws = 0;
    int rc = svmc_slice_workspace_bytes(n_path, &ws);
    // the multi-set replay (svmc_logsv_chain_price_fixed_sets) writes two partial columns per (expiry, set): a session created
    // for m x P chains (max_expiries = m P) holds them all, whatever n_path -- the slice workspace alone covers 16 columns pairs
    const size_t fused_sets = static_cast<size_t>(wave_rows(n_path)) * 2 * static_cast<size_t>(max_expiries) * sizeof(double);
    if (fused_sets > ws) ws = fused_sets;
    s->ws_bytes = ws;
    const size_t nb = n_path * sizeof(double);
    hipError_t e = hipSuccess;
    if (rc == SVMC_OK && s->owns_stream) e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (rc == SVMC_OK && e == hipSuccess && s->owns_state) e = hipMalloc(reinterpret_cast<void **>(&s->x), nb);
    if (rc == SVMC_OK && e == hipSuccess && s->owns_state) e = hipMalloc(reinterpret_cast<void **>(&s->vol), nb);
    if (rc == SVMC_OK && e == hipSuccess && s->owns_state) e = hipMalloc(reinterpret_cast<void **>(&s->qvar), nb);
    if (rc == SVMC_OK && e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s->snap), 2 * static_cast<size_t>(max_expiries) * nb);
    if (rc == SVMC_OK && e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s->spot), 2 * static_cast<size_t>(max_expiries) * sizeof(double));
    if (rc == SVMC_OK && e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s->sums), 3 * max_strikes_total * sizeof(double));
    if (rc == SVMC_OK && e == hipSuccess) e = hipMalloc(&s->ws, ws);
    s->spot_ws_bytes = (fused_sets > 2 * sizeof(double)) ? fused_sets : 2 * sizeof(double);
    if (rc == SVMC_OK && e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s->spot_ws), s->spot_ws_bytes);
    if (rc == SVMC_OK && e == hipSuccess)
        e = hipHostMalloc(reinterpret_cast<void **>(&s->sums_pinned), 3 * max_strikes_total * sizeof(double), hipHostMallocDefault);
    if (rc != SVMC_OK || e != hipSuccess) {
        session_release(s);
        return rc != SVMC_OK ? rc : fail(SVMC_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
    }
    *session = reinterpret_cast<svmc_session_t>(s);
    return SVMC_OK;
}

int svmc_session_set_comm(svmc_session_t session, svmc_comm_t comm, int rank, int world, uint64_t n_path_total,
                          uint64_t path_offset)
{
    Session *s = reinterpret_cast<Session *>(session);
    SVMC_REQUIRE(s != nullptr, "svmc_session_set_comm: null session");
    s->reduce_fn = nullptr;
    s->reduce_user = nullptr;
    if (comm == nullptr) {                     // back to a single-GPU session
        s->comm = nullptr;
        s->rank = 0;
        s->world = 1;
        s->n_total = 0;
        s->path_offset = 0;
        return SVMC_OK;
    }
    SVMC_REQUIRE(world >= 1 && rank >= 0 && rank < world, "svmc_session_set_comm: need 0 <= rank < world");
    SVMC_REQUIRE(path_offset + s->n_path <= n_path_total, "svmc_session_set_comm: the session's paths exceed the job");
    s->comm = comm;
    s->rank = rank;
    s->world = world;
    s->n_total = n_path_total;
    s->path_offset = path_offset;
    return SVMC_OK;
}

int svmc_session_set_reducer(svmc_session_t session, svmc_all_reduce_fn fn, void *user, int rank, int world,
                             uint64_t n_path_total, uint64_t path_offset)
{
    Session *s = reinterpret_cast<Session *>(session);
    SVMC_REQUIRE(s != nullptr, "svmc_session_set_reducer: null session");
    if (fn == nullptr) return svmc_session_set_comm(session, nullptr, 0, 1, 0, 0);
    SVMC_REQUIRE(world >= 1 && rank >= 0 && rank < world, "svmc_session_set_reducer: need 0 <= rank < world");
    SVMC_REQUIRE(path_offset + s->n_path <= n_path_total, "svmc_session_set_reducer: the session's paths exceed the job");
    s->comm = nullptr;
    s->reduce_fn = fn;
    s->reduce_user = user;
    s->rank = rank;
    s->world = world;
    s->n_total = n_path_total;
    s->path_offset = path_offset;
    return SVMC_OK;
}

int svmc_session_time_stepping(svmc_session_t session, int enable)
{
    Session *s = reinterpret_cast<Session *>(session);
    SVMC_REQUIRE(s != nullptr, "svmc_session_time_stepping: null session");
    if (enable && s->ev0 == nullptr) {
        SVMC_HIP_TRY(hipEventCreate(&s->ev0));
        SVMC_HIP_TRY(hipEventCreate(&s->ev1));
    }
    s->time_stepping = enable != 0;
    s->last_stepping_ms = -1.0f;
    return SVMC_OK;
}

int svmc_session_last_stepping_ms(svmc_session_t session, float *ms)
{
    Session *s = reinterpret_cast<Session *>(session);
    SVMC_REQUIRE(s != nullptr && ms != nullptr, "svmc_session_last_stepping_ms: null argument");
    *ms = s->last_stepping_ms;
    return SVMC_OK;
}

int svmc_session_destroy(svmc_session_t session)
{
    session_release(reinterpret_cast<Session *>(session));
    return SVMC_OK;
}

int svmc_logsv_chain_price(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                           const double *discfactors_host, const double *vol_backbone_etas_host, int n_expiries,
                           const double *strikes_host, const int8_t *types_host, const size_t *strike_offsets_host,
                           double v0, double theta, double kappa1, double kappa2, double beta, double volvol,
                           int is_spot_measure, int nb_steps_per_year, int variable_type, uint64_t seed,
                           uint32_t call_id, double *prices_host, double *stderrs_host)
{
    const char *fn = "svmc_logsv_chain_price";
    Session *s = reinterpret_cast<Session *>(session);
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    // the stepping of :832-865 (a single expiry: the plain slice kernel -- the same bits, the one bench.py profiles)
    const Stepped st = single_step(fn, s, c, nb_steps_per_year, variable_type, prices_host, stderrs_host, true, true,
                                   [&](const int *nbs, const double *dts, double *qsnap, double *spot, void *ws, size_t ws_bytes) {
        return logsv_step_partials(v0, s->x, s->vol, s->qvar, s->n_path, c.m, nbs, dts, vol_backbone_etas_host, c.forwards, theta, kappa1,
                                   kappa2, beta, volvol, is_spot_measure, seed, call_id, s->path_offset, s->snap, qsnap, spot, ws,
                                   ws_bytes, s->stream);
    });
    return st.rc ? st.rc : reduce_and_finalize(s, c, variable_type, prices_host, stderrs_host, st.pending);
}

int svmc_logsv_chain_price_fixed(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                 const double *discfactors_host, const double *vol_backbone_etas_host, int n_expiries,
                                 const double *strikes_host, const int8_t *types_host, const size_t *strike_offsets_host,
                                 double v0, double theta, double kappa1, double kappa2, double beta, double volvol,
                                 int is_spot_measure, int variable_type, const double *const *W0s, const double *const *W1s,
                                 const int *nb_steps_host, const double *dts_host, size_t ldw, double *prices_host,
                                 double *stderrs_host)
{
    return svmc_logsv_chain_price_fixed_iv(session, ttms_host, forwards_host, discfactors_host, vol_backbone_etas_host,
                                           n_expiries, strikes_host, types_host, strike_offsets_host, v0, theta, kappa1, kappa2,
                                           beta, volvol, is_spot_measure, variable_type, W0s, W1s, nb_steps_host, dts_host, ldw,
                                           prices_host, stderrs_host, nullptr);
}

int svmc_logsv_chain_price_fixed_iv(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                    const double *discfactors_host, const double *vol_backbone_etas_host, int n_expiries,
                                    const double *strikes_host, const int8_t *types_host, const size_t *strike_offsets_host,
                                    double v0, double theta, double kappa1, double kappa2, double beta, double volvol,
                                    int is_spot_measure, int variable_type, const double *const *W0s,
                                    const double *const *W1s, const int *nb_steps_host, const double *dts_host, size_t ldw,
                                    double *prices_host, double *stderrs_host, double *ivols_host)
{
    const char *fn = "svmc_logsv_chain_price_fixed";
    Session *s = reinterpret_cast<Session *>(session);
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    if (int rc = check_chain(fn, s, c, variable_type, prices_host, stderrs_host)) return rc;
    SVMC_REQUIRE(W0s && W1s && nb_steps_host && dts_host, "svmc_logsv_chain_price_fixed: null randoms / grids");
    const size_t n = s->n_path;
    if (s->use_graphs && !s->sharded()) {
        // ---- replay path: the launch structure is captured once per (chain, randoms) and replayed per parameter set
        for (int i = 0; i < c.m; ++i)
            SVMC_REQUIRE(dts_host[i] > 0.0 && nb_steps_host[i] > 0, "svmc_logsv_chain_price_fixed: dt and nb_steps must be positive");
        const int want_iv = (ivols_host != nullptr && variable_type == SVMC_LOG_RETURN) ? 1 : 0;
        const std::vector<unsigned char> key = fixed_key(c, 1, variable_type, want_iv, ldw, W0s, W1s, nb_steps_host);
        FixedGraph &g = s->fixed;
        std::vector<double> shifts;
        payoff_shifts_of(c, variable_type, shifts);
        auto enqueue = [&]() -> int {
            SVMC_HIP_TRY(hipMemcpyAsync(g.params_dev, g.params_host, g.params_doubles * sizeof(double), hipMemcpyHostToDevice, s->stream));
            if (c.m <= MAX_FUSED_SLICES) {
                // the whole chain in one launch: state initialised in the kernel (:1128-1130), slice loop inside (:1136-1160)
                double *qsnaps = (variable_type == SVMC_Q_VAR) ? s->snap + static_cast<size_t>(c.m) * n : nullptr;
                if (int rc = logsv_chain_w_indirect(s->x, s->vol, s->qvar, n, c.m, nb_steps_host, g.params_dev + 1, g.params_dev, W0s,
                                                    W1s, ldw, c.forwards, s->snap, qsnaps, s->spot, s->ws, s->ws_bytes, s->stream))
                    return rc;
            } else {
                if (int rc = fill_state_indirect(s->x, s->vol, s->qvar, n, g.params_dev, s->stream)) return rc;      // :1128-1130
                for (int i = 0; i < c.m; ++i) {                                                                        // :1136-1160
                    double *qsnap = (variable_type == SVMC_Q_VAR) ? s->snap + static_cast<size_t>(c.m + i) * n : nullptr;
                    if (int rc = logsv_slice_w_indirect(s->x, s->vol, s->qvar, n, nb_steps_host[i],
                                                        g.params_dev + 1 + static_cast<size_t>(i) * LOGSV_CONSTS_DOUBLES, W0s[i], W1s[i],
                                                        ldw, c.forwards[i], s->snap + static_cast<size_t>(i) * n, qsnap, s->spot + 2 * i,
                                                        s->ws, s->ws_bytes, s->stream))
                        return rc;
                }
            }
            if (int rc = enqueue_payoff_sums_of_set(s, c, variable_type, shifts, 0, 1)) return rc;
            return enqueue_results_home(s, g);
        };
        if (g.key != key)
            if (int rc = graph_prepare(g, key, c, shifts, 1, LOGSV_CONSTS_DOUBLES, want_iv)) return rc;
        if (g.exec == nullptr)
            if (int rc = graph_capture(s, g, fn, enqueue)) return rc;
        const double set[6] = {v0, theta, kappa1, kappa2, beta, volvol};
        fill_params<logsv_consts_to_doubles, LOGSV_CONSTS_DOUBLES>(g.params_host, c, 1, set, vol_backbone_etas_host, 0, dts_host,
                                                                   is_spot_measure);
        SVMC_HIP_TRY(hipGraphLaunch(g.exec, s->stream));
        SVMC_HIP_TRY(hipStreamSynchronize(s->stream));
        ++s->graph_launches;
        return finish_sets(s, c, g.sums_host, shifts, 1, variable_type, prices_host, stderrs_host, ivols_host, g.ivols_host);
    }
    if (int rc = svmc_fill_state(s->x, s->vol, s->qvar, n, 0.0, v0, 0.0, s->stream)) return rc;           // :1128-1130
    for (int i = 0; i < c.m; ++i) {                                                                       // :1136-1160
        const double eta = vol_backbone_etas_host ? vol_backbone_etas_host[i] : 1.0;
        double *qsnap = (variable_type == SVMC_Q_VAR) ? s->snap + static_cast<size_t>(c.m + i) * n : nullptr;
        if (int rc = svmc_logsv_slice_w(s->x, s->vol, s->qvar, n, nb_steps_host[i], dts_host[i], theta, kappa1, kappa2,
                                        beta, volvol, eta, is_spot_measure, W0s[i], W1s[i], ldw, c.forwards[i],
                                        s->snap + static_cast<size_t>(i) * n, qsnap, s->spot + 2 * i, s->ws, s->ws_bytes,
                                        s->stream))
            return rc;
    }
    if (int rc = reduce_and_finalize(s, c, variable_type, prices_host, stderrs_host, false)) return rc;
    if (ivols_host != nullptr) implied_vols_on_host(c, variable_type, prices_host, ivols_host);
    return SVMC_OK;
}

int svmc_logsv_chain_price_fixed_sets(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                      const double *discfactors_host, int n_expiries, const double *strikes_host,
                                      const int8_t *types_host, const size_t *strike_offsets_host, int n_sets,
                                      const double *params_host, int is_spot_measure, int variable_type,
                                      const double *const *W0s, const double *const *W1s, const int *nb_steps_host,
                                      const double *dts_host, size_t ldw, double *prices_host, double *stderrs_host,
                                      double *ivols_host)
{
    const char *fn = "svmc_logsv_chain_price_fixed_sets";
    Session *s = reinterpret_cast<Session *>(session);
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    if (int rc = check_chain(fn, s, c, variable_type, prices_host, stderrs_host)) return rc;
    SVMC_REQUIRE(W0s && W1s && nb_steps_host && dts_host && params_host, "svmc_logsv_chain_price_fixed_sets: null randoms / grids / parameters");
    SVMC_REQUIRE(n_sets >= 1, "svmc_logsv_chain_price_fixed_sets: n_sets must be positive");
    const size_t K = c.offsets[c.m], row = 6 + static_cast<size_t>(c.m);          // doubles per parameter set
    // the routes without a multi-set graph (one set, more sets than a launch takes, graphs off, a communicator attached, a
    // session not sized for n_sets chains): the sets one after the other through the single-set entry -- the same numbers
    const bool batched = s->use_graphs && !s->sharded() && n_sets >= 2 && n_sets <= MAX_FUSED_SETS && c.m <= MAX_FUSED_SLICES &&
                         c.m * n_sets <= s->max_expiries && K * static_cast<size_t>(n_sets) <= s->max_strikes &&
                         static_cast<size_t>(wave_rows(s->n_path)) * 2 * static_cast<size_t>(c.m) * n_sets * sizeof(double) <= s->ws_bytes;
    if (!batched) {
        for (int q = 0; q < n_sets; ++q) {
            const double *pr = params_host + row * q;
            if (int rc = svmc_logsv_chain_price_fixed_iv(session, ttms_host, forwards_host, discfactors_host, pr + 6, n_expiries,
                                                         strikes_host, types_host, strike_offsets_host, pr[0], pr[1], pr[2], pr[3],
                                                         pr[4], pr[5], is_spot_measure, variable_type, W0s, W1s, nb_steps_host,
                                                         dts_host, ldw, prices_host + K * q, stderrs_host + K * q,
                                                         ivols_host ? ivols_host + K * q : nullptr))
                return rc;
        }
        return SVMC_OK;
    }
    const size_t n = s->n_path;
    const int P = n_sets;
    for (int i = 0; i < c.m; ++i)
        SVMC_REQUIRE(dts_host[i] > 0.0 && nb_steps_host[i] > 0, "svmc_logsv_chain_price_fixed_sets: dt and nb_steps must be positive");
    const int want_iv = (ivols_host != nullptr && variable_type == SVMC_LOG_RETURN) ? 1 : 0;
    const std::vector<unsigned char> key = fixed_key(c, P, variable_type, want_iv, ldw, W0s, W1s, nb_steps_host);
    FixedGraph &g = s->fixed_sets;
    std::vector<double> shifts;
    payoff_shifts_of(c, variable_type, shifts);
    auto enqueue = [&]() -> int {
        SVMC_HIP_TRY(hipMemcpyAsync(g.params_dev, g.params_host, g.params_doubles * sizeof(double), hipMemcpyHostToDevice, s->stream));
        double *qsnaps = (variable_type == SVMC_Q_VAR) ? s->snap + static_cast<size_t>(c.m) * P * n : nullptr;
        if (int rc = logsv_chain_w_sets(n, P, c.m, nb_steps_host, g.params_dev + P, g.params_dev, W0s, W1s, ldw, c.forwards, s->snap,
                                        qsnaps, s->spot, s->ws, s->ws_bytes, s->stream))
            return rc;
        if (int rc = enqueue_payoff_sums_of_sets(s, c, variable_type, shifts, P)) return rc;
        return enqueue_results_home(s, g);
    };
    if (g.key != key)
        if (int rc = graph_prepare(g, key, c, shifts, P, LOGSV_CONSTS_DOUBLES, want_iv)) return rc;
    if (g.exec == nullptr)
        if (int rc = graph_capture(s, g, fn, enqueue)) return rc;
    fill_params<logsv_consts_to_doubles, LOGSV_CONSTS_DOUBLES>(g.params_host, c, P, params_host, params_host + 6, row, dts_host,
                                                               is_spot_measure);
    SVMC_HIP_TRY(hipGraphLaunch(g.exec, s->stream));
    SVMC_HIP_TRY(hipStreamSynchronize(s->stream));
    ++s->graph_launches;
    return finish_sets(s, c, g.sums_host, shifts, P, variable_type, prices_host, stderrs_host, ivols_host, g.ivols_host);
}

int svmc_logsv_chain_price_frozen_sets(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                       const double *discfactors_host, int n_expiries, const double *strikes_host,
                                       const int8_t *types_host, const size_t *strike_offsets_host, int n_sets,
                                       const double *params_host, int is_spot_measure, int variable_type,
                                       const int *nb_steps_host, const double *dts_host, uint64_t seed, uint32_t call_id,
                                       double *prices_host, double *stderrs_host, double *ivols_host)
{
    const char *fn = "svmc_logsv_chain_price_frozen_sets";
    Session *s = reinterpret_cast<Session *>(session);
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    if (int rc = check_chain(fn, s, c, variable_type, prices_host, stderrs_host)) return rc;
    SVMC_REQUIRE(nb_steps_host && dts_host && params_host, std::string(fn) + ": null grids / parameters");
    SVMC_REQUIRE(n_sets >= 1, std::string(fn) + ": n_sets must be positive");
    SVMC_REQUIRE(call_id < (1u << 24), std::string(fn) + ": call_id must fit 24 bits");
    const size_t K = c.offsets[c.m], row = 6 + static_cast<size_t>(c.m);          // doubles per parameter set
    for (int i = 0; i < c.m; ++i)
        SVMC_REQUIRE(dts_host[i] > 0.0 && nb_steps_host[i] > 0, std::string(fn) + ": dt and nb_steps must be positive");
    if (n_sets > MAX_FUSED_SETS) {              // more sets than a launch takes: in launches of MAX_FUSED_SETS
        for (int q = 0; q < n_sets; q += MAX_FUSED_SETS) {
            const int P = (n_sets - q < MAX_FUSED_SETS) ? n_sets - q : MAX_FUSED_SETS;
            if (int rc = svmc_logsv_chain_price_frozen_sets(session, ttms_host, forwards_host, discfactors_host, n_expiries,
                                                            strikes_host, types_host, strike_offsets_host, P, params_host + row * q,
                                                            is_spot_measure, variable_type, nb_steps_host, dts_host, seed, call_id,
                                                            prices_host + K * q, stderrs_host + K * q,
                                                            ivols_host ? ivols_host + K * q : nullptr))
                return rc;
        }
        return SVMC_OK;
    }
    const int P = n_sets;
    SVMC_REQUIRE(c.m <= MAX_FUSED_SLICES, std::string(fn) + ": at most 16 expiries");
    SVMC_REQUIRE(c.m * P <= s->max_expiries && K * static_cast<size_t>(P) <= s->max_strikes &&
                     static_cast<size_t>(wave_rows(s->n_path)) * 2 * static_cast<size_t>(c.m) * P * sizeof(double) <= s->ws_bytes,
                 std::string(fn) + ": the session must be created for n_sets chains (max_expiries >= n_sets x n_expiries, "
                                   "max_strikes_total >= n_sets x sum K_i)");
    const size_t n = s->n_path;
    const bool graph = s->use_graphs && !s->sharded();
    const int want_iv = (ivols_host != nullptr && variable_type == SVMC_LOG_RETURN) ? 1 : 0;
    // everything that shapes the launches; the model constants travel in the parameter block
    std::vector<unsigned char> key = chain_key(c, P, variable_type, want_iv);
    const int sharded = s->sharded() ? 1 : 0;
    key_append(key, &sharded, 1);
    key_append(key, &seed, 1);
    key_append(key, &call_id, 1);
    key_append(key, &s->path_offset, 1);
    key_append(key, nb_steps_host, c.m);
    FixedGraph &g = s->frozen[P];
    std::vector<double> shifts;
    payoff_shifts_of(c, variable_type, shifts);
    // the chain's launches, queued on the session's stream: captured into the graph, or issued as they are (a communicator
    // attached, graphs off) with the two all-reduces between them
    auto enqueue = [&]() -> int {
        SVMC_HIP_TRY(hipMemcpyAsync(g.params_dev, g.params_host, g.params_doubles * sizeof(double), hipMemcpyHostToDevice, s->stream));
        double *qsnaps = (variable_type == SVMC_Q_VAR) ? s->snap + static_cast<size_t>(c.m) * P * n : nullptr;
        // (a captured launch never carries the thread's clock probe: the graph outlives the probe's buffer)
        if (int rc = logsv_chain_rng_sets(n, P, c.m, nb_steps_host, g.params_dev + P, g.params_dev, c.forwards, seed, call_id,
                                          s->path_offset, s->snap, qsnaps, s->spot, s->ws, s->ws_bytes, s->stream, !graph))
            return rc;
        if (int rc = all_reduce(s, s->spot, 2 * static_cast<size_t>(c.m) * P)) return rc;
        if (int rc = enqueue_payoff_sums_of_sets(s, c, variable_type, shifts, P)) return rc;
        if (int rc = all_reduce(s, s->sums, g.sums_doubles)) return rc;
        return enqueue_results_home(s, g);
    };
    if (g.key != key)
        if (int rc = graph_prepare(g, key, c, shifts, P, LOGSV_FAST_CONSTS_DOUBLES, want_iv)) return rc;
    if (graph && g.exec == nullptr)        // captured at the first replayed call of this shape (an un-replayed call may come first)
        if (int rc = graph_capture(s, g, fn, enqueue)) return rc;
    fill_params<logsv_fast_to_doubles, LOGSV_FAST_CONSTS_DOUBLES>(g.params_host, c, P, params_host, params_host + 6, row, dts_host,
                                                                  is_spot_measure);
    if (graph) {
        SVMC_HIP_TRY(hipGraphLaunch(g.exec, s->stream));
        ++s->graph_launches;
    } else if (int rc = enqueue()) {
        return rc;
    }
    SVMC_HIP_TRY(hipStreamSynchronize(s->stream));
    return finish_sets(s, c, g.sums_host, shifts, P, variable_type, prices_host, stderrs_host, ivols_host, g.ivols_host);
}

int svmc_session_use_graphs(svmc_session_t session, int enable)
{
    Session *s = reinterpret_cast<Session *>(session);
    SVMC_REQUIRE(s != nullptr, "svmc_session_use_graphs: null session");
    s->use_graphs = enable != 0;
    return SVMC_OK;
}

int svmc_session_graph_launches(svmc_session_t session, size_t *count)
{
    Session *s = reinterpret_cast<Session *>(session);
    SVMC_REQUIRE(s != nullptr && count != nullptr, "svmc_session_graph_launches: null pointer");
    *count = s->graph_launches;
    return SVMC_OK;
}

int svmc_heston_chain_price(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                            const double *discfactors_host, int n_expiries, const double *strikes_host,
                            const int8_t *types_host, const size_t *strike_offsets_host, double v0, double theta,
                            double kappa, double rho, double volvol, int scheme, int nb_steps_per_year,
                            int variable_type, uint64_t seed, uint32_t call_id, double *prices_host,
                            double *stderrs_host)
{
    const char *fn = "svmc_heston_chain_price";
    Session *s = reinterpret_cast<Session *>(session);
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    // the stepping of :303-329
    const Stepped st = single_step(fn, s, c, nb_steps_per_year, variable_type, prices_host, stderrs_host, true, true,
                                   [&](const int *nbs, const double *dts, double *qsnap, double *spot, void *ws, size_t ws_bytes) {
        return heston_step_partials(v0, s->x, s->vol, s->qvar, s->n_path, c.m, nbs, dts, c.forwards, theta, kappa, rho, volvol, scheme, seed,
                                    call_id, s->path_offset, s->snap, qsnap, spot, ws, ws_bytes, s->stream);
    });
    return st.rc ? st.rc : reduce_and_finalize(s, c, variable_type, prices_host, stderrs_host, st.pending);
}

int svmc_logsv_chain_price_cmc(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                               const double *discfactors_host, const double *vol_backbone_etas_host, int n_expiries,
                               const double *strikes_host, const int8_t *types_host, const size_t *strike_offsets_host, double v0,
                               double theta, double kappa1, double kappa2, double beta, double volvol, int is_spot_measure,
                               int nb_steps_per_year, int recenter, uint64_t seed, uint32_t call_id, double *prices_host,
                               double *stderrs_host, double *stats_host)
{
    Session *s = reinterpret_cast<Session *>(session);
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    return chain_price_cmc("svmc_logsv_chain_price_cmc", s, c, nb_steps_per_year, recenter, prices_host, stderrs_host, nullptr, stats_host,
                           [&](const int *nbs, const double *dts, double *mu_snap, double *cv_snap) {
        return logsv_cmc_step_from(v0, s->x, s->cmc_cv, s->vol, s->qvar, s->n_path, c.m, nbs, dts, vol_backbone_etas_host, theta, kappa1,
                                   kappa2, beta, volvol, is_spot_measure, seed, call_id, s->path_offset, mu_snap, cv_snap, s->stream);
    });
}

int svmc_heston_chain_price_cmc(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                const double *discfactors_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                const size_t *strike_offsets_host, double v0, double theta, double kappa, double rho, double volvol,
                                int nb_steps_per_year, int recenter, uint64_t seed, uint32_t call_id, double *prices_host,
                                double *stderrs_host, double *stats_host)
{
    Session *s = reinterpret_cast<Session *>(session);
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    return chain_price_cmc("svmc_heston_chain_price_cmc", s, c, nb_steps_per_year, recenter, prices_host, stderrs_host, nullptr, stats_host,
                           [&](const int *nbs, const double *dts, double *mu_snap, double *cv_snap) {
        return heston_cmc_step_from(v0, s->x, s->cmc_cv, s->vol, s->qvar, s->n_path, c.m, nbs, dts, theta, kappa, rho, volvol, seed,
                                    call_id, s->path_offset, mu_snap, cv_snap, s->stream);
    });
}

int svmc_logsv_chain_price_cmc_greeks(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                      const double *discfactors_host, const double *vol_backbone_etas_host, int n_expiries,
                                      const double *strikes_host, const int8_t *types_host, const size_t *strike_offsets_host, double v0,
                                      double theta, double kappa1, double kappa2, double beta, double volvol, int is_spot_measure,
                                      int nb_steps_per_year, int recenter, uint64_t seed, uint32_t call_id, double *greeks_host,
                                      double *stats_host)
{
    const char *fn = "svmc_logsv_chain_price_cmc_greeks";
    SVMC_REQUIRE(greeks_host != nullptr && strike_offsets_host != nullptr && n_expiries >= 1, std::string(fn) + ": null pointer or no expiries");
    Session *s = reinterpret_cast<Session *>(session);
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    return chain_price_cmc(fn, s, c, nb_steps_per_year, recenter, greeks_host, greeks_host + strike_offsets_host[n_expiries], greeks_host,
                           stats_host, [&](const int *nbs, const double *dts, double *mu_snap, double *cv_snap) {
        return logsv_cmc_step_from(v0, s->x, s->cmc_cv, s->vol, s->qvar, s->n_path, c.m, nbs, dts, vol_backbone_etas_host, theta, kappa1,
                                   kappa2, beta, volvol, is_spot_measure, seed, call_id, s->path_offset, mu_snap, cv_snap, s->stream);
    });
}

int svmc_heston_chain_price_cmc_greeks(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                       const double *discfactors_host, int n_expiries, const double *strikes_host,
                                       const int8_t *types_host, const size_t *strike_offsets_host, double v0, double theta, double kappa,
                                       double rho, double volvol, int nb_steps_per_year, int recenter, uint64_t seed, uint32_t call_id,
                                       double *greeks_host, double *stats_host)
{
    const char *fn = "svmc_heston_chain_price_cmc_greeks";
    SVMC_REQUIRE(greeks_host != nullptr && strike_offsets_host != nullptr && n_expiries >= 1, std::string(fn) + ": null pointer or no expiries");
    Session *s = reinterpret_cast<Session *>(session);
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    return chain_price_cmc(fn, s, c, nb_steps_per_year, recenter, greeks_host, greeks_host + strike_offsets_host[n_expiries], greeks_host,
                           stats_host, [&](const int *nbs, const double *dts, double *mu_snap, double *cv_snap) {
        return heston_cmc_step_from(v0, s->x, s->cmc_cv, s->vol, s->qvar, s->n_path, c.m, nbs, dts, theta, kappa, rho, volvol, seed,
                                    call_id, s->path_offset, mu_snap, cv_snap, s->stream);
    });
}

int svmc_hawkesjd_chain_price(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                              const double *discfactors_host, int n_expiries, const double *strikes_host,
                              const int8_t *types_host, const size_t *strike_offsets_host, const double *params_host,
                              int nb_steps_per_year, int variable_type, uint64_t seed, uint32_t call_id, double *prices_host,
                              double *stderrs_host)
{
    const char *fn = "svmc_hawkesjd_chain_price";
    Session *s = reinterpret_cast<Session *>(session);
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    const auto check = [&]() -> int {          // (the reference would price the log-return as a variance, :701-707)
        if (variable_type != SVMC_LOG_RETURN) return fail(SVMC_ERR_UNSUPPORTED_VARIABLE, "svmc_hawkesjd_chain_price: LOG_RETURN only");
        SVMC_REQUIRE(params_host != nullptr, "svmc_hawkesjd_chain_price: null params");
        return SVMC_OK;
    };
    // the stepping of :680-700; the session's vol / qvar slots hold lambda_p / lambda_m
    const Stepped st = single_step(fn, s, c, nb_steps_per_year, variable_type, prices_host, stderrs_host, true, true,
                                   [&](const int *nbs, const double *dts, double *, double *spot, void *ws, size_t ws_bytes) {
        return hawkes_step_partials(params_host, s->x, s->vol, s->qvar, s->n_path, c.m, nbs, dts, c.forwards, seed, call_id,
                                    s->path_offset, s->snap, spot, ws, ws_bytes, s->stream);
    }, check);
    return st.rc ? st.rc : reduce_and_finalize(s, c, variable_type, prices_host, stderrs_host, st.pending);
}

int svmc_hawkesjd_chain_price_tilted(svmc_session_t session, const double *ttms_host, const double *forwards_host, int n_expiries,
                                     const double *strikes_host, const int8_t *types_host, const size_t *strike_offsets_host,
                                     const double *params_host, int nb_steps_per_year, uint64_t seed, uint32_t call_id,
                                     const double *gammas_host, int n_gammas, int recenter, double *prices_host, double *stderrs_host,
                                     double *stats_host)
{
    const char *fn = "svmc_hawkesjd_chain_price_tilted";
    Session *s = reinterpret_cast<Session *>(session);
    // the chain's own checks (the discount factors play no part: the prices are undiscounted)
    const ChainView c = {n_expiries, ttms_host, forwards_host, nullptr, strikes_host, types_host, strike_offsets_host};
    TiltedBlock out;
    std::vector<double> shifts;
    const auto check = [&]() -> int {
        SVMC_REQUIRE(!s->sharded(), std::string(fn) + ": single-device sessions only");
        SVMC_REQUIRE(params_host != nullptr && gammas_host != nullptr && stats_host != nullptr, std::string(fn) + ": null pointer");
        return SVMC_OK;
    };
    const auto prepare = [&]() -> int {        // the gammas' checks come after the step count's; then the shifts and the pinned block
        if (int rc = check_tilted(fn, c, gammas_host, static_cast<size_t>(n_gammas), n_gammas, stats_host)) return rc;
        size_t need_ws = 0;
        if (int rc = svmc_payoff_workspace_bytes(&need_ws)) return rc;
        if (s->ws_bytes < need_ws) return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": the session's workspace is too small");
        payoff_shifts_of(c, SVMC_LOG_RETURN, shifts);
        return tilted_block(s, c, n_gammas, 1, out);
    };
    // svmc_hawkesjd_chain_price's stepping launch, once for every gamma; its spot sums are reduced only where the recentring reads them
    const Stepped st = single_step(fn, s, c, nb_steps_per_year, SVMC_LOG_RETURN, prices_host, stderrs_host, false, !recenter,
                                   [&](const int *nbs, const double *dts, double *, double *spot, void *ws, size_t ws_bytes) {
        return hawkes_step_partials(params_host, s->x, s->vol, s->qvar, s->n_path, c.m, nbs, dts, c.forwards, seed, call_id,
                                    s->path_offset, s->snap, spot, ws, ws_bytes, s->stream);
    }, check, prepare);
    if (st.rc) return st.rc;
    const SnapshotRows r = snapshot_rows(s, c, 0, 1);
    if (int rc = svmc_tilted_payoff_chain(r.x.data(), s->n_path, c.forwards, c.m, c.strikes, c.types, shifts.data(), c.offsets, gammas_host,
                                          n_gammas, recenter, recenter ? s->spot : nullptr, out.prices(0), out.stderrs(0), out.stats(0),
                                          s->ws, s->ws_bytes, reinterpret_cast<svmc_stream_t>(s->stream)))
        return rc;
    SVMC_HIP_TRY(hipStreamSynchronize(s->stream));
    stepping_read(s);
    out.copy_home(0, prices_host, stderrs_host, stats_host);
    return SVMC_OK;
}

// conditional Monte Carlo for the Hawkes jump-diffusion (row f16): chain_price_cmc on the session's x / vol / qvar as (mu, lambda_p,
// lambda_m); every cv row is one double (hawkes_cond_step_from), the tail is the one of rows f11 / f13
int svmc_hawkesjd_chain_price_cmc(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                  const double *discfactors_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                  const size_t *strike_offsets_host, const double *params_host, int nb_steps_per_year, int recenter,
                                  uint64_t seed, uint32_t call_id, double *prices_host, double *stderrs_host, double *stats_host)
{
    const char *fn = "svmc_hawkesjd_chain_price_cmc";
    if (int rc = hawkes_check_params(fn, params_host)) return rc;
    Session *s = reinterpret_cast<Session *>(session);
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    return chain_price_cmc(fn, s, c, nb_steps_per_year, recenter, prices_host, stderrs_host, nullptr, stats_host,
                           [&](const int *nbs, const double *dts, double *mu_snap, double *cv_snap) {
        return hawkes_cond_step_from(fn, params_host, s->x, s->vol, s->qvar, s->n_path, c.m, nbs, dts, seed, call_id, s->path_offset,
                                     mu_snap, cv_snap, s->stream);
    });
}

int svmc_hawkesjd_chain_price_cmc_greeks(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                         const double *discfactors_host, int n_expiries, const double *strikes_host,
                                         const int8_t *types_host, const size_t *strike_offsets_host, const double *params_host,
                                         int nb_steps_per_year, int recenter, uint64_t seed, uint32_t call_id, double *greeks_host,
                                         double *stats_host)
{
    const char *fn = "svmc_hawkesjd_chain_price_cmc_greeks";
    SVMC_REQUIRE(greeks_host != nullptr && strike_offsets_host != nullptr && n_expiries >= 1, std::string(fn) + ": null pointer or no expiries");
    if (int rc = hawkes_check_params(fn, params_host)) return rc;
    Session *s = reinterpret_cast<Session *>(session);
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    return chain_price_cmc(fn, s, c, nb_steps_per_year, recenter, greeks_host, greeks_host + strike_offsets_host[n_expiries], greeks_host,
                           stats_host, [&](const int *nbs, const double *dts, double *mu_snap, double *cv_snap) {
        return hawkes_cond_step_from(fn, params_host, s->x, s->vol, s->qvar, s->n_path, c.m, nbs, dts, seed, call_id, s->path_offset,
                                     mu_snap, cv_snap, s->stream);
    });
}

}  // extern "C"

// ---- many jobs of one chain (svmc_logsv_chain_price_many / svmc_heston_chain_price_many / svmc_hawkesjd_chain_price[_tilted]_many)

// (min_ws_bytes: a floor for the payoff workspace, for a tail other than chain_payoff_and_finish_sets)
static int grow_many(const char *fn, ManyBuffers &mb, size_t n, size_t J, size_t m, size_t K, bool need_q, size_t min_ws_bytes = 0)
{
    const size_t d = sizeof(double), sums = (3 * K * J > 0 ? 3 * K * J : 1) * d;
    const size_t sets_ws = payoff_sets_workspace_bytes(n, K, static_cast<int>(J)), ws = sets_ws > min_ws_bytes ? sets_ws : min_ws_bytes;
    const struct {
        void **p;
        size_t *cap, need;
        bool pinned;
    } bufs[] = {
        {reinterpret_cast<void **>(&mb.snap), &mb.snap_bytes, (need_q ? 2 : 1) * J * m * n * d, false},
        {reinterpret_cast<void **>(&mb.spot_ws), &mb.spot_ws_bytes, static_cast<size_t>(wave_rows(n)) * 2 * m * J * d, false},
        {reinterpret_cast<void **>(&mb.spot), &mb.spot_bytes, 2 * m * J * d, false},
        {reinterpret_cast<void **>(&mb.sums), &mb.sums_bytes, sums, false},
        {&mb.ws, &mb.ws_bytes, ws, false},
        {&mb.table_dev, &mb.table_bytes, many_table_bytes(static_cast<int>(J), static_cast<int>(m)), false},
        {&mb.table_host, &mb.table_host_bytes, many_table_bytes(static_cast<int>(J), static_cast<int>(m)), true},
        {reinterpret_cast<void **>(&mb.sums_pinned), &mb.sums_pinned_bytes, sums, true},
    };
    for (const auto &b : bufs)
        if (hipError_t e = grow(b.p, *b.cap, b.need, b.pinned))
            return fail(SVMC_ERR_HIP, std::string(fn) + ": per-job workspace: " + hipGetErrorString(e));
    return SVMC_OK;
}

// The first half of every many-job driver: the checks (all before any device work; check(): the model's own, once the shared
// ones have found every pointer and size in order), the per-job workspace, then step(nbs, dts, qsnap) -- the model's ONE
// stepping launch of every job into the ManyBuffers -- and the jobs' spot sums (one column reduce).  `shifts` gets the chain's
// payoff shifts.
template <class Check, class Step>
static int many_step(const char *fn, Session *s, const ChainView &c, int n_jobs, const void *params, const uint64_t *seeds,
                     const uint32_t *call_ids, int nb_steps_per_year, int variable_type, const double *prices, const double *stderrs,
                     bool needs_discfactors, size_t min_ws_bytes, std::vector<double> &shifts, Check &&check, Step &&step)
{
    SVMC_REQUIRE(s != nullptr, std::string(fn) + ": null session");
    SVMC_REQUIRE(n_jobs >= 1 && n_jobs <= SVMC_MANY_MAX_JOBS, std::string(fn) + ": n_jobs must be in [1, SVMC_MANY_MAX_JOBS]");
    SVMC_REQUIRE(params && seeds && call_ids && c.ttms && c.forwards && (c.discfactors || !needs_discfactors) && c.strikes && c.types &&
                     c.offsets && prices && stderrs,
                 std::string(fn) + ": null pointer");
    SVMC_REQUIRE(c.m >= 1 && c.m <= MAX_FUSED_SLICES, std::string(fn) + ": 1 to 16 expiries");
    if (c.m > s->max_expiries || c.offsets[c.m] > s->max_strikes)
        return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": the chain exceeds the session (max_expiries / max_strikes_total)");
    SVMC_REQUIRE(!s->sharded(), std::string(fn) + ": no sharded batch: detach the communicator / reducer");
    SVMC_REQUIRE(nb_steps_per_year > 0, std::string(fn) + ": nb_steps_per_year must be positive");
    for (int j = 0; j < n_jobs; ++j) SVMC_REQUIRE(call_ids[j] < (1u << 24), std::string(fn) + ": call_id must fit 24 bits");
    if (int rc = check()) return rc;
    if (int rc = check_chain(fn, s, c, variable_type, prices, stderrs, needs_discfactors)) return rc;
    const size_t n = s->n_path, J = static_cast<size_t>(n_jobs), m = static_cast<size_t>(c.m), K = c.offsets[c.m];
    const bool need_q = variable_type == SVMC_Q_VAR;
    ManyBuffers &mb = s->many;
    if (int rc = grow_many(fn, mb, n, J, m, K, need_q, min_ws_bytes)) return rc;
    std::vector<int> nbs;
    std::vector<double> dts;
    expiry_grids(c, nb_steps_per_year, nbs, dts);
    payoff_shifts_of(c, variable_type, shifts);
    stepping_begin(s);
    if (int rc = step(nbs, dts, need_q ? mb.snap + J * m * n : nullptr)) return rc;
    if (int rc = reduce_spot_partials(mb.spot_ws, n, static_cast<int>(2 * m * J), mb.spot, s->stream)) return rc;
    stepping_end(s);
    return SVMC_OK;
}

// The driver of the plain many-job calls: many_step, then ONE payoff launch and ONE finish launch for all jobs (a payoff launch
// per job where the chain does not fit one), and the host finalisation per job.
template <class Check, class Step>
static int chain_price_many(const char *fn, svmc_session_t session, const ChainView &c, int n_jobs, const void *params,
                            const uint64_t *seeds, const uint32_t *call_ids, int nb_steps_per_year, int variable_type, double *prices,
                            double *stderrs, Check &&check, Step &&step)
{
    Session *s = reinterpret_cast<Session *>(session);
    std::vector<double> shifts;
    if (int rc = many_step(fn, s, c, n_jobs, params, seeds, call_ids, nb_steps_per_year, variable_type, prices, stderrs, true, 0, shifts,
                           check, step))
        return rc;
    const size_t n = s->n_path, J = static_cast<size_t>(n_jobs), m = static_cast<size_t>(c.m), K = c.offsets[c.m];
    const bool need_q = variable_type == SVMC_Q_VAR;
    ManyBuffers &mb = s->many;
    double *qsnap = need_q ? mb.snap + J * m * n : nullptr;
    std::vector<const double *> xs(m), qs(m);
    for (size_t i = 0; i < m; ++i) {
        xs[i] = mb.snap + i * n;
        qs[i] = need_q ? qsnap + i * n : nullptr;
    }
    if (payoff_sets_fit(n, c.m, c.offsets, c.types, n_jobs, mb.ws_bytes)) {
        if (int rc = chain_payoff_and_finish_sets(xs.data(), need_q ? qs.data() : nullptr, n, c.forwards, c.ttms, mb.spot, c.m, c.strikes,
                                                  c.types, shifts.data(), c.offsets, variable_type, mb.ws, mb.ws_bytes, s->stream, n_jobs,
                                                  m * n, m * n, 2 * m, mb.sums, mb.sums_pinned))
            return rc;
    } else {
        // more strike groups than one payoff launch takes: a payoff pass per job, as the single call then runs it
        for (size_t j = 0; j < J; ++j) {
            std::vector<const double *> xj(m), qj(m);
            for (size_t i = 0; i < m; ++i) {
                xj[i] = xs[i] + j * m * n;
                qj[i] = need_q ? qs[i] + j * m * n : nullptr;
            }
            if (int rc = svmc_payoff_sums_chain(xj.data(), need_q ? qj.data() : nullptr, n, c.forwards, c.ttms, mb.spot + 2 * m * j, c.m,
                                                c.strikes, c.types, shifts.data(), c.offsets, variable_type, mb.sums + 3 * K * j, mb.ws,
                                                mb.ws_bytes, reinterpret_cast<svmc_stream_t>(s->stream)))
                return rc;
        }
        SVMC_HIP_TRY(hipMemcpyAsync(mb.sums_pinned, mb.sums, 3 * K * J * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    }
    SVMC_HIP_TRY(hipStreamSynchronize(s->stream));
    stepping_read(s);
    return finish_sets(s, c, mb.sums_pinned, shifts, n_jobs, variable_type, prices, stderrs, nullptr, nullptr);
}

// the step() of the two Hawkes many-job drivers: every job's paths from ONE launch into the ManyBuffers
static auto hawkes_many_stepper(Session *s, const ChainView &c, int n_jobs, const double *params, const uint64_t *seeds, const uint32_t *call_ids)
{
    return [=](const std::vector<int> &nbs, const std::vector<double> &dts, double *) {
        ManyBuffers &mb = s->many;
        return hawkes_chain_rng_many(s->n_path, n_jobs, c.m, nbs.data(), dts.data(), c.forwards, params, seeds, call_ids, s->path_offset,
                                     mb.table_host, mb.table_dev, mb.snap, mb.spot_ws, s->stream);
    };
}

// ---- Monte Carlo chain Greeks (include/svmc.h; the tail: svmc_greeks.hip): many_step with the 1 + 2P rows of `params` on one
// (seed, call id) -- step(nbs, dts, seeds, call_ids) is the model's many-job launch --, then job 0's plain tail -- the launches the many-job driver gives a job, hence the single call's bits -- and
// the Greeks tail on the jobs' rows and spot sums, everything on the session's stream and one synchronise.
template <class Step>
static int chain_price_greeks(const char *fn, Session *s, const ChainView &c, int n_params, const double *params, const double *steps,
                              int nb_steps_per_year, uint64_t seed, uint32_t call_id, double *prices, double *stderrs, double *greeks,
                              double *sens, Step &&step)
{
    SVMC_REQUIRE(n_params >= 0 && n_params <= SVMC_GREEKS_MAX_PARAMS, std::string(fn) + ": n_params must be in [0, SVMC_GREEKS_MAX_PARAMS]");
    SVMC_REQUIRE(greeks != nullptr && (n_params == 0 || sens != nullptr), std::string(fn) + ": null pointer");
    const int P = n_params, J = 1 + 2 * P;
    const std::vector<uint64_t> seeds(J, seed);
    const std::vector<uint32_t> call_ids(J, call_id);
    std::vector<double> shifts;
    if (int rc = many_step(fn, s, c, J, params, seeds.data(), call_ids.data(), nb_steps_per_year, SVMC_LOG_RETURN, prices, stderrs, true, 0,
                           shifts,
                           [&]() -> int {
        if (int rc = check_steps(fn, P, steps, 0)) return rc;
        if (int rc = check_quotes(fn, s->n_path, c.forwards, c.discfactors, c.m, c.strikes, c.types, c.offsets, 1u << 24, 1)) return rc;
        const size_t K = c.offsets[c.m];
        SVMC_HIP_TRY(grow(&s->greeks_ws, s->greeks_ws_bytes, greeks_payoff_workspace_bytes_of(s->n_path, c.m, K, P), false));
        SVMC_HIP_TRY(grow(&s->greeks_pinned, s->greeks_pinned_bytes, greeks_pinned(nullptr, c.m, K, P, nullptr), true));
        return SVMC_OK;
    },
                           [&](const std::vector<int> &nbs, const std::vector<double> &dts, double *) {
        return step(nbs, dts, seeds.data(), call_ids.data());
    }))
        return rc;
    const size_t n = s->n_path, m = static_cast<size_t>(c.m), K = c.offsets[c.m];
    ManyBuffers &mb = s->many;
    std::vector<const double *> rows(static_cast<size_t>(J) * m);
    for (size_t r = 0; r < rows.size(); ++r) rows[r] = mb.snap + r * n;
    if (payoff_sets_fit(n, c.m, c.offsets, c.types, 1, mb.ws_bytes)) {
        if (int rc = chain_payoff_and_finish_sets(rows.data(), nullptr, n, c.forwards, c.ttms, mb.spot, c.m, c.strikes, c.types, shifts.data(),
                                                  c.offsets, SVMC_LOG_RETURN, mb.ws, mb.ws_bytes, s->stream, 1, m * n, m * n, 2 * m, mb.sums,
                                                  mb.sums_pinned))
            return rc;
    } else {
        if (int rc = svmc_payoff_sums_chain(rows.data(), nullptr, n, c.forwards, c.ttms, mb.spot, c.m, c.strikes, c.types, shifts.data(),
                                            c.offsets, SVMC_LOG_RETURN, mb.sums, mb.ws, mb.ws_bytes, reinterpret_cast<svmc_stream_t>(s->stream)))
            return rc;
        SVMC_HIP_TRY(hipMemcpyAsync(mb.sums_pinned, mb.sums, 3 * K * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    }
    GreeksResults out;                                     // (the kernels store the results in the page-locked block themselves)
    greeks_pinned(s->greeks_pinned, c.m, K, P, &out);
    if (int rc = greeks_payoff_enqueue(fn, rows.data(), n, c.forwards, c.discfactors, c.m, c.strikes, c.types, c.offsets, P, steps, mb.spot,
                                       out.base, out.sens, s->greeks_pinned, s->greeks_ws, s->greeks_ws_bytes, s->stream, nullptr))
        return rc;
    SVMC_HIP_TRY(hipStreamSynchronize(s->stream));
    stepping_read(s);
    memcpy(greeks, out.base, SVMC_GREEKS_BASE_ROWS * K * sizeof(double));
    if (P > 0) memcpy(sens, out.sens, static_cast<size_t>(SVMC_GREEKS_SENS_ROWS) * P * K * sizeof(double));
    return finish_sets(s, c, mb.sums_pinned, shifts, 1, SVMC_LOG_RETURN, prices, stderrs, nullptr, nullptr);
}

extern "C" {

int svmc_logsv_chain_price_greeks(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                  const double *discfactors_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                  const size_t *strike_offsets_host, int n_params, const double *params_host, const double *steps_host,
                                  int is_spot_measure, int nb_steps_per_year, uint64_t seed, uint32_t call_id, double *prices_host,
                                  double *stderrs_host, double *greeks_host, double *sens_host)
{
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    Session *s = reinterpret_cast<Session *>(session);
    const int n_jobs = 1 + 2 * n_params;
    return chain_price_greeks("svmc_logsv_chain_price_greeks", s, c, n_params, params_host, steps_host, nb_steps_per_year, seed, call_id,
                              prices_host, stderrs_host, greeks_host, sens_host,
                              [&](const std::vector<int> &nbs, const std::vector<double> &dts, const uint64_t *seeds, const uint32_t *call_ids) {
        ManyBuffers &mb = s->many;
        return logsv_chain_rng_many(s->n_path, n_jobs, c.m, nbs.data(), dts.data(), c.forwards, params_host, is_spot_measure, seeds, call_ids,
                                    s->path_offset, mb.table_host, mb.table_dev, mb.snap, nullptr, mb.spot_ws, s->stream);
    });
}

int svmc_heston_chain_price_greeks(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                   const double *discfactors_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                   const size_t *strike_offsets_host, int n_params, const double *params_host, const double *steps_host,
                                   int scheme, int nb_steps_per_year, uint64_t seed, uint32_t call_id, double *prices_host,
                                   double *stderrs_host, double *greeks_host, double *sens_host)
{
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    Session *s = reinterpret_cast<Session *>(session);
    SVMC_REQUIRE(scheme == SVMC_HESTON_EULER_FLOOR || scheme == SVMC_HESTON_QE, "svmc_heston_chain_price_greeks: unknown scheme");
    const int n_jobs = 1 + 2 * n_params;
    return chain_price_greeks("svmc_heston_chain_price_greeks", s, c, n_params, params_host, steps_host, nb_steps_per_year, seed, call_id,
                              prices_host, stderrs_host, greeks_host, sens_host,
                              [&](const std::vector<int> &nbs, const std::vector<double> &dts, const uint64_t *seeds, const uint32_t *call_ids) {
        ManyBuffers &mb = s->many;
        return heston_chain_rng_many(s->n_path, n_jobs, c.m, nbs.data(), dts.data(), c.forwards, params_host, scheme, seeds, call_ids,
                                     s->path_offset, mb.table_host, mb.table_dev, mb.snap, nullptr, mb.spot_ws, s->stream);
    });
}

}  // extern "C"

extern "C" {

int svmc_logsv_chain_price_many(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                const double *discfactors_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                const size_t *strike_offsets_host, int n_jobs, const double *params_host, const uint64_t *seeds_host,
                                const uint32_t *call_ids_host, int is_spot_measure, int nb_steps_per_year, int variable_type,
                                double *prices_host, double *stderrs_host)
{
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    Session *s = reinterpret_cast<Session *>(session);
    return chain_price_many("svmc_logsv_chain_price_many", session, c, n_jobs, params_host, seeds_host, call_ids_host, nb_steps_per_year,
                            variable_type, prices_host, stderrs_host, [] { return SVMC_OK; },
                            [&](const std::vector<int> &nbs, const std::vector<double> &dts, double *qsnap) {
        ManyBuffers &mb = s->many;
        return logsv_chain_rng_many(s->n_path, n_jobs, c.m, nbs.data(), dts.data(), c.forwards, params_host, is_spot_measure, seeds_host,
                                    call_ids_host, s->path_offset, mb.table_host, mb.table_dev, mb.snap, qsnap, mb.spot_ws, s->stream);
    });
}

int svmc_heston_chain_price_many(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                 const double *discfactors_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                 const size_t *strike_offsets_host, int n_jobs, const double *params_host, const uint64_t *seeds_host,
                                 const uint32_t *call_ids_host, int scheme, int nb_steps_per_year, int variable_type,
                                 double *prices_host, double *stderrs_host)
{
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    Session *s = reinterpret_cast<Session *>(session);
    SVMC_REQUIRE(scheme == SVMC_HESTON_EULER_FLOOR || scheme == SVMC_HESTON_QE, "svmc_heston_chain_price_many: unknown scheme");
    return chain_price_many("svmc_heston_chain_price_many", session, c, n_jobs, params_host, seeds_host, call_ids_host,
                            nb_steps_per_year, variable_type, prices_host, stderrs_host, [] { return SVMC_OK; },
                            [&](const std::vector<int> &nbs, const std::vector<double> &dts, double *qsnap) {
        ManyBuffers &mb = s->many;
        return heston_chain_rng_many(s->n_path, n_jobs, c.m, nbs.data(), dts.data(), c.forwards, params_host, scheme, seeds_host,
                                     call_ids_host, s->path_offset, mb.table_host, mb.table_dev, mb.snap, qsnap, mb.spot_ws, s->stream);
    });
}

int svmc_hawkesjd_chain_price_many(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                   const double *discfactors_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                   const size_t *strike_offsets_host, int n_jobs, const double *params_host, const uint64_t *seeds_host,
                                   const uint32_t *call_ids_host, int nb_steps_per_year, int variable_type, double *prices_host,
                                   double *stderrs_host)
{
    const char *fn = "svmc_hawkesjd_chain_price_many";
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    Session *s = reinterpret_cast<Session *>(session);
    return chain_price_many(fn, session, c, n_jobs, params_host, seeds_host, call_ids_host, nb_steps_per_year, variable_type, prices_host,
                            stderrs_host, [&]() -> int {
        if (variable_type != SVMC_LOG_RETURN)  // the reference would price the log-return as a variance (:701-707)
            return fail(SVMC_ERR_UNSUPPORTED_VARIABLE, std::string(fn) + ": LOG_RETURN only");
        return hawkes_check_many(fn, n_jobs, params_host);
    },
                            hawkes_many_stepper(s, c, n_jobs, params_host, seeds_host, call_ids_host));
}

int svmc_hawkesjd_chain_price_tilted_many(svmc_session_t session, const double *ttms_host, const double *forwards_host, int n_expiries,
                                          const double *strikes_host, const int8_t *types_host, const size_t *strike_offsets_host,
                                          int n_jobs, const double *params_host, const uint64_t *seeds_host,
                                          const uint32_t *call_ids_host, int nb_steps_per_year, const double *gammas_host, int n_gammas,
                                          int recenter, double *prices_host, double *stderrs_host, double *stats_host)
{
    const char *fn = "svmc_hawkesjd_chain_price_tilted_many";
    const ChainView c = {n_expiries, ttms_host, forwards_host, nullptr, strikes_host, types_host, strike_offsets_host};
    Session *s = reinterpret_cast<Session *>(session);
    size_t need_ws = 0;
    if (int rc = svmc_payoff_workspace_bytes(&need_ws)) return rc;
    std::vector<double> shifts;
    TiltedBlock out;
    if (int rc = many_step(fn, s, c, n_jobs, params_host, seeds_host, call_ids_host, nb_steps_per_year, SVMC_LOG_RETURN, prices_host,
                           stderrs_host, false, need_ws, shifts,
                           [&]() -> int {
        // svmc_hawkesjd_chain_price_tilted's checks, for every job
        if (int rc = check_tilted(fn, c, gammas_host, static_cast<size_t>(n_jobs) * n_gammas, n_gammas, stats_host)) return rc;
        if (int rc = hawkes_check_many(fn, n_jobs, params_host)) return rc;
        return tilted_block(s, c, n_gammas, n_jobs, out);
    },
                           hawkes_many_stepper(s, c, n_jobs, params_host, seeds_host, call_ids_host)))
        return rc;
    ManyBuffers &mb = s->many;
    const size_t n = s->n_path, J = static_cast<size_t>(n_jobs), m = static_cast<size_t>(c.m), G = static_cast<size_t>(n_gammas);
    // per job the tilted launches of the single call on that job's snapshot rows (and, recentring, its rows of the spot sums)
    std::vector<const double *> xs(m);
    for (size_t j = 0; j < J; ++j) {
        for (size_t i = 0; i < m; ++i) xs[i] = mb.snap + (j * m + i) * n;
        if (int rc = svmc_tilted_payoff_chain(xs.data(), n, c.forwards, c.m, c.strikes, c.types, shifts.data(), c.offsets,
                                              gammas_host + j * G, n_gammas, recenter, recenter ? mb.spot + 2 * m * j : nullptr,
                                              out.prices(j), out.stderrs(j), out.stats(j), mb.ws, mb.ws_bytes,
                                              reinterpret_cast<svmc_stream_t>(s->stream)))
            return rc;
    }
    SVMC_HIP_TRY(hipStreamSynchronize(s->stream));
    stepping_read(s);
    for (size_t j = 0; j < J; ++j) out.copy_home(j, prices_host, stderrs_host, stats_host);
    return SVMC_OK;
}

int svmc_session_state(svmc_session_t session, double *x_host, double *vol_host, double *qvar_host)
{
    Session *s = reinterpret_cast<Session *>(session);
    SVMC_REQUIRE(s != nullptr, "svmc_session_state: null session");
    const size_t nb = s->n_path * sizeof(double);
    if (x_host) SVMC_HIP_TRY(hipMemcpyAsync(x_host, s->x, nb, hipMemcpyDeviceToHost, s->stream));
    if (vol_host) SVMC_HIP_TRY(hipMemcpyAsync(vol_host, s->vol, nb, hipMemcpyDeviceToHost, s->stream));
    if (qvar_host) SVMC_HIP_TRY(hipMemcpyAsync(qvar_host, s->qvar, nb, hipMemcpyDeviceToHost, s->stream));
    SVMC_HIP_TRY(hipStreamSynchronize(s->stream));
    return SVMC_OK;
}

}  // extern "C"

// ---- many conditional jobs of one chain and the conditional estimator's parameter sensitivities (include/svmc.h, DESIGN.md row
// f14; kernels and tails: svmc_cmc.hip).  The first half of both drivers: every check (check(): the caller's own), the session's
// buffers -- job j's mu rows at j m + i of s->cmany_snap, its cv rows J m rows further --, then step(nbs, dts, mu, cv): the model's ONE
// stepping launch of every job.
// the captured conditional evaluations read the shared stepping buffers at the addresses they had at capture
static void cmc_sets_drop(Session *s)
{
    for (CmcSetsGraph &cg : s->cmc_sets) fixed_graph_release(cg.g);
}

// cmc_many_prepare is that half up to the launch: the checks, the buffers and the step grids (svmc_*_chain_price_cmc_sets enqueues
// the launch itself, into a graph).  A regrown buffer drops the graphs that captured its old address.
template <class Check>
static int cmc_many_prepare(const char *fn, Session *s, const ChainView &c, int n_jobs, const void *params, const uint64_t *seeds,
                            const uint32_t *call_ids, int nb_steps_per_year, const double *out_a, const double *out_b,
                            size_t quotes_per_strike, Check &&check, std::vector<int> &nbs, std::vector<double> &dts)
{
    SVMC_REQUIRE(s != nullptr, std::string(fn) + ": null session");
    SVMC_REQUIRE(n_jobs >= 1 && n_jobs <= SVMC_MANY_MAX_JOBS, std::string(fn) + ": n_jobs must be in [1, SVMC_MANY_MAX_JOBS]");
    SVMC_REQUIRE(params && seeds && call_ids && c.ttms && c.forwards && c.discfactors && c.strikes && c.types && c.offsets && out_a && out_b,
                 std::string(fn) + ": null pointer");
    SVMC_REQUIRE(c.m >= 1 && c.m <= MAX_FUSED_SLICES, std::string(fn) + ": 1 to 16 expiries");
    if (c.m > s->max_expiries || c.offsets[c.m] > s->max_strikes)
        return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": the chain exceeds the session (max_expiries / max_strikes_total)");
    SVMC_REQUIRE(!s->sharded(), std::string(fn) + ": the conditional estimator is not sharded");
    SVMC_REQUIRE(nb_steps_per_year > 0, std::string(fn) + ": nb_steps_per_year must be positive");
    for (int j = 0; j < n_jobs; ++j) SVMC_REQUIRE(call_ids[j] < (1u << 24), std::string(fn) + ": call_id must fit 24 bits");
    if (int rc = check_quotes(fn, s->n_path, c.forwards, c.discfactors, c.m, c.strikes, c.types, c.offsets, 1u << 30, quotes_per_strike))
        return rc;
    if (int rc = check()) return rc;
    if (int rc = check_chain(fn, s, c, SVMC_LOG_RETURN, out_a, out_b, true)) return rc;
    const size_t n = s->n_path, J = static_cast<size_t>(n_jobs), m = static_cast<size_t>(c.m);
    const size_t table = cmc_many_table_bytes(n_jobs, c.m);
    const void *const before[3] = {s->cmany_snap, s->cmany_table_dev, s->cmany_table_host};
    const hipError_t e0 = grow(reinterpret_cast<void **>(&s->cmany_snap), s->cmany_snap_bytes, 2 * J * m * n * sizeof(double), false);
    const hipError_t e1 = grow(&s->cmany_table_dev, s->cmany_table_bytes, table, false);
    const hipError_t e2 = grow(&s->cmany_table_host, s->cmany_table_host_bytes, table, true);
    if (before[0] != s->cmany_snap || before[1] != s->cmany_table_dev || before[2] != s->cmany_table_host) cmc_sets_drop(s);
    SVMC_HIP_TRY(e0);
    SVMC_HIP_TRY(e1);
    SVMC_HIP_TRY(e2);
    expiry_grids(c, nb_steps_per_year, nbs, dts);
    return SVMC_OK;
}

template <class Check, class Step>
static int cmc_many_step(const char *fn, Session *s, const ChainView &c, int n_jobs, const void *params, const uint64_t *seeds,
                         const uint32_t *call_ids, int nb_steps_per_year, const double *out_a, const double *out_b, size_t quotes_per_strike,
                         Check &&check, Step &&step)
{
    std::vector<int> nbs;
    std::vector<double> dts;
    if (int rc = cmc_many_prepare(fn, s, c, n_jobs, params, seeds, call_ids, nb_steps_per_year, out_a, out_b, quotes_per_strike, check, nbs, dts))
        return rc;
    const size_t n = s->n_path, J = static_cast<size_t>(n_jobs), m = static_cast<size_t>(c.m);
    stepping_begin(s);
    if (int rc = step(nbs, dts, s->cmany_snap, s->cmany_snap + J * m * n)) return rc;
    stepping_end(s);
    return SVMC_OK;
}

// job j's mu and cv rows after cmc_many_step
static void cmc_many_rows(const Session *s, const ChainView &c, int n_jobs, int j, std::vector<const double *> &mus, std::vector<const double *> &cvs)
{
    const size_t n = s->n_path, m = static_cast<size_t>(c.m), J = static_cast<size_t>(n_jobs);
    mus.resize(m);
    cvs.resize(m);
    for (size_t i = 0; i < m; ++i) {
        mus[i] = s->cmany_snap + (static_cast<size_t>(j) * m + i) * n;
        cvs[i] = s->cmany_snap + ((J + static_cast<size_t>(j)) * m + i) * n;
    }
}

// the many-job conditional pricer: cmc_many_step, then per job svmc_cmc_payoff_chain's tail on its rows (each ends synchronised)
template <class Step>
static int chain_price_cmc_many(const char *fn, Session *s, const ChainView &c, int n_jobs, const void *params, const uint64_t *seeds,
                                const uint32_t *call_ids, int nb_steps_per_year, int recenter, double *prices, double *stderrs,
                                double *stats, Step &&step)
{
    if (int rc = cmc_many_step(fn, s, c, n_jobs, params, seeds, call_ids, nb_steps_per_year, prices, stderrs, 1, [&]() -> int {
        const size_t K = c.offsets[c.m];
        SVMC_HIP_TRY(grow(&s->cmc_ws, s->cmc_ws_bytes, cmc_workspace_bytes_of(s->n_path, c.m, K, false), false));
        SVMC_HIP_TRY(grow(&s->cmc_pinned, s->cmc_pinned_bytes, cmc_pinned_bytes_of(c.m, K, false), true));
        return SVMC_OK;
    }, step))
        return rc;
    const size_t K = c.offsets[c.m];
    std::vector<const double *> mus, cvs;
    for (int j = 0; j < n_jobs; ++j) {
        cmc_many_rows(s, c, n_jobs, j, mus, cvs);
        if (int rc = cmc_tail(fn, mus.data(), cvs.data(), s->n_path, c.forwards, c.discfactors, c.m, c.strikes, c.types, c.offsets, recenter,
                              prices + K * j, stderrs + K * j, nullptr,
                              stats ? stats + static_cast<size_t>(SVMC_CMC_STATS_DOUBLES) * c.m * j : nullptr, s->cmc_ws, s->cmc_ws_bytes,
                              s->stream, s->cmc_pinned, s->cmc_pinned_bytes))
            return rc;
    }
    stepping_read(s);
    return SVMC_OK;
}

// the fused sensitivity driver: the 1 + 2P rows of `params` on one (seed, call id) and one stepping launch, the sensitivity tail on
// the bumped jobs' rows with its results copied into page-locked memory, then svmc_cmc_greeks_chain's tail on job 0's rows, whose
// synchronisation is the call's only one
template <class Step>
static int chain_price_cmc_sens(const char *fn, Session *s, const ChainView &c, int n_params, const double *params, const double *steps,
                                int nb_steps_per_year, int recenter, uint64_t seed, uint32_t call_id, double *greeks, double *stats,
                                double *sens, Step &&step)
{
    SVMC_REQUIRE(n_params >= 0 && n_params <= SVMC_GREEKS_MAX_PARAMS, std::string(fn) + ": n_params must be in [0, SVMC_GREEKS_MAX_PARAMS]");
    SVMC_REQUIRE(greeks != nullptr && (n_params == 0 || (sens != nullptr && steps != nullptr)), std::string(fn) + ": null pointer");
    const int P = n_params, J = 1 + 2 * P;
    const std::vector<uint64_t> seeds(J, seed);
    const std::vector<uint32_t> call_ids(J, call_id);
    // (the sensitivity tail's table holds every quote once per bumped job: 2 P K strikes)
    if (int rc = cmc_many_step(fn, s, c, J, params, seeds.data(), call_ids.data(), nb_steps_per_year, greeks, greeks, 2 * static_cast<size_t>(P),
                               [&]() -> int {
        const size_t K = c.offsets[c.m];
        if (P > 0) {
            if (int rc = check_steps(fn, P, steps, 1)) return rc;
            SVMC_HIP_TRY(grow(&s->csens_ws, s->csens_ws_bytes, cmc_sens_workspace_bytes_of(s->n_path, c.m, K, P), false));
            SVMC_HIP_TRY(grow(&s->csens_pinned, s->csens_pinned_bytes, cmc_sens_pinned(nullptr, c.m, K, P, nullptr), true));
        }
        SVMC_HIP_TRY(grow(&s->cmc_ws, s->cmc_ws_bytes, cmc_workspace_bytes_of(s->n_path, c.m, K, true), false));
        SVMC_HIP_TRY(grow(&s->cmc_pinned, s->cmc_pinned_bytes, cmc_pinned_bytes_of(c.m, K, true), true));
        return SVMC_OK;
    },
                               [&](const std::vector<int> &nbs, const std::vector<double> &dts, double *mu, double *cv) {
        return step(nbs, dts, seeds.data(), call_ids.data(), mu, cv);
    }))
        return rc;
    const size_t n = s->n_path, m = static_cast<size_t>(c.m), K = c.offsets[c.m];
    double *sens_out = nullptr;
    if (P > 0) {
        std::vector<const double *> up_mu(P * m), up_cv(P * m), dn_mu(P * m), dn_cv(P * m);
        const double *mu0 = s->cmany_snap, *cv0 = s->cmany_snap + static_cast<size_t>(J) * m * n;
        for (size_t p = 0; p < static_cast<size_t>(P); ++p)
            for (size_t i = 0; i < m; ++i) {
                const size_t up = ((1 + 2 * p) * m + i) * n, dn = ((2 + 2 * p) * m + i) * n;
                up_mu[p * m + i] = mu0 + up;
                up_cv[p * m + i] = cv0 + up;
                dn_mu[p * m + i] = mu0 + dn;
                dn_cv[p * m + i] = cv0 + dn;
            }
        double *res = nullptr;
        if (int rc = cmc_sens_enqueue(fn, up_mu.data(), up_cv.data(), dn_mu.data(), dn_cv.data(), n, c.forwards, c.discfactors, c.m, c.strikes,
                                      c.types, c.offsets, P, steps, recenter, s->csens_pinned, s->csens_ws, s->csens_ws_bytes, s->stream, &res))
            return rc;
        cmc_sens_pinned(s->csens_pinned, c.m, K, P, &sens_out);
        if (K > 0)
            SVMC_HIP_TRY(hipMemcpyAsync(sens_out, res, static_cast<size_t>(SVMC_CMC_SENS_ROWS) * P * K * sizeof(double), hipMemcpyDeviceToHost,
                                        s->stream));
    }
    std::vector<const double *> mus, cvs;
    cmc_many_rows(s, c, J, 0, mus, cvs);
    if (int rc = cmc_tail(fn, mus.data(), cvs.data(), n, c.forwards, c.discfactors, c.m, c.strikes, c.types, c.offsets, recenter, nullptr,
                          nullptr, greeks, stats, s->cmc_ws, s->cmc_ws_bytes, s->stream, s->cmc_pinned, s->cmc_pinned_bytes))
        return rc;                                         // (returns synchronised: the sensitivities have landed too)
    stepping_read(s);
    if (P > 0 && K > 0) memcpy(sens, sens_out, static_cast<size_t>(SVMC_CMC_SENS_ROWS) * P * K * sizeof(double));
    return SVMC_OK;
}

// ---- the conditional calibration objective (include/svmc.h): n_sets parameter sets of one chain on ONE (seed,
// call id) as one replayed graph -- a linear chain of [upload of the job table | the many-job stepping launch | the tail of
// cmc_sets_enqueue, whose last kernels store the results in page-locked memory].  step(nbs, dts, seeds, call_ids, mu, cv, stream,
// what) is the model's {log,heston}_cmc_step_many.  Everything that shapes the launches is in the slot's key, the parameters travel in the job
// table; with graphs off the same launches are issued directly.
template <class Step>
static int chain_price_cmc_sets(const char *fn, Session *s, const ChainView &c, int model, int n_sets, const double *params, int is_spot_measure,
                                int nb_steps_per_year, int recenter, uint64_t seed, uint32_t call_id, double *prices, double *stderrs,
                                double *stats, double *ivols, Step &&step)
{
    SVMC_REQUIRE(s != nullptr, std::string(fn) + ": null session");
    SVMC_REQUIRE(n_sets >= 1 && n_sets <= SVMC_CMC_SETS_MAX, std::string(fn) + ": n_sets must be in [1, SVMC_CMC_SETS_MAX]");
    const int P = n_sets, want_iv = ivols != nullptr ? 1 : 0, rec = recenter ? 1 : 0, spot = is_spot_measure ? 1 : 0;
    const std::vector<uint64_t> seeds(P, seed);
    const std::vector<uint32_t> call_ids(P, call_id);
    CmcSetsGraph &cg = s->cmc_sets[P];
    std::vector<int> nbs;
    std::vector<double> dts;
    if (int rc = cmc_many_prepare(fn, s, c, P, params, seeds.data(), call_ids.data(), nb_steps_per_year, prices, stderrs, static_cast<size_t>(P),
                                  [&]() -> int {
        // (the slot's own buffers: a regrown one has lost the table's image)
        const size_t K = c.offsets[c.m];
        const void *const ws = cg.ws, *const pinned = cg.pinned;
        const hipError_t e0 = grow(&cg.ws, cg.ws_bytes, cmc_sets_workspace_bytes(s->n_path, c.m, K, P), false);
        const hipError_t e1 = grow(&cg.pinned, cg.pinned_bytes, cmc_sets_pinned_bytes(c.m, K, P), true);
        if (ws != cg.ws || pinned != cg.pinned) fixed_graph_release(cg.g);
        SVMC_HIP_TRY(e0);
        SVMC_HIP_TRY(e1);
        return SVMC_OK;
    }, nbs, dts))
        return rc;
    const size_t n = s->n_path, m = static_cast<size_t>(c.m), K = c.offsets[c.m];
    double *mu = s->cmany_snap, *cv = s->cmany_snap + static_cast<size_t>(P) * m * n;
    if (s->stream == nullptr && s->cmc_sets_stream == nullptr)
        SVMC_HIP_TRY(hipStreamCreateWithFlags(&s->cmc_sets_stream, hipStreamNonBlocking));
    const hipStream_t stream = s->stream != nullptr ? s->stream : s->cmc_sets_stream;
    // the chain (with its discount factors: they are in the table), the model and everything else that shapes a launch or the
    // table's image, and the address of every buffer the graph reads or writes
    std::vector<unsigned char> key = chain_key(c, P, SVMC_LOG_RETURN, 1);
    for (const int v : {model, spot, rec, want_iv}) key_append(key, &v, 1);
    key_append(key, nbs.data(), c.m);
    key_append(key, &seed, 1);
    key_append(key, &call_id, 1);
    key_append(key, &s->path_offset, 1);
    key_append(key, &n, 1);
    for (const void *p : {static_cast<const void *>(s->cmany_snap), static_cast<const void *>(s->cmany_table_dev),
                          static_cast<const void *>(s->cmany_table_host), static_cast<const void *>(cg.ws), static_cast<const void *>(cg.pinned)})
        key_append(key, &p, 1);
    auto enqueue = [&](int what) -> int {
        if (int rc = step(nbs, dts, seeds.data(), call_ids.data(), mu, cv, stream, what)) return rc;
        if (!(what & CMC_MANY_ENQUEUE)) return SVMC_OK;
        return cmc_sets_enqueue(fn, n, c.m, c.offsets, P, rec, want_iv != 0, IV_VOL_LO, IV_VOL_HI, cg.ws, cg.ws_bytes, cg.pinned, stream);
    };
    if (cg.g.key != key) {
        fixed_graph_release(cg.g);
        if (int rc = cmc_sets_upload(fn, mu, cv, n, c.ttms, c.forwards, c.discfactors, c.m, c.strikes, c.types, c.offsets, P, cg.ws, cg.ws_bytes,
                                     cg.pinned, stream))
            return rc;
        cg.g.key = key;
    }
    if (s->use_graphs) {
        if (cg.g.exec == nullptr) {    // captured at the first replayed call of this key (an un-replayed call may come first)
            if (int rc = graph_capture(s, cg.g, fn, [&]() { return enqueue(CMC_MANY_FILL | CMC_MANY_ENQUEUE); }, stream)) return rc;
        } else if (int rc = enqueue(CMC_MANY_FILL)) {
            return rc;
        }
        SVMC_HIP_TRY(hipGraphLaunch(cg.g.exec, stream));
        ++s->graph_launches;
    } else if (int rc = enqueue(CMC_MANY_FILL | CMC_MANY_ENQUEUE)) {
        return rc;
    }
    SVMC_HIP_TRY(hipStreamSynchronize(stream));
    const double *r_prices, *r_stderrs, *r_stats, *r_ivols;
    cmc_sets_results(cg.pinned, c.m, K, P, &r_prices, &r_stderrs, &r_stats, &r_ivols);
    memcpy(prices, r_prices, P * K * sizeof(double));
    memcpy(stderrs, r_stderrs, P * K * sizeof(double));
    if (stats != nullptr) memcpy(stats, r_stats, static_cast<size_t>(SVMC_CMC_STATS_DOUBLES) * P * m * sizeof(double));
    if (ivols != nullptr) memcpy(ivols, r_ivols, P * K * sizeof(double));
    return SVMC_OK;
}

extern "C" {

int svmc_logsv_chain_price_cmc_many(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                    const double *discfactors_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                    const size_t *strike_offsets_host, int n_jobs, const double *params_host, const uint64_t *seeds_host,
                                    const uint32_t *call_ids_host, int is_spot_measure, int nb_steps_per_year, int recenter,
                                    double *prices_host, double *stderrs_host, double *stats_host)
{
    const char *fn = "svmc_logsv_chain_price_cmc_many";
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    Session *s = reinterpret_cast<Session *>(session);
    return chain_price_cmc_many(fn, s, c, n_jobs, params_host, seeds_host, call_ids_host, nb_steps_per_year, recenter, prices_host,
                                stderrs_host, stats_host,
                                [&](const std::vector<int> &nbs, const std::vector<double> &dts, double *mu, double *cv) {
        return logsv_cmc_step_many(fn, s->n_path, n_jobs, c.m, nbs.data(), dts.data(), params_host, is_spot_measure, seeds_host, call_ids_host,
                                   s->path_offset, s->cmany_table_host, s->cmany_table_dev, mu, cv, s->stream);
    });
}

int svmc_heston_chain_price_cmc_many(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                     const double *discfactors_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                     const size_t *strike_offsets_host, int n_jobs, const double *params_host, const uint64_t *seeds_host,
                                     const uint32_t *call_ids_host, int nb_steps_per_year, int recenter, double *prices_host,
                                     double *stderrs_host, double *stats_host)
{
    const char *fn = "svmc_heston_chain_price_cmc_many";
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    Session *s = reinterpret_cast<Session *>(session);
    return chain_price_cmc_many(fn, s, c, n_jobs, params_host, seeds_host, call_ids_host, nb_steps_per_year, recenter, prices_host,
                                stderrs_host, stats_host,
                                [&](const std::vector<int> &nbs, const std::vector<double> &dts, double *mu, double *cv) {
        return heston_cmc_step_many(fn, s->n_path, n_jobs, c.m, nbs.data(), dts.data(), params_host, seeds_host, call_ids_host,
                                    s->path_offset, s->cmany_table_host, s->cmany_table_dev, mu, cv, s->stream);
    });
}

int svmc_logsv_chain_price_cmc_sens(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                    const double *discfactors_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                    const size_t *strike_offsets_host, int n_params, const double *params_host, const double *steps_host,
                                    int is_spot_measure, int nb_steps_per_year, int recenter, uint64_t seed, uint32_t call_id,
                                    double *greeks_host, double *stats_host, double *sens_host)
{
    const char *fn = "svmc_logsv_chain_price_cmc_sens";
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    Session *s = reinterpret_cast<Session *>(session);
    const int n_jobs = 1 + 2 * n_params;
    return chain_price_cmc_sens(fn, s, c, n_params, params_host, steps_host, nb_steps_per_year, recenter, seed, call_id, greeks_host,
                                stats_host, sens_host,
                                [&](const std::vector<int> &nbs, const std::vector<double> &dts, const uint64_t *seeds, const uint32_t *call_ids,
                                    double *mu, double *cv) {
        return logsv_cmc_step_many(fn, s->n_path, n_jobs, c.m, nbs.data(), dts.data(), params_host, is_spot_measure, seeds, call_ids,
                                   s->path_offset, s->cmany_table_host, s->cmany_table_dev, mu, cv, s->stream);
    });
}

int svmc_heston_chain_price_cmc_sens(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                     const double *discfactors_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                     const size_t *strike_offsets_host, int n_params, const double *params_host, const double *steps_host,
                                     int nb_steps_per_year, int recenter, uint64_t seed, uint32_t call_id, double *greeks_host,
                                     double *stats_host, double *sens_host)
{
    const char *fn = "svmc_heston_chain_price_cmc_sens";
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    Session *s = reinterpret_cast<Session *>(session);
    const int n_jobs = 1 + 2 * n_params;
    return chain_price_cmc_sens(fn, s, c, n_params, params_host, steps_host, nb_steps_per_year, recenter, seed, call_id, greeks_host,
                                stats_host, sens_host,
                                [&](const std::vector<int> &nbs, const std::vector<double> &dts, const uint64_t *seeds, const uint32_t *call_ids,
                                    double *mu, double *cv) {
        return heston_cmc_step_many(fn, s->n_path, n_jobs, c.m, nbs.data(), dts.data(), params_host, seeds, call_ids, s->path_offset,
                                    s->cmany_table_host, s->cmany_table_dev, mu, cv, s->stream);
    });
}

int svmc_logsv_chain_price_cmc_sets(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                    const double *discfactors_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                    const size_t *strike_offsets_host, int n_sets, const double *params_host, int is_spot_measure,
                                    int nb_steps_per_year, int recenter, uint64_t seed, uint32_t call_id, double *prices_host,
                                    double *stderrs_host, double *stats_host, double *ivols_host)
{
    const char *fn = "svmc_logsv_chain_price_cmc_sets";
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    Session *s = reinterpret_cast<Session *>(session);
    return chain_price_cmc_sets(fn, s, c, 0, n_sets, params_host, is_spot_measure, nb_steps_per_year, recenter, seed, call_id, prices_host,
                                stderrs_host, stats_host, ivols_host,
                                [&](const std::vector<int> &nbs, const std::vector<double> &dts, const uint64_t *seeds, const uint32_t *call_ids,
                                    double *mu, double *cv, hipStream_t stream, int what) {
        return logsv_cmc_step_many(fn, s->n_path, n_sets, c.m, nbs.data(), dts.data(), params_host, is_spot_measure, seeds, call_ids,
                                   s->path_offset, s->cmany_table_host, s->cmany_table_dev, mu, cv, stream, what);
    });
}

int svmc_heston_chain_price_cmc_sets(svmc_session_t session, const double *ttms_host, const double *forwards_host,
                                     const double *discfactors_host, int n_expiries, const double *strikes_host, const int8_t *types_host,
                                     const size_t *strike_offsets_host, int n_sets, const double *params_host, int nb_steps_per_year,
                                     int recenter, uint64_t seed, uint32_t call_id, double *prices_host, double *stderrs_host,
                                     double *stats_host, double *ivols_host)
{
    const char *fn = "svmc_heston_chain_price_cmc_sets";
    const ChainView c = {n_expiries, ttms_host, forwards_host, discfactors_host, strikes_host, types_host, strike_offsets_host};
    Session *s = reinterpret_cast<Session *>(session);
    return chain_price_cmc_sets(fn, s, c, 1, n_sets, params_host, 0, nb_steps_per_year, recenter, seed, call_id, prices_host, stderrs_host,
                                stats_host, ivols_host,
                                [&](const std::vector<int> &nbs, const std::vector<double> &dts, const uint64_t *seeds, const uint32_t *call_ids,
                                    double *mu, double *cv, hipStream_t stream, int what) {
        return heston_cmc_step_many(fn, s->n_path, n_sets, c.m, nbs.data(), dts.data(), params_host, seeds, call_ids, s->path_offset,
                                    s->cmany_table_host, s->cmany_table_dev, mu, cv, stream, what);
    });
}

}  // extern "C"
