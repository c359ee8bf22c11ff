// svmc_quotes.h -- the host side of a chain's quote table, shared by the four payoff tails that upload one: the Greeks tail
// (svmc_greeks.hip) and the conditional payoff tail, its derivatives in F and K and its parameter sensitivities (svmc_cmc.hip).
// The strike groups, the device tables, ONE walk per tail that is both the byte count of its workspace and its carving (the uploaded
// image and the page-locked block the same), the image builders.  No HIP header: tests/native/quote_layout_probe.cpp is g++'s.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "svmc.h"

namespace svmc {

constexpr int QUOTE_BLOCK = 256;           // = BLOCK of svmc_block.h: paths per block of the tails' kernels
constexpr unsigned QUOTE_ROWS = 1024;      // path blocks per launch at most: rows(n) is a function of n_path alone
inline unsigned quote_rows(size_t n) { return static_cast<unsigned>(std::min<size_t>((n + QUOTE_BLOCK - 1) / QUOTE_BLOCK, QUOTE_ROWS)); }

// A walk over a block of memory: take() hands out the next 8-aligned region.  base null: nothing is carved and bytes() is the
// size the same walk needs, so a block's size and its carving cannot disagree.
struct Layout {
    unsigned char *base;
    size_t offset = 0;
    template <class T>
    T *take(size_t count)
    {
        offset = (offset + 7) & ~static_cast<size_t>(7);
        T *p = base ? reinterpret_cast<T *>(base + offset) : nullptr;
        offset += sizeof(T) * count;
        return p;
    }
    size_t bytes() const { return offset; }
};

// strikes [k0, k0 + nk) of `expiry`; pad = 1: the expiry's first group (read by the derivative tail, which counts the cv == 0
// paths of an expiry there)
struct QuoteGroup {
    int expiry, k0, nk, pad;
};
// The groups of up to kt strikes that tile every expiry's [offsets[i], offsets[i + 1]), written to `out` where it is not null;
// one_for_empty: an expiry without strikes gets one group of nk = 0.  Returns their count.
inline int quote_groups(int m, const size_t *offsets, int kt, bool one_for_empty, QuoteGroup *out = nullptr)
{
    int g = 0;
    for (int i = 0; i < m; ++i) {
        const int k0 = static_cast<int>(offsets[i]), k1 = static_cast<int>(offsets[i + 1]);
        if (one_for_empty && k0 == k1) {
            if (out) out[g] = QuoteGroup{i, 0, 0, 1};
            ++g;
        }
        for (int k = k0; k < k1; k += kt, ++g)
            if (out) out[g] = QuoteGroup{i, k, std::min(k1 - k, kt), (k == k0) ? 1 : 0};
    }
    return g;
}
// ... and what bounds the count for any offsets: every expiry may end in a ragged group (or be empty)
inline int quote_groups_bound(int m, size_t K, int kt) { return static_cast<int>(K / kt) + m; }

// the loop every image builder makes: expiry(i, k0, k1) per expiry, then column(i, k) per strike of it
template <class Expiry, class Column>
inline void quote_image(int m, const size_t *offsets, Expiry &&expiry, Column &&column)
{
    for (int i = 0; i < m; ++i) {
        const int k0 = static_cast<int>(offsets[i]), k1 = static_cast<int>(offsets[i + 1]);
        expiry(i, k0, k1);
        for (int k = k0; k < k1; ++k) column(i, k);
    }
}

// ---- the conditional payoff tail and its derivatives in F and K ----------------------------------------------------------------
constexpr int CMC_KT = 8;                      // strikes per group: two accumulators and three constants per strike in vector registers
constexpr int CMC_DKT = SVMC_CMC_GREEKS_KT;    // strikes per group: six accumulators, three shifts and three constants per strike
constexpr int CMC_DQ = 6;                      // per strike: sum and sum of squares of delta, dual delta, dual gamma (minus their shifts)

// the device table of a chain, uploaded once per call
struct CmcExpiry {
    const double *mu, *cv;
    double forward, ln_forward, discfactor;
    int k0, k1;                        // its strikes [k0, k1)
};
struct CmcTable {
    const CmcExpiry *expiries;
    const QuoteGroup *groups;
    const double *strikes;             // [K]
    const double *is_put;              // [K] 0 | 1
    const double *intrinsic;           // [K] max(+-(F - K), 0): the shift where path 0 of the expiry is dropped
    double *kp, *ln_kp, *shift;        // [K] device-computed: K + corr, its logarithm (0 where K + corr <= 0), the sums' shift
    double *fwd;                       // [m][4]: sum (e - 1), sum (e - 1)^2, kept count, corr
    double *stats;                     // [m][SVMC_CMC_STATS_DOUBLES]
    double *fwd_partials;              // [rows][m][3]
    double *pay_partials;              // [rows][K][2]
    double *out;                       // [2][K]: prices, errors
    int m, K;
    unsigned rows;
};
// what the derivative launches add to a chain's CmcTable
struct CmcDerivTable {
    const QuoteGroup *groups;          // groups of up to CMC_DKT strikes; pad = 1: the expiry's first group, which counts its cv == 0
                                       // paths (an expiry without strikes has one group of nk = 0 for that count)
    double *shift;                     // [K][3]: delta, dual delta and dual gamma of the expiry's path 0 -- or of (mu, cv) = (0, 0)
    double *partials;                  // [rows][K][CMC_DQ]
    double *zero_partials;             // [rows][m]
    double *out;                       // [8][K]: delta, dual delta, gamma, dual gamma, each followed by its error
    double *zero;                      // [m]: kept paths with cv == 0
};

// The uploaded image of the conditional tails: expiries, groups (GD: the derivative launches', 0 without them), strikes / is_put /
// intrinsic, steps (the sensitivity tail's; its table counts every expiry and strike once per bumped job) -- and the head of the
// workspace that cmc_forward_kernel and its finish work on: the image, then kp, ln_kp, shift and fwd.
struct CmcImage {
    CmcExpiry *expiries;
    QuoteGroup *groups, *dgroups;
    double *strikes, *is_put, *intrinsic, *steps;
};
inline CmcImage cmc_image(Layout &w, size_t n_expiries, size_t n_strikes, int G, int GD, int n_steps)
{
    return CmcImage{w.take<CmcExpiry>(n_expiries), w.take<QuoteGroup>(G), w.take<QuoteGroup>(GD), w.take<double>(n_strikes),
                    w.take<double>(n_strikes), w.take<double>(n_strikes), w.take<double>(n_steps)};     // (a braced list: in this order)
}
inline CmcImage cmc_table_head(Layout &w, size_t n_path, size_t n_expiries, size_t n_strikes, int G, int GD, int n_steps, CmcTable &t,
                               size_t &image_bytes)
{
    const CmcImage im = cmc_image(w, n_expiries, n_strikes, G, GD, n_steps);
    image_bytes = w.bytes();
    t.expiries = im.expiries;
    t.strikes = im.strikes;
    t.is_put = im.is_put;
    t.intrinsic = im.intrinsic;
    t.kp = w.take<double>(n_strikes);
    t.ln_kp = w.take<double>(n_strikes);
    t.shift = w.take<double>(n_strikes);
    t.fwd = w.take<double>(4 * n_expiries);
    t.m = static_cast<int>(n_expiries);
    t.K = static_cast<int>(n_strikes);
    t.rows = quote_rows(n_path);
    return im;
}
// the results, one block: prices [K], errors [K], (the derivatives [8][K],) statistics [m][5] (, the cv == 0 counts [m])
struct CmcResults {
    double *out, *deriv_out, *stats, *zero;
};
inline CmcResults cmc_results(Layout &w, int m, size_t K, bool deriv)
{
    return CmcResults{w.take<double>(2 * K), w.take<double>(deriv ? 8 * K : 0), w.take<double>(static_cast<size_t>(SVMC_CMC_STATS_DOUBLES) * m),
                      w.take<double>(deriv ? m : 0)};
}
// the workspace: the head, the results, the partials; GD > 0: with the derivative launches' regions.  Returns the bytes of the
// image, which the walk starts with.
inline size_t cmc_workspace(Layout &w, size_t n_path, int m, size_t K, int G, int GD, CmcTable &t, CmcDerivTable &dt)
{
    const size_t rows = quote_rows(n_path), deriv = GD > 0 ? 1 : 0;
    size_t image_bytes;
    const CmcImage im = cmc_table_head(w, n_path, m, K, G, GD, 0, t, image_bytes);
    t.groups = im.groups;
    dt.groups = im.dgroups;
    const CmcResults r = cmc_results(w, m, K, deriv != 0);
    t.out = r.out;
    dt.out = r.deriv_out;
    t.stats = r.stats;
    dt.zero = r.zero;
    t.fwd_partials = w.take<double>(rows * 3 * m);
    t.pay_partials = w.take<double>(rows * 2 * K);
    dt.shift = w.take<double>(deriv * 3 * K);
    dt.partials = w.take<double>(deriv * rows * CMC_DQ * K);
    dt.zero_partials = w.take<double>(deriv * rows * m);
    return image_bytes;
}
// the host block of a call, page-locked in the fused drivers: the image, then the results' landing
inline CmcResults cmc_pinned(Layout &w, int m, size_t K, int G, int GD, CmcImage &im)
{
    im = cmc_image(w, m, K, G, GD, 0);
    return cmc_results(w, m, K, GD > 0);
}
// The sizes a caller allocates before it knows the offsets: the walks at the group counts no chain of K strikes exceeds.
inline size_t cmc_workspace_bytes_of(size_t n_path, int m, size_t K, bool deriv)
{
    CmcTable t;
    CmcDerivTable dt;
    Layout w{nullptr};
    cmc_workspace(w, n_path, m, K, quote_groups_bound(m, K, CMC_KT), deriv ? quote_groups_bound(m, K, CMC_DKT) : 0, t, dt);
    return w.bytes();
}
inline size_t cmc_pinned_bytes_of(int m, size_t K, bool deriv)
{
    CmcImage im;
    Layout w{nullptr};
    cmc_pinned(w, m, K, quote_groups_bound(m, K, CMC_KT), deriv ? quote_groups_bound(m, K, CMC_DKT) : 0, im);
    return w.bytes();
}

// strike `at` of the conditional tails' three columns
inline void cmc_columns(double *strikes, double *is_put, double *intrinsic, size_t at, double strike, bool put, double forward)
{
    strikes[at] = strike;
    is_put[at] = put ? 1.0 : 0.0;
    intrinsic[at] = put ? std::fmax(strike - forward, 0.0) : std::fmax(forward - strike, 0.0);
}
inline void cmc_fill_image(const CmcImage &im, const double *const *mu, const double *const *cv, const double *forwards,
                           const double *discfactors, int m, const double *strikes, const int8_t *types, const size_t *offsets, bool deriv)
{
    quote_image(m, offsets,
                [&](int i, int k0, int k1) { im.expiries[i] = CmcExpiry{mu[i], cv[i], forwards[i], std::log(forwards[i]), discfactors[i], k0, k1}; },
                [&](int i, int k) { cmc_columns(im.strikes, im.is_put, im.intrinsic, k, strikes[k], types[k] == SVMC_PUT, forwards[i]); });
    quote_groups(m, offsets, CMC_KT, false, im.groups);
    if (deriv) quote_groups(m, offsets, CMC_DKT, true, im.dgroups);
}

// ---- the conditional estimator's parameter sensitivities: the 2P bumped jobs as ONE CmcTable of 2P m expiries and 2P K strikes ------
constexpr int SENS_KT = SVMC_CMC_GREEKS_KT;    // strikes per group
constexpr int SENS_PQ = 4;                     // per (pair, quote): sum (d - d0), sum (dt - dt0), its squares, the kept pairs

struct CmcSensTable {
    const QuoteGroup *groups;          // groups of up to SENS_KT strikes of one expiry of the CHAIN: k0 in [0, K)
    const double *steps;               // [P]
    double *q_partials;                // [rows][2P K]
    double *q;                         // [2P K]: mean_kept_j(B_k), the job's dual delta before discounting
    double *pair_shift;                // [P K][2]: d and dt of the expiry's path 0, or 0 where it is not a kept pair
    double *pair_partials;             // [rows][P K][SENS_PQ]
    double *out;                       // [P][SVMC_CMC_SENS_ROWS][K]
    int P, m, K;                       // the chain's expiries and quotes
};

// the image: cmc_image of 2P m expiries and 2P K strikes with the steps [P]
inline CmcImage cmc_sens_image(Layout &w, int m, size_t K, int G, int P) { return cmc_image(w, 2 * static_cast<size_t>(P) * m, 2 * P * K, G, 0, P); }
// the workspace: the head; stats; the forward partials; q partials and q; the pair shifts and partials; the results -> image bytes
inline size_t cmc_sens_workspace(Layout &w, size_t n_path, int m, size_t K, int G, int P, CmcTable &t, CmcSensTable &st)
{
    const size_t rows = quote_rows(n_path), JK = 2 * P * K, Jm = 2 * static_cast<size_t>(P) * m;
    size_t image_bytes;
    const CmcImage im = cmc_table_head(w, n_path, Jm, JK, G, 0, P, t, image_bytes);
    t.groups = nullptr;
    st.groups = im.groups;
    st.steps = im.steps;
    t.stats = w.take<double>(SVMC_CMC_STATS_DOUBLES * Jm);
    t.fwd_partials = w.take<double>(rows * 3 * Jm);
    t.pay_partials = nullptr;
    t.out = nullptr;
    st.q_partials = w.take<double>(rows * JK);
    st.q = w.take<double>(JK);
    st.pair_shift = w.take<double>(JK);
    st.pair_partials = w.take<double>(rows * SENS_PQ * P * K);
    st.out = w.take<double>(static_cast<size_t>(SVMC_CMC_SENS_ROWS) * P * K);
    st.P = P;
    st.m = m;
    st.K = static_cast<int>(K);
    return image_bytes;
}
inline size_t cmc_sens_workspace_bytes_of(size_t n_path, int m, size_t K, int P)
{
    CmcTable t;
    CmcSensTable st;
    Layout w{nullptr};
    cmc_sens_workspace(w, n_path, m, K, quote_groups_bound(m, K, SENS_KT), P, t, st);
    return w.bytes();
}
// The host block of a call, page-locked in the fused driver: the image at the group bound -- the launch builds its own, at the chain's
// count, in its head -- then the [P][SVMC_CMC_SENS_ROWS][K] results' landing.  Returns the bytes; pinned not null: *sens_out is the landing.
inline size_t cmc_sens_pinned(void *pinned, int m, size_t K, int P, double **sens_out)
{
    Layout w{static_cast<unsigned char *>(pinned)};
    cmc_sens_image(w, m, K, quote_groups_bound(m, K, SENS_KT), P);
    double *out = w.take<double>(static_cast<size_t>(SVMC_CMC_SENS_ROWS) * P * K);
    if (sens_out != nullptr) *sens_out = out;
    return w.bytes();
}
// up / dn rows [P][m]; job j = 2 p + (0: up | 1: dn) holds expiries [j m, (j + 1) m) and strikes [j K, (j + 1) K)
inline void cmc_sens_fill_image(const CmcImage &im, const double *const *up_mu, const double *const *up_cv, const double *const *dn_mu,
                                const double *const *dn_cv, const double *forwards, const double *discfactors, int m, const double *strikes,
                                const int8_t *types, const size_t *offsets, int P, const double *steps)
{
    const int K = static_cast<int>(offsets[m]);
    for (int j = 0; j < 2 * P; ++j) {
        const int r0 = (j / 2) * m, o = j * K;
        const bool up = (j & 1) == 0;
        quote_image(m, offsets,
            [&](int i, int k0, int k1) {
                im.expiries[j * m + i] = CmcExpiry{up ? up_mu[r0 + i] : dn_mu[r0 + i], up ? up_cv[r0 + i] : dn_cv[r0 + i], forwards[i],
                                                   std::log(forwards[i]), discfactors[i], o + k0, o + k1};
            },
            [&](int i, int k) { cmc_columns(im.strikes, im.is_put, im.intrinsic, o + k, strikes[k], types[k] == SVMC_PUT, forwards[i]); });
    }
    quote_groups(m, offsets, SENS_KT, false, im.groups);
    for (int p = 0; p < P; ++p) im.steps[p] = steps[p];
}

// ---- the conditional calibration objective: P parameter sets as ONE CmcTable of P m expiries and P K strikes, set-major -----------
constexpr int SETS_QC = 3;                     // per quote of the table: forward, time to maturity, discount factor

// what the finish with the implied vols adds to the sets' CmcTable: the landing of the results in page-locked host memory
struct CmcSetsTable {
    const double *quote_consts;        // [P K][SETS_QC]
    double *prices, *stderrs;          // [P][K]                          page-locked
    double *stats;                     // [P][m][SVMC_CMC_STATS_DOUBLES]  page-locked
    double *ivols;                     // [P][K]                          page-locked; null: no implied vols
    int m, K;                          // the chain's expiries and quotes
};
// the offsets of the table's P m expiries: set q's expiry i holds strikes [q K + offsets[i], q K + offsets[i + 1])
inline void cmc_sets_offsets(int m, const size_t *offsets, int P, size_t *out /* [P m + 1] */)
{
    const size_t K = offsets[m];
    for (int q = 0; q < P; ++q)
        for (int i = 0; i <= m; ++i) out[static_cast<size_t>(q) * m + i] = q * K + offsets[i];
}
// the image: cmc_image of P m expiries and P K strikes, G groups of up to CMC_KT strikes in the TABLE's coordinates, and the quotes'
// constants where the other tails have their steps
inline CmcImage cmc_sets_image(Layout &w, int m, size_t K, int G, int P)
{
    return cmc_image(w, static_cast<size_t>(P) * m, P * K, G, 0, static_cast<int>(SETS_QC * P * K));
}
// the workspace: the head; stats; prices and errors; the forward and payoff partials -> image bytes
inline size_t cmc_sets_workspace(Layout &w, size_t n_path, int m, size_t K, int G, int P, CmcTable &t, CmcSetsTable &st)
{
    const size_t rows = quote_rows(n_path), PK = P * K, Pm = static_cast<size_t>(P) * m;
    size_t image_bytes;
    const CmcImage im = cmc_table_head(w, n_path, Pm, PK, G, 0, static_cast<int>(SETS_QC * PK), t, image_bytes);
    t.groups = im.groups;
    st.quote_consts = im.steps;
    t.stats = w.take<double>(SVMC_CMC_STATS_DOUBLES * Pm);
    t.out = w.take<double>(2 * PK);
    t.fwd_partials = w.take<double>(rows * 3 * Pm);
    t.pay_partials = w.take<double>(rows * 2 * PK);
    st.m = m;
    st.K = static_cast<int>(K);
    return image_bytes;
}
inline size_t cmc_sets_workspace_bytes_of(size_t n_path, int m, size_t K, int P)
{
    CmcTable t;
    CmcSetsTable st;
    Layout w{nullptr};
    cmc_sets_workspace(w, n_path, m, K, P * quote_groups_bound(m, K, CMC_KT), P, t, st);
    return w.bytes();
}
// the page-locked results of a call: prices, errors [P][K], statistics [P][m][5], implied vols [P][K].  Returns the bytes.
inline size_t cmc_sets_pinned(void *pinned, int m, size_t K, int P, bool want_ivols, CmcSetsTable &st)
{
    Layout w{static_cast<unsigned char *>(pinned)};
    st.prices = w.take<double>(P * K);
    st.stderrs = w.take<double>(P * K);
    st.stats = w.take<double>(static_cast<size_t>(SVMC_CMC_STATS_DOUBLES) * P * m);
    double *ivols = w.take<double>(P * K);
    st.ivols = want_ivols ? ivols : nullptr;
    return w.bytes();
}
// mu / cv rows [P][m], set-major
inline void cmc_sets_fill_image(const CmcImage &im, const double *const *mu, const double *const *cv, const double *ttms, const double *forwards,
                                const double *discfactors, int m, const double *strikes, const int8_t *types, const size_t *offsets, int P,
                                const size_t *table_offsets /* cmc_sets_offsets */)
{
    const int K = static_cast<int>(offsets[m]);
    for (int q = 0; q < P; ++q) {
        const int o = q * K;
        quote_image(m, offsets,
            [&](int i, int k0, int k1) {
                im.expiries[q * m + i] = CmcExpiry{mu[q * m + i], cv[q * m + i], forwards[i], std::log(forwards[i]), discfactors[i], o + k0, o + k1};
            },
            [&](int i, int k) {
                cmc_columns(im.strikes, im.is_put, im.intrinsic, o + k, strikes[k], types[k] == SVMC_PUT, forwards[i]);
                double *qc = im.steps + static_cast<size_t>(SETS_QC) * (o + k);
                qc[0] = forwards[i];
                qc[1] = ttms[i];
                qc[2] = discfactors[i];
            });
    }
    quote_groups(P * m, table_offsets, CMC_KT, false, im.groups);
}

// ---- the Greeks tail on common random numbers ----------------------------------------------------------------------------------
constexpr int GREEKS_KT = SVMC_GREEKS_KT;      // strikes per group: three accumulators and four constants per strike
constexpr int GREEKS_COLS = 4;                 // partial columns per quote: job pass [g - shift, its square, itm, -], pair pass [d, dt, dt^2, count]

// the device table of a call, uploaded once
struct GreeksExpiry {
    double forward, discfactor;
    int k0, k1;                        // its strikes [k0, k1)
};
struct GreeksTable {
    const GreeksExpiry *expiries;      // [m]
    const QuoteGroup *groups;          // [G]
    const double *const *rows;         // [1 + 2P][m]: the jobs' snapshot rows -- base, then up, dn per parameter
    const double *spot_sums;           // [1 + 2P][m][2]: the jobs' [sum F exp(x), count]
    const double *sg;                  // [K] +1 call, -1 put
    const double *c;                   // [K] -sg K
    const double *gshift;              // [K] sg 1{sg (F - K) > 0}: g at the forward, the shift of the delta's sums
    const double *steps;               // [P] h_p
    double *itm_fraction;              // [1 + 2P][K] q = n_itm / n_path of every job, written by the job pass's finish
    double *partials;                  // [rows][slots][K][GREEKS_COLS], slots = 1 + 2P (job pass) | P (pair pass)
    double *base_out;                  // [SVMC_GREEKS_BASE_ROWS][K]
    double *sens_out;                  // [P][SVMC_GREEKS_SENS_ROWS][K]
    int m, K, P;
    unsigned n_rows;
};

// the uploaded image: expiries, groups, row pointers, then the doubles sg / c / gshift [K] and steps [P]
struct GreeksImage {
    GreeksExpiry *expiries;
    QuoteGroup *groups;
    const double **rows;
    double *sg, *c, *gshift, *steps;
};
inline GreeksImage greeks_image(Layout &w, int m, size_t K, int G, int P)
{
    return GreeksImage{w.take<GreeksExpiry>(m), w.take<QuoteGroup>(G), w.take<const double *>(static_cast<size_t>(1 + 2 * P) * m),
                       w.take<double>(K), w.take<double>(K), w.take<double>(K), w.take<double>(P)};
}
// the results, one block: base [SVMC_GREEKS_BASE_ROWS][K], then sens [P][SVMC_GREEKS_SENS_ROWS][K]
struct GreeksResults {
    double *base, *sens;
};
inline GreeksResults greeks_results(Layout &w, size_t K, int P)
{
    return GreeksResults{w.take<double>(SVMC_GREEKS_BASE_ROWS * K), w.take<double>(static_cast<size_t>(SVMC_GREEKS_SENS_ROWS) * P * K)};
}
// the workspace: the image, the results (t.base_out, t.sens_out), every job's in-the-money fractions, the partials.  Returns the
// bytes of the image; t.spot_sums is the caller's.
inline size_t greeks_workspace(Layout &w, size_t n_path, int m, size_t K, int G, int P, GreeksTable &t)
{
    const size_t rows = quote_rows(n_path), J = static_cast<size_t>(1 + 2 * P);
    const GreeksImage im = greeks_image(w, m, K, G, P);
    const size_t image_bytes = w.bytes();
    t.expiries = im.expiries;
    t.groups = im.groups;
    t.rows = im.rows;
    t.sg = im.sg;
    t.c = im.c;
    t.gshift = im.gshift;
    t.steps = im.steps;
    const GreeksResults r = greeks_results(w, K, P);
    t.base_out = r.base;
    t.sens_out = r.sens;
    t.itm_fraction = w.take<double>(J * K);
    t.partials = w.take<double>(rows * J * GREEKS_COLS * K);
    t.m = m;
    t.K = static_cast<int>(K);
    t.P = P;
    t.n_rows = static_cast<unsigned>(rows);
    return image_bytes;
}
inline size_t greeks_payoff_workspace_bytes_of(size_t n_path, int m, size_t K, int P)
{
    GreeksTable t;
    Layout w{nullptr};
    greeks_workspace(w, n_path, m, K, quote_groups_bound(m, K, GREEKS_KT), P, t);
    return w.bytes();
}
// The host block of a call, page-locked in the fused drivers: the image at the group bound -- the launch builds its own, at the chain's
// count, in its head -- then the results, which the fused drivers' kernels store there themselves.  Returns the bytes; *results: the blocks.
inline size_t greeks_pinned(void *pinned, int m, size_t K, int P, GreeksResults *results)
{
    Layout w{static_cast<unsigned char *>(pinned)};
    greeks_image(w, m, K, quote_groups_bound(m, K, GREEKS_KT), P);
    const GreeksResults r = greeks_results(w, K, P);
    if (results != nullptr) *results = r;
    return w.bytes();
}
// rows_host [1 + 2P][m], job-major
inline void greeks_fill_image(const GreeksImage &im, const double *const *rows_host, const double *forwards, const double *discfactors, int m,
                              const double *strikes, const int8_t *types, const size_t *offsets, int P, const double *steps)
{
    quote_image(
        m, offsets, [&](int i, int k0, int k1) { im.expiries[i] = GreeksExpiry{forwards[i], discfactors[i], k0, k1}; },
        [&](int i, int k) {
            const double sgn = (types[k] == SVMC_PUT) ? -1.0 : 1.0;
            im.sg[k] = sgn;
            im.c[k] = -sgn * strikes[k];
            im.gshift[k] = (sgn * (forwards[i] - strikes[k]) > 0.0) ? sgn : 0.0;
        });
    quote_groups(m, offsets, GREEKS_KT, false, im.groups);
    for (int j = 0; j < (1 + 2 * P) * m; ++j) im.rows[j] = rows_host[j];
    for (int p = 0; p < P; ++p) im.steps[p] = steps[p];
}

}  // namespace svmc
