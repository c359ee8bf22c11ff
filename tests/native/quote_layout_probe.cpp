// quote_layout_probe.cpp -- the workspace / image / page-locked layouts and the image builders of csrc/svmc_quotes.h on the host,
// with no GPU and no HIP: tests/test_quote_layout_host.py compiles this file with g++ and runs it.
//
// Per layout function, on the grid n_path in {1, 256, 257, 300000} x (m, K) in {(1, 0), (1, 1), (3, 17), (16, 208), (16, 115 ragged)}
// x P in {1, 6, 31}: the bytes measured with a null base equal the end of the carved walk; every region -- its size restated here
// from what the kernels index, the second description that the library no longer keeps -- is 8-aligned, lies inside the block,
// overlaps no other and together they fill the block; the walk at the chain's actual group count never exceeds the walk at the
// bound the public size functions use.  Per image builder: it writes into a heap block of exactly the image's bytes with a canary
// behind it, and the groups it wrote tile every expiry's strikes exactly once.  Prints one "size" line per grid point (the four
// public workspace sizes, which the test compares with the recorded ones) and "ok"; a failed check prints its place and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "svmc_quotes.h"

using namespace svmc;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::printf("FAILED %s:%d %s [%s]\n", __FILE__, __LINE__, #cond, g_case); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

static char g_case[160];

// a heap block that is never touched: the layouts are walked over it, nothing is stored
static std::unique_ptr<unsigned char[]> untouched(size_t bytes) { return std::unique_ptr<unsigned char[]>(new unsigned char[bytes ? bytes : 1]); }

struct Region {
    const void *p;
    size_t bytes;
};

static size_t align8(size_t b) { return (b + 7) & ~static_cast<size_t>(7); }

// the regions lie 8-aligned inside [base, base + total), none overlaps another, and with their padding they fill the block
static void check_regions(const unsigned char *base, size_t total, const std::vector<Region> &regions)
{
    size_t sum = 0;
    for (size_t a = 0; a < regions.size(); ++a) {
        const unsigned char *p = static_cast<const unsigned char *>(regions[a].p);
        CHECK(p >= base && static_cast<size_t>(p - base) % 8 == 0);
        CHECK(static_cast<size_t>(p - base) + regions[a].bytes <= total);
        sum += align8(regions[a].bytes);
        for (size_t b = 0; b < a; ++b) {
            const unsigned char *q = static_cast<const unsigned char *>(regions[b].p);
            CHECK(regions[a].bytes == 0 || regions[b].bytes == 0 || p + regions[a].bytes <= q || q + regions[b].bytes <= p);
        }
    }
    CHECK(sum == total);
}

static const size_t D = sizeof(double);

static std::vector<Region> cmc_image_regions(const CmcImage &im, size_t m, size_t K, size_t G, size_t GD)
{
    return {{im.expiries, m * sizeof(CmcExpiry)}, {im.groups, G * sizeof(QuoteGroup)}, {im.dgroups, GD * sizeof(QuoteGroup)},
            {im.strikes, K * D}, {im.is_put, K * D}, {im.intrinsic, K * D}, {im.steps, 0}};
}
static void add_cmc_results(std::vector<Region> &r, const CmcResults &res, size_t m, size_t K, size_t d)
{
    r.insert(r.end(), {{res.out, 2 * K * D}, {res.deriv_out, d * 8 * K * D}, {res.stats, m * SVMC_CMC_STATS_DOUBLES * D}, {res.zero, d * m * D}});
}

// the conditional payoff tail (GD = 0) and its derivative tail: workspace and host block at group counts (G, GD); returns the bytes
static size_t probe_cmc(size_t n_path, int m, size_t K, int G, int GD, size_t *pinned_bytes)
{
    const size_t rows = quote_rows(n_path), d = GD > 0 ? 1 : 0, um = m;
    CmcTable t;
    CmcDerivTable dt;
    Layout measure{nullptr};
    const size_t image_measured = cmc_workspace(measure, n_path, m, K, G, GD, t, dt);
    CHECK(t.expiries == nullptr && dt.partials == nullptr);
    const auto block = untouched(measure.bytes());
    Layout w{block.get()};
    CHECK(cmc_workspace(w, n_path, m, K, G, GD, t, dt) == image_measured && w.bytes() == measure.bytes());
    CHECK(t.m == m && t.K == static_cast<int>(K) && t.rows == rows);
    CmcImage im{const_cast<CmcExpiry *>(t.expiries), const_cast<QuoteGroup *>(t.groups), const_cast<QuoteGroup *>(dt.groups),
                const_cast<double *>(t.strikes), const_cast<double *>(t.is_put), const_cast<double *>(t.intrinsic), nullptr};
    im.steps = t.kp;                       // (no steps: the empty region ends the image)
    std::vector<Region> r = cmc_image_regions(im, um, K, G, GD);
    size_t image = 0;
    for (const Region &x : r) image += align8(x.bytes);
    CHECK(image == image_measured);
    r.insert(r.end(), {{t.kp, K * D}, {t.ln_kp, K * D}, {t.shift, K * D}, {t.fwd, um * 4 * D}});
    add_cmc_results(r, CmcResults{t.out, dt.out, t.stats, dt.zero}, um, K, d);
    r.insert(r.end(), {{t.fwd_partials, rows * um * 3 * D}, {t.pay_partials, rows * K * 2 * D}, {dt.shift, d * K * 3 * D},
                       {dt.partials, d * rows * K * CMC_DQ * D}, {dt.zero_partials, d * rows * um * D}});
    check_regions(block.get(), w.bytes(), r);
    // the results are one block in the order the host copies them out: prices, errors, derivatives, statistics, counts
    CHECK(t.out + 2 * K == (d ? dt.out : t.stats) && (!d || (dt.out + 8 * K == t.stats && t.stats + SVMC_CMC_STATS_DOUBLES * um == dt.zero)));

    Layout pm{nullptr};
    cmc_pinned(pm, m, K, G, GD, im);
    const auto host = untouched(pm.bytes());
    Layout ph{host.get()};
    const CmcResults res = cmc_pinned(ph, m, K, G, GD, im);
    CHECK(ph.bytes() == pm.bytes());
    r = cmc_image_regions(im, um, K, G, GD);
    add_cmc_results(r, res, um, K, d);
    check_regions(host.get(), ph.bytes(), r);
    CHECK(static_cast<size_t>(reinterpret_cast<unsigned char *>(res.out) - host.get()) == image_measured);
    *pinned_bytes = pm.bytes();
    return measure.bytes();
}

static std::vector<Region> sens_image_regions(const CmcImage &im, size_t m, size_t K, size_t G, size_t P)
{
    return {{im.expiries, 2 * P * m * sizeof(CmcExpiry)}, {im.groups, G * sizeof(QuoteGroup)}, {im.strikes, 2 * P * K * D},
            {im.is_put, 2 * P * K * D}, {im.intrinsic, 2 * P * K * D}, {im.steps, P * D}};
}

static size_t probe_sens(size_t n_path, int m, size_t K, int G, int P, size_t *pinned_bytes)
{
    const size_t rows = quote_rows(n_path), um = m, uP = P, JK = 2 * uP * K, Jm = 2 * uP * um;
    CmcTable t;
    CmcSensTable st;
    Layout measure{nullptr};
    const size_t image_measured = cmc_sens_workspace(measure, n_path, m, K, G, P, t, st);
    const auto block = untouched(measure.bytes());
    Layout w{block.get()};
    CHECK(cmc_sens_workspace(w, n_path, m, K, G, P, t, st) == image_measured && w.bytes() == measure.bytes());
    CHECK(t.m == static_cast<int>(Jm) && t.K == static_cast<int>(JK) && t.rows == rows && st.P == P && st.m == m && st.K == static_cast<int>(K));
    CHECK(t.groups == nullptr && t.pay_partials == nullptr && t.out == nullptr);
    CmcImage im{const_cast<CmcExpiry *>(t.expiries), const_cast<QuoteGroup *>(st.groups), nullptr, const_cast<double *>(t.strikes),
                const_cast<double *>(t.is_put), const_cast<double *>(t.intrinsic), const_cast<double *>(st.steps)};
    std::vector<Region> r = sens_image_regions(im, um, K, G, uP);
    size_t image = 0;
    for (const Region &x : r) image += align8(x.bytes);
    CHECK(image == image_measured);
    r.insert(r.end(), {{t.kp, JK * D}, {t.ln_kp, JK * D}, {t.shift, JK * D}, {t.fwd, Jm * 4 * D}, {t.stats, Jm * SVMC_CMC_STATS_DOUBLES * D},
                       {t.fwd_partials, rows * Jm * 3 * D}, {st.q_partials, rows * JK * D}, {st.q, JK * D}, {st.pair_shift, uP * K * 2 * D},
                       {st.pair_partials, rows * uP * K * SENS_PQ * D}, {st.out, uP * SVMC_CMC_SENS_ROWS * K * D}});
    check_regions(block.get(), w.bytes(), r);

    // the host block: the image at the bound, then the landing; the image at this call's count fits in front of the landing
    const size_t pinned = cmc_sens_pinned(nullptr, m, K, P, nullptr), bound = quote_groups_bound(m, K, SENS_KT);
    const auto host = untouched(pinned);
    Layout pi{host.get()};
    double *out = nullptr;
    CHECK(cmc_sens_pinned(host.get(), m, K, P, &out) == pinned);
    r = sens_image_regions(cmc_sens_image(pi, m, K, static_cast<int>(bound), P), um, K, bound, uP);
    r.push_back({out, uP * SVMC_CMC_SENS_ROWS * K * D});
    check_regions(host.get(), pinned, r);
    CHECK(static_cast<size_t>(G) <= bound && host.get() + image_measured <= reinterpret_cast<unsigned char *>(out));
    *pinned_bytes = pinned;
    return measure.bytes();
}

static std::vector<Region> greeks_image_regions(const GreeksImage &im, size_t m, size_t K, size_t G, size_t P)
{
    return {{im.expiries, m * sizeof(GreeksExpiry)}, {im.groups, G * sizeof(QuoteGroup)}, {im.rows, (1 + 2 * P) * m * sizeof(double *)},
            {im.sg, K * D}, {im.c, K * D}, {im.gshift, K * D}, {im.steps, P * D}};
}

static size_t probe_greeks(size_t n_path, int m, size_t K, int G, int P, size_t *pinned_bytes)
{
    const size_t rows = quote_rows(n_path), um = m, uP = P, J = 1 + 2 * uP;
    GreeksTable t;
    Layout measure{nullptr};
    const size_t image_measured = greeks_workspace(measure, n_path, m, K, G, P, t);
    const auto block = untouched(measure.bytes());
    Layout w{block.get()};
    CHECK(greeks_workspace(w, n_path, m, K, G, P, t) == image_measured && w.bytes() == measure.bytes());
    CHECK(t.m == m && t.K == static_cast<int>(K) && t.P == P && t.n_rows == rows);
    GreeksImage im{const_cast<GreeksExpiry *>(t.expiries), const_cast<QuoteGroup *>(t.groups), const_cast<const double **>(t.rows),
                   const_cast<double *>(t.sg), const_cast<double *>(t.c), const_cast<double *>(t.gshift), const_cast<double *>(t.steps)};
    std::vector<Region> r = greeks_image_regions(im, um, K, G, uP);
    size_t image = 0;
    for (const Region &x : r) image += align8(x.bytes);
    CHECK(image == image_measured);
    r.insert(r.end(), {{t.base_out, SVMC_GREEKS_BASE_ROWS * K * D}, {t.sens_out, uP * SVMC_GREEKS_SENS_ROWS * K * D}, {t.itm_fraction, J * K * D},
                       {t.partials, rows * J * K * GREEKS_COLS * D}});
    check_regions(block.get(), w.bytes(), r);
    CHECK(t.base_out + SVMC_GREEKS_BASE_ROWS * K == t.sens_out);         // (one block: the stand-alone entry copies both out of it)

    // the host block: the image at the bound, then the results; the image at this call's count fits in front of the results
    const size_t pinned = greeks_pinned(nullptr, m, K, P, nullptr), bound = quote_groups_bound(m, K, GREEKS_KT);
    const auto host = untouched(pinned);
    Layout pi{host.get()};
    GreeksResults res{nullptr, nullptr};
    CHECK(greeks_pinned(host.get(), m, K, P, &res) == pinned);
    r = greeks_image_regions(greeks_image(pi, m, K, static_cast<int>(bound), P), um, K, bound, uP);
    r.insert(r.end(), {{res.base, SVMC_GREEKS_BASE_ROWS * K * D}, {res.sens, uP * SVMC_GREEKS_SENS_ROWS * K * D}});
    check_regions(host.get(), pinned, r);
    CHECK(static_cast<size_t>(G) <= bound && host.get() + image_measured <= reinterpret_cast<unsigned char *>(res.base));
    *pinned_bytes = pinned;
    return measure.bytes();
}

// ---- the groups and the image builders ------------------------------------------------------------------------------------------
// the groups tile every expiry's [k0, k1) exactly once in order; one_for_empty: one nk = 0 group for an expiry without strikes;
// pad = 1 on each expiry's first group only
static void check_groups(const QuoteGroup *g, int count, int m, const size_t *offsets, int kt, bool one_for_empty)
{
    CHECK(count == quote_groups(m, offsets, kt, one_for_empty) && count <= quote_groups_bound(m, offsets[m], kt));
    int at = 0;
    for (int i = 0; i < m; ++i) {
        const int k0 = static_cast<int>(offsets[i]), k1 = static_cast<int>(offsets[i + 1]);
        if (k0 == k1 && one_for_empty) {
            CHECK(at < count && g[at].expiry == i && g[at].nk == 0 && g[at].pad == 1 && g[at].k0 == 0);
            ++at;
        }
        for (int k = k0; k < k1; ++at) {
            CHECK(at < count && g[at].expiry == i && g[at].k0 == k && g[at].nk >= 1 && g[at].nk <= kt && k + g[at].nk <= k1);
            CHECK((k + g[at].nk == k1 || g[at].nk == kt) && g[at].pad == (k == k0 ? 1 : 0));
            k += g[at].nk;
        }
    }
    CHECK(at == count);
}

// a heap block of exactly `bytes` for an image, with a canary behind it
struct Guarded {
    static constexpr size_t CANARY = 64;
    std::vector<unsigned char> mem;
    explicit Guarded(size_t bytes) : mem(bytes + CANARY, 0xA5) {}
    bool intact() const
    {
        for (size_t i = mem.size() - CANARY; i < mem.size(); ++i)
            if (mem[i] != 0xA5) return false;
        return true;
    }
};

static void probe_images(int m, const size_t *offsets, int P)
{
    const size_t K = offsets[m];
    std::vector<double> forwards(m), dfs(m), strikes(K), steps(P), row(1);
    std::vector<int8_t> types(K);
    for (int i = 0; i < m; ++i) forwards[i] = 1.0 + 0.01 * i, dfs[i] = 1.0 - 0.01 * i;
    for (size_t k = 0; k < K; ++k) strikes[k] = 0.7 + 0.005 * static_cast<double>(k), types[k] = static_cast<int8_t>((k % 3 == 0) ? SVMC_PUT : SVMC_CALL);
    for (int p = 0; p < P; ++p) steps[p] = 0.01 * (p + 1);
    std::vector<const double *> rows(static_cast<size_t>(1 + 2 * P) * m, row.data());
    for (size_t j = 0; j < rows.size(); ++j) rows[j] = row.data() + j;         // (told apart, never read)

    for (int deriv = 0; deriv <= 1; ++deriv) {
        const int G = quote_groups(m, offsets, CMC_KT, false), GD = deriv ? quote_groups(m, offsets, CMC_DKT, true) : 0;
        Layout measure{nullptr};
        cmc_image(measure, m, K, G, GD, 0);
        Guarded block(measure.bytes());
        Layout w{block.mem.data()};
        const CmcImage im = cmc_image(w, m, K, G, GD, 0);
        cmc_fill_image(im, rows.data(), rows.data() + m, forwards.data(), dfs.data(), m, strikes.data(), types.data(), offsets, deriv != 0);
        CHECK(block.intact());
        check_groups(im.groups, G, m, offsets, CMC_KT, false);
        if (deriv) check_groups(im.dgroups, GD, m, offsets, CMC_DKT, true);
        for (int i = 0; i < m; ++i) {
            const CmcExpiry &e = im.expiries[i];
            CHECK(e.mu == rows[i] && e.cv == rows[m + i] && e.forward == forwards[i] && e.discfactor == dfs[i]);
            CHECK(e.k0 == static_cast<int>(offsets[i]) && e.k1 == static_cast<int>(offsets[i + 1]));
            for (int k = e.k0; k < e.k1; ++k) {
                const double want = types[k] == SVMC_PUT ? strikes[k] - forwards[i] : forwards[i] - strikes[k];
                CHECK(im.strikes[k] == strikes[k] && im.is_put[k] == (types[k] == SVMC_PUT ? 1.0 : 0.0) && im.intrinsic[k] == (want > 0.0 ? want : 0.0));
            }
        }
    }
    {
        const int G = quote_groups(m, offsets, SENS_KT, false), iK = static_cast<int>(K);
        Layout measure{nullptr};
        cmc_sens_image(measure, m, K, G, P);
        Guarded block(measure.bytes());
        Layout w{block.mem.data()};
        const CmcImage im = cmc_sens_image(w, m, K, G, P);
        const double *const *r = rows.data();      // up_mu = rows [0, P m), then up_cv, dn_mu, dn_cv
        cmc_sens_fill_image(im, r, r + P * m, r, r + P * m, forwards.data(), dfs.data(), m, strikes.data(), types.data(), offsets, P, steps.data());
        CHECK(block.intact());
        check_groups(im.groups, G, m, offsets, SENS_KT, false);
        for (int j = 0; j < 2 * P; ++j)
            for (int i = 0; i < m; ++i) {
                const CmcExpiry &e = im.expiries[j * m + i];
                CHECK(e.mu == rows[(j / 2) * m + i] && e.cv == rows[(P + j / 2) * m + i] && e.forward == forwards[i]);
                CHECK(e.k0 == j * iK + static_cast<int>(offsets[i]) && e.k1 == j * iK + static_cast<int>(offsets[i + 1]));
                for (int k = e.k0; k < e.k1; ++k) CHECK(im.strikes[k] == strikes[k - j * iK] && im.is_put[k] == (types[k - j * iK] == SVMC_PUT ? 1.0 : 0.0));
            }
        for (int p = 0; p < P; ++p) CHECK(im.steps[p] == steps[p]);
    }
    {
        const int G = quote_groups(m, offsets, GREEKS_KT, false);
        Layout measure{nullptr};
        greeks_image(measure, m, K, G, P);
        Guarded block(measure.bytes());
        Layout w{block.mem.data()};
        const GreeksImage im = greeks_image(w, m, K, G, P);
        greeks_fill_image(im, rows.data(), forwards.data(), dfs.data(), m, strikes.data(), types.data(), offsets, P, steps.data());
        CHECK(block.intact());
        check_groups(im.groups, G, m, offsets, GREEKS_KT, false);
        for (size_t j = 0; j < rows.size(); ++j) CHECK(im.rows[j] == rows[j]);
        for (int i = 0; i < m; ++i) {
            CHECK(im.expiries[i].k0 == static_cast<int>(offsets[i]) && im.expiries[i].k1 == static_cast<int>(offsets[i + 1]));
            for (size_t k = offsets[i]; k < offsets[i + 1]; ++k) {
                const double sg = types[k] == SVMC_PUT ? -1.0 : 1.0;
                CHECK(im.sg[k] == sg && im.c[k] == -sg * strikes[k] && im.gshift[k] == (sg * (forwards[i] - strikes[k]) > 0.0 ? sg : 0.0));
            }
        }
        for (int p = 0; p < P; ++p) CHECK(im.steps[p] == steps[p]);
    }
}

int main()
{
    const size_t ns[] = {1, 256, 257, 300000};
    const int Ps[] = {1, 6, 31};
    // (m, the strikes of each expiry): the grid's four chains in even cuts, and 16 ragged expiries with empty ones
    const std::vector<std::vector<size_t>> chains = {{0}, {1}, {9, 0, 8}, std::vector<size_t>(16, 13), {1, 0, 9, 8, 0, 4, 5, 3, 12, 0, 16, 7, 2, 0, 31, 17}};
    for (const std::vector<size_t> &counts : chains) {
        const int m = static_cast<int>(counts.size());
        std::vector<size_t> offsets(1, 0);
        for (size_t c : counts) offsets.push_back(offsets.back() + c);
        const size_t K = offsets.back();
        for (int P : Ps) {
            std::snprintf(g_case, sizeof g_case, "images m %d K %zu P %d", m, K, P);
            probe_images(m, offsets.data(), P);
            for (size_t n : ns) {
                std::snprintf(g_case, sizeof g_case, "layouts n %zu m %d K %zu P %d", n, m, K, P);
                size_t size[4][2], pinned[4][2];       // [payoff, derivative, sensitivity, Greeks][at the bound, at the actual count]
                for (int actual = 0; actual <= 1; ++actual) {
                    const auto groups = [&](int kt, bool one_for_empty) {
                        return actual ? quote_groups(m, offsets.data(), kt, one_for_empty) : quote_groups_bound(m, K, kt);
                    };
                    size[0][actual] = probe_cmc(n, m, K, groups(CMC_KT, false), 0, &pinned[0][actual]);
                    size[1][actual] = probe_cmc(n, m, K, groups(CMC_KT, false), groups(CMC_DKT, true), &pinned[1][actual]);
                    size[2][actual] = probe_sens(n, m, K, groups(SENS_KT, false), P, &pinned[2][actual]);
                    size[3][actual] = probe_greeks(n, m, K, groups(GREEKS_KT, false), P, &pinned[3][actual]);
                }
                for (int f = 0; f < 4; ++f) CHECK(size[f][1] <= size[f][0] && pinned[f][1] <= pinned[f][0]);
                // what the public size functions and the fused drivers allocate: the walks at the bound
                CHECK(size[0][0] == cmc_workspace_bytes_of(n, m, K, false) && size[1][0] == cmc_workspace_bytes_of(n, m, K, true));
                CHECK(size[2][0] == cmc_sens_workspace_bytes_of(n, m, K, P) && size[3][0] == greeks_payoff_workspace_bytes_of(n, m, K, P));
                CHECK(pinned[0][0] == cmc_pinned_bytes_of(m, K, false) && pinned[1][0] == cmc_pinned_bytes_of(m, K, true));
                std::printf("size %zu %d %zu %d %zu %zu %zu %zu\n", n, m, K, P, size[0][0], size[1][0], size[2][0], size[3][0]);
            }
        }
    }
    std::printf("ok\n");
    return 0;
}
