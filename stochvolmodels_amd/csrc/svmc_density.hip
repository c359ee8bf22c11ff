// svmc_density.hip -- model densities, digital options and histograms on gfx950: DESIGN.md row f6.
//
//   mgf_pdf_slice_kernel       one block per space point z_i = (space_i - shift) / scale: the bin mass
//                              dx sum_j Re[ (w_j / pi) exp(z_i u_j + log E_j) ] over the transform grid u   (utils/mgf_pricer.py:361-384)
//   mgf_digital_slice_kernel   one block per strike: sum_j Re[ p_j exp(-x_K phi_j + log E_j) ], p_j = -+(w_j / pi) / phi_j
//                              (utils/mgf_pricer.py:224-269; the C / P complement and the discount factor are the host's)
//   mgf_il_slice_kernel        one block per impermanent-loss case (forward, range): the five sums of row f10, described where it stands
//   histogram_uniform_kernel   integer counts of a state vector on equal bins with np.histogram's semantics: per-block counts in
//                              LDS, one 64-bit integer atomic per non-empty bin and block
//   kde_* kernels              the Gaussian kernel density estimate of a state vector, plain (row f7) and, as their WEIGHTED
//                              instantiation, with a weight per sample (row f9); described where they stand
//
// The weights w are the reference's LEGACY pricer weights (:157-171), as mgf_vanilla_slice_kernel forms them: Simpson 1,4,2,...
// with every odd index 4 (an even-length grid keeps 4 on its last point), or for is_simpson = 0 half the first step on the
// first point and the local step p_j - p_(j-1) on the others.
//
// Decomposition of the density kernel: a block per space point, 256 threads striding the grid.  The kernel is bound by the
// fp64 exp and sincos of each term (a few hundred instructions against 32 bytes read), the transform and the log-MGF of the
// longest grid (40 000 points) are 1.3 MB that every block re-reads from L2, and a figure's 200 space points are already 800
// waves; a tile of space points per block would share loads that cost nothing and leave fewer, longer blocks.  The order of
// the sum over j depends on the grid length alone -- thread t adds j = t, t + 256, ... in order, the 64 lanes of a wave meet in
// one shuffle tree and the four waves are added in order -- so a set of a batch (blockIdx.y) is bit-equal to the set alone.
#include "svmc_internal.h"

#include <cmath>

#include "svmc_math.h"
#include "svmc_complex.h"
#include "svmc_slice.h"
#include "svmc_mgf_slice.h"

namespace svmc {

constexpr int MAX_PDF_SETS = 64;         // parameter sets per launch (kernel-argument block: 64 x 16 B)

struct PdfSets {
    double shift[MAX_PDF_SETS];
    double scale[MAX_PDF_SETS];
};

__global__ __launch_bounds__(MGF_SLICE_BLOCK) void mgf_pdf_slice_kernel(const cd *__restrict__ u, const cd *__restrict__ log_mgf,
                                                                        int n_grid, const double *__restrict__ space, int n_space,
                                                                        PdfSets ps, int is_simpson, double *__restrict__ pdf)
{
    __shared__ double lds[4];
    const int set = blockIdx.y;                                       // the parameter set of a batched call
    u += static_cast<size_t>(set) * n_grid;
    log_mgf += static_cast<size_t>(set) * n_grid;
    space += static_cast<size_t>(set) * n_space;
    pdf += static_cast<size_t>(set) * n_space;
    const double z = (space[blockIdx.x] - ps.shift[set]) / ps.scale[set];                       // :379
    const double h = u[1].im - u[0].im;
    const double total = mgf_slice_nansum(n_grid, lds, [&](int j) {
        const double w = legacy_weight(u, j, n_grid, h, is_simpson) / PI;                       // :375-377
        const cd uj = u[j], lm = log_mgf[j];
        const cd e = cexp_(cd{z * uj.re + lm.re, z * uj.im + lm.im});
        return w * e.re;                                                                        // nansum :381
    });
    if (threadIdx.x == 0) pdf[blockIdx.x] = (space[1] - space[0]) * total;                      // :382-383
}

__global__ __launch_bounds__(MGF_SLICE_BLOCK) void mgf_digital_slice_kernel(const cd *__restrict__ phi,
                                                                            const cd *__restrict__ log_mgf, int n_grid,
                                                                            SliceStrikes da, int negative_contour, int is_simpson,
                                                                            double *__restrict__ sums, int sums_ld)
{
    __shared__ double lds[4];
    phi += static_cast<size_t>(blockIdx.y) * n_grid;                  // blockIdx.y: the parameter set of a batched call
    log_mgf += static_cast<size_t>(blockIdx.y) * n_grid;
    sums += static_cast<size_t>(blockIdx.y) * sums_ld;
    const double x = da.x[blockIdx.x];
    const double h = phi[1].im - phi[0].im;
    const double total = mgf_slice_nansum(n_grid, lds, [&](int j) {
        const double a = legacy_weight(phi, j, n_grid, h, is_simpson) / PI;
        const cd b = phi[j];
        cd p = real_over_complex(a, b);                                                         // as NumPy divides
        if (negative_contour) p = -p;                                                           // calls :244, puts :247
        const cd arg = log_mgf[j] - x * b;
        cd e = cexp_(arg);
        // exp(r + 0i) = exp(r) + 0i as C99's cexp and NumPy's: at r = +inf (a log E of +inf at the money, x = 0, or on the
        // grid's first point, Im phi = 0) inf * sin(0) is NaN, and with the complex p the whole term would be dropped where the
        // reference keeps Re[p] inf.  For a finite r the product is this signed zero already: no other term changes a bit.
        if (arg.im == 0.0) e.im = arg.im;
        return p.re * e.re - p.im * e.im;                                                       // nansum :253
    });
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// ---- impermanent loss of a liquidity range [pa, pb] from the transform: DESIGN.md row f10 -------------------------------------
// The five sums the reference's logsv_il_pricer composes (papers/il_hedging/run_logsv_for_il_payoff.py), for the case
// (x, xa, xb) = (log p1, log pa, log pb) of blockIdx.x and the parameter set of blockIdx.y, each through mgf_slice_nansum -- five
// passes over the grid, every one in the family's fixed order, so a case of a batch is bit-equal to the case alone:
//   0  square root   Re[ (v_j / pi) (exp((phi + 1/2) xb - phi x) - exp((phi + 1/2) xa - phi x)) / (phi + 1/2) exp(log E_j) ]  (:113-120)
//   1  vanilla, pa   Re[ -(w_j / pi) / ((phi + 1) phi) exp(-(x - xa) phi + log E_j) ]   (utils/mgf_pricer.py:197, spot measure)
//   2  vanilla, pb   the same with x - xb
//   3  digital, pa   Re[ (w_j / pi) / phi exp(-(x - xa) phi + log E_j) ]: mgf_digital_slice_kernel's term on its put side; the
//   4  digital, pb   host changes the sign of the SUM on a contour with every Re phi < 0 (the same bits as negated terms)
// w: the legacy weights; v: the validated weights of compute_integration_weights -- Simpson's are the legacy ones on the odd
// grids that rule accepts, the trapezoid's are one step with half a step on the first AND the last point.  The complex divisions
// are NumPy's (Smith's form).  NaN terms are dropped, inf is kept, a log E of -inf gives a zero term.  A log E of +inf: the
// exponential's real part is inf cos and its imaginary part inf sin, and where the imaginary part of the exponent is exactly 0
// it is kept 0 as C99's cexp and NumPy's do (mgf_digital_slice_kernel's rule), so that point contributes Re[p] inf and not NaN;
// elsewhere the product is inf - inf = NaN (dropped) or a signed inf (kept), as NumPy's product of the same factors gives.
// Five passes and not one pass of five sums: mgf_slice_nansum stays the family's only sum loop.  They do show: 256 cases x 1 001
// points take 154 us in eight launches where the digital entry takes 43 us for 256 strikes (profiles/il_bench.json: 19 us a
// launch against a launch floor of 5).  A profile of 1 001 forwards is 1.1 ms with the ODE launch against the reference's second
// per forward; widening the loop to carry five sums is the step after this one and is not taken here.
constexpr int IL_SLICE_SUMS = SVMC_IL_SLICE_SUMS;

struct IlSliceCases {
    double x[MGF_SLICE_STRIKES], xa[MGF_SLICE_STRIKES], xb[MGF_SLICE_STRIKES];     // 768 B of kernel arguments
};

__global__ __launch_bounds__(MGF_SLICE_BLOCK) void mgf_il_slice_kernel(const cd *__restrict__ phi, const cd *__restrict__ log_mgf,
                                                                       int n_grid, IlSliceCases ca, int is_simpson,
                                                                       double *__restrict__ sums, int sums_ld)
{
    __shared__ double lds[4];
    phi += static_cast<size_t>(blockIdx.y) * n_grid;                  // blockIdx.y: the parameter set of a batched call
    log_mgf += static_cast<size_t>(blockIdx.y) * n_grid;
    sums += static_cast<size_t>(blockIdx.y) * sums_ld + static_cast<size_t>(IL_SLICE_SUMS) * blockIdx.x;
    const double x = ca.x[blockIdx.x], xa = ca.xa[blockIdx.x], xb = ca.xb[blockIdx.x];
    const double h = phi[1].im - phi[0].im;
    const auto store = [&](int k, double total) {
        if (threadIdx.x == 0) sums[k] = total;
        __syncthreads();                                              // every thread has read the wave totals: lds may be written again
    };
    // exp(arg) with the imaginary part of a real exponent kept (see above)
    const auto cexp_real_kept = [](cd arg) {
        cd e = cexp_(arg);
        if (arg.im == 0.0) e.im = arg.im;
        return e;
    };
    store(0, mgf_slice_nansum(n_grid, lds, [&](int j) {
        const double v = (is_simpson ? legacy_weight(phi, j, n_grid, h, 1) : ((j == 0 || j == n_grid - 1) ? 0.5 * h : h)) / PI;
        const cd b = phi[j], bh = b + 0.5;
        const cd eb = cexp_(cd{bh.re * xb - b.re * x, bh.im * xb - b.im * x});
        const cd ea = cexp_(cd{bh.re * xa - b.re * x, bh.im * xa - b.im * x});
        const cd p = complex_over_complex(v * (eb - ea), bh);                                   // :118-119
        const cd e = cexp_real_kept(log_mgf[j]);
        return p.re * e.re - p.im * e.im;                                                       // nansum :120
    }));
    for (int piece = 0; piece < 4; ++piece) {                         // (block-uniform)
        const double xk = x - ((piece & 1) ? xb : xa);
        const bool vanilla = piece < 2;
        store(1 + piece, mgf_slice_nansum(n_grid, lds, [&](int j) {
            const double a = legacy_weight(phi, j, n_grid, h, is_simpson) / PI;
            const cd b = phi[j];
            const cd p = vanilla ? -real_over_complex(a, (b + 1.0) * b) : real_over_complex(a, b);
            const cd e = cexp_real_kept(log_mgf[j] - xk * b);
            return p.re * e.re - p.im * e.im;
        }));
    }
}

// np.histogram(a, bins=n_bins, range=(lo, hi)) on equal bins, NumPy's own steps: values outside [lo, hi] and NaNs are dropped; the
// index is trunc(((a - lo) / (hi - lo)) n_bins), n_bins folded into the last bin, then corrected against the edges (the
// host's linspace(lo, hi, n_bins + 1)): one down where a < edge[i], one up where a >= edge[i + 1] except in the last bin, which
// owns `hi`.  `divisor` divides the value first (ttm for the annualised quadratic variance, as the host's qvar / ttm; 1 is exact).
// Counts are integers and integer addition commutes: the result does not depend on the order the atomics arrive in.
constexpr int HIST_BLOCK = 256;
constexpr int HIST_MAX_BINS = 8192;      // 32 KB of LDS counters
constexpr int HIST_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(HIST_BLOCK) void histogram_uniform_kernel(const double *__restrict__ a, size_t n, double divisor,
                                                                       const double *__restrict__ edges, int n_bins,
                                                                       unsigned long long *__restrict__ counts)
{
    extern __shared__ unsigned int bins[];
    for (int b = threadIdx.x; b < n_bins; b += HIST_BLOCK) bins[b] = 0u;
    __syncthreads();
    const double lo = edges[0], hi = edges[n_bins], width = hi - lo;
    for (size_t p = static_cast<size_t>(blockIdx.x) * HIST_BLOCK + threadIdx.x; p < n;
         p += static_cast<size_t>(gridDim.x) * HIST_BLOCK) {
        const double v = a[p] / divisor;
        if (!(v >= lo && v <= hi)) continue;                          // outside the range, or NaN
        int i = static_cast<int>(((v - lo) / width) * n_bins);
        i = (i >= n_bins) ? n_bins - 1 : (i < 0 ? 0 : i);             // n_bins -> the last bin; the clamp keeps every read below in bounds
        if (i > 0 && v < edges[i]) --i;
        if (i != n_bins - 1 && v >= edges[i + 1]) ++i;
        atomicAdd(&bins[i], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < n_bins; b += HIST_BLOCK) {
        const unsigned int c = bins[b];
        if (c != 0u) atomicAdd(&counts[b], static_cast<unsigned long long>(c));
    }
}

// ---- Gaussian kernel density estimate of a resident state vector, plain and weighted: DESIGN.md rows f7 and f9 ---------------
// scipy.stats.gaussian_kde(kept)(points) written out (reference pricers/model_pricer.py:243-265): the sample is a[i] / divisor;
// NaNs and samples beyond +-limit (strict comparisons) are dropped and counted; mean and variance of the kept samples in two
// passes as np.cov takes them; h = sqrt(var) factor with Scott's factor n_kept^(-1/5) unless one is given;
// density_j = sum_i exp(-((g_j - v_i) / h)^2 / 2) / (n_kept h sqrt(2 pi)).  The six launches (W: the template argument WEIGHTED):
//
//   kde_moments_kernel<W, 1>      per block [kept, NaN, low, high, sum v]          kde_moments_finish_kernel<W, 1>   counts, mean
//   kde_moments_kernel<W, 2>      per block sum (v - mean)^2, mean from the block  kde_moments_finish_kernel<W, 2>   var, h
//   kde_gaussian_kernel<W>        block (x, y): the KDE_TILE points of tile x against the samples of chunk y; a thread keeps the
//                                 tile in registers and streams its samples past it (one 8-byte load and one division feed
//                                 KDE_TILE exponentials); partials[y][point]
//   kde_finish_kernel<W>          a thread per point adds its chunks in order and scales by 1 / (n_kept h sqrt(2 pi))
//
// Every launch after the first reads what it needs (mean, h, n_kept) from the stats block on the device: no host round trip.
// Order of every sum: a thread adds its samples in index order, the 64 lanes of a wave meet in one shuffle tree, the four waves
// are added in order, the blocks / chunks in order.  The grids of the moment kernels and the chunk length are functions of n
// alone (kde_chunk_length, kde_moment_blocks) and a point's sum does not depend on the tile it sits in: the density of a
// vector at a point is the same bits whatever other points, vectors or gammas share the call.
//
// WEIGHTED is scipy.stats.gaussian_kde(kept, weights=w_kept)(points) (include/svmc.h states the semantics): the weight
// w = weights[i] exp_full(gamma tilt[i]), either factor 1 where its vector is NULL, is formed once per sample (one or two more
// 8-byte loads, with a tilt one more exp_full) and multiplies the sample's terms; a sample whose value passes the filter is dropped
// for its weight, and counted, unless w >= 0 with w and w^2 finite.  The first moment pass carries [kept, NaN, low, high, bad
// weight, sum w, sum w^2, sum w v]; sw = sum w, sw2 = sum w^2, mean = sum w v / sw, var = sum w (v - mean)^2 / (sw - sw2 / sw) as
// np.cov(aweights=w, ddof=1), neff = sw^2 / sw2 in Scott's factor, and sw takes n_kept's place in the last scaling.  KdeLayout
// and the `if constexpr (WEIGHTED)` branches are all that differs: the plain instantiation has no weight to load, test or
// multiply by.  With both vectors NULL the weighted one has w the literal 1.0 and every product with it is exact: sum w =
// sum w^2 = n_kept, sum w v = sum v, sw - sw2 / sw = n_kept - 1 and neff = sw (sw / sw2) = n_kept, so its density and stats
// EQUAL the plain instantiation's.
constexpr int KDE_BLOCK = 256;
constexpr int KDE_TILE = SVMC_KDE_TILE;
constexpr size_t KDE_MIN_CHUNK = 2048;       // samples per chunk up to 2^19 samples: 8 per thread, 64 exponentials against a
constexpr size_t KDE_MAX_CHUNKS = 256;       // block reduction of ~200 instructions; beyond that 256 chunks of n / 256
constexpr int KDE_MOMENT_BLOCKS = 256;       // most blocks of a moment pass (their partials fit one finishing block)
constexpr size_t KDE_MOMENT_PER_BLOCK = 2048;
static_assert(KDE_BLOCK == 256 && KDE_MOMENT_BLOCKS <= KDE_BLOCK, "block_sum_rows adds four waves");

// rows of the first moment pass, the stats block (the first four entries are shared) and the normaliser of the last scaling
template <bool WEIGHTED> struct KdeLayout;
template <> struct KdeLayout<false> {
    enum { N_KEPT = 0, N_NAN, N_LOW, N_HIGH, MEAN, VAR, H, FACTOR, ROWS = 5, NORM = N_KEPT };
    static_assert(FACTOR + 1 == SVMC_KDE_STATS_DOUBLES, "stats block layout");
};
template <> struct KdeLayout<true> {
    enum { N_KEPT = 0, N_NAN, N_LOW, N_HIGH, N_BAD_WEIGHT, SUM_W, NEFF, MEAN, VAR, H, FACTOR, SUM_W2, ROWS = 8, NORM = SUM_W };
    static_assert(SUM_W2 + 1 == SVMC_KDE_WEIGHTED_STATS_DOUBLES, "weighted stats block layout");
};

inline size_t kde_chunk_length(size_t n)
{
    const size_t per = (n + KDE_MAX_CHUNKS - 1) / KDE_MAX_CHUNKS;
    const size_t len = (per + KDE_BLOCK - 1) / KDE_BLOCK * KDE_BLOCK;
    return len < KDE_MIN_CHUNK ? KDE_MIN_CHUNK : len;
}

inline unsigned kde_moment_blocks(size_t n)
{
    const size_t want = (n + KDE_MOMENT_PER_BLOCK - 1) / KDE_MOMENT_PER_BLOCK;
    return static_cast<unsigned>(want < static_cast<size_t>(KDE_MOMENT_BLOCKS) ? want : KDE_MOMENT_BLOCKS);
}

// NV block sums in the fixed order of block_sum; every thread of the first NV holds sum k in thread k
template <int NV>
__device__ __forceinline__ void block_sum_rows(double (&v)[NV], double (*lds)[4])
{
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const double s = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0) lds[k][threadIdx.x >> 6] = s;
    }
    __syncthreads();
}

__device__ __forceinline__ double rows_total(const double (*lds)[4], int k) { return ((lds[k][0] + lds[k][1]) + lds[k][2]) + lds[k][3]; }

struct KdeWeight {                           // what WEIGHTED reads; the plain kernels carry it unread
    const double *weights, *tilt;
    double gamma;
};

// w_i; NaN, negative and overflowed weights come out as they are and fail kde_weight_kept
template <bool WEIGHTED>
__device__ __forceinline__ double kde_weight(const KdeWeight &wt, size_t p)
{
    if constexpr (!WEIGHTED) return 1.0;
    else {
        double w = wt.weights ? wt.weights[p] : 1.0;
        if (wt.tilt) w *= exp_full(wt.gamma * wt.tilt[p]);
        return w;
    }
}

template <bool WEIGHTED>
__device__ __forceinline__ bool kde_weight_kept(double w)
{
    if constexpr (!WEIGHTED) return true;
    else return w >= 0.0 && w * w < __builtin_huge_val();                      // w^2 finite: so is w
}

// w e, or e as it stands: the plain sums hold no product with 1.0 for the compiler to fold
template <bool WEIGHTED>
__device__ __forceinline__ double kde_times_weight(double w, double e)
{
    if constexpr (WEIGHTED) return w * e;
    else return e;
}

template <bool WEIGHTED, int PASS>
__global__ __launch_bounds__(KDE_BLOCK) void kde_moments_kernel(const double *__restrict__ a, KdeWeight wt, size_t n, double divisor,
                                                                double limit, const double *__restrict__ stats,
                                                                double *__restrict__ partials)
{
    using L = KdeLayout<WEIGHTED>;
    constexpr int NV = (PASS == 1) ? L::ROWS : 1;
    __shared__ double lds[NV][4];
    const double mean = (PASS == 2) ? stats[L::MEAN] : 0.0;
    double acc[NV] = {};
    for (size_t p = static_cast<size_t>(blockIdx.x) * KDE_BLOCK + threadIdx.x; p < n; p += static_cast<size_t>(gridDim.x) * KDE_BLOCK) {
        const double v = a[p] / divisor;
        const double w = kde_weight<WEIGHTED>(wt, p);
        const bool is_nan = v != v, high = v > limit, low = v < -limit;
        const bool passed = !(is_nan || high || low);
        const bool kept = passed && kde_weight_kept<WEIGHTED>(w);
        if constexpr (PASS == 1) {
            acc[0] += kept ? 1.0 : 0.0;
            acc[1] += is_nan ? 1.0 : 0.0;
            acc[2] += low ? 1.0 : 0.0;
            acc[3] += high ? 1.0 : 0.0;
            if constexpr (WEIGHTED) {
                acc[4] += (passed && !kept) ? 1.0 : 0.0;
                acc[5] += kept ? w : 0.0;
                acc[6] += kept ? w * w : 0.0;
                acc[7] += kept ? w * v : 0.0;
            } else {
                acc[4] += kept ? v : 0.0;
            }
        } else {
            const double d = v - mean;
            acc[0] += kept ? kde_times_weight<WEIGHTED>(w, d * d) : 0.0;
        }
    }
    block_sum_rows<NV>(acc, lds);
    if (threadIdx.x < NV) partials[threadIdx.x * gridDim.x + blockIdx.x] = rows_total(lds, threadIdx.x);
}

// one block: the blocks' partials in order (thread t holds block t's), then the stats the later launches read
template <bool WEIGHTED, int PASS>
__global__ __launch_bounds__(KDE_BLOCK) void kde_moments_finish_kernel(const double *__restrict__ partials, int n_blocks, double factor,
                                                                       double *__restrict__ stats)
{
    using L = KdeLayout<WEIGHTED>;
    constexpr int NV = (PASS == 1) ? L::ROWS : 1;
    __shared__ double lds[NV][4];
    double v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = (static_cast<int>(threadIdx.x) < n_blocks) ? partials[k * n_blocks + threadIdx.x] : 0.0;
    block_sum_rows<NV>(v, lds);
    if (threadIdx.x != 0) return;
    if constexpr (PASS == 1) {
        const double n_kept = rows_total(lds, 0);
        stats[L::N_KEPT] = n_kept;
        stats[L::N_NAN] = rows_total(lds, 1);
        stats[L::N_LOW] = rows_total(lds, 2);
        stats[L::N_HIGH] = rows_total(lds, 3);
        if constexpr (WEIGHTED) {
            const double sw = rows_total(lds, 5), sw2 = rows_total(lds, 6);
            stats[L::N_BAD_WEIGHT] = rows_total(lds, 4);
            stats[L::SUM_W] = sw;
            stats[L::SUM_W2] = sw2;
            stats[L::NEFF] = sw * (sw / sw2);                                 // sw^2 / sw2; at unit weights n (n / n), exact for any n
            stats[L::MEAN] = rows_total(lds, 7) / sw;
        } else {
            stats[L::MEAN] = rows_total(lds, 4) / n_kept;
        }
    } else {
        double neff, dof;                                                     // Scott's n and np.cov's ddof=1 divisor
        if constexpr (WEIGHTED) {
            const double sw = stats[L::SUM_W], sw2 = stats[L::SUM_W2];
            neff = stats[L::NEFF];
            dof = sw - sw2 / sw;                                              // np.cov(aweights=w, ddof=1)
        } else {
            neff = stats[L::N_KEPT];
            dof = neff - 1.0;
        }
        const double var = rows_total(lds, 0) / dof;
        const double f = (factor > 0.0) ? factor : pow(neff, -0.2);           // Scott's rule in one dimension
        stats[L::VAR] = var;
        stats[L::H] = sqrt(var) * f;
        stats[L::FACTOR] = f;
    }
}

template <bool WEIGHTED>
__global__ __launch_bounds__(KDE_BLOCK) void kde_gaussian_kernel(const double *__restrict__ a, KdeWeight wt, size_t n, size_t chunk_len,
                                                                 double divisor, double limit, const double *__restrict__ points,
                                                                 int m, const double *__restrict__ stats,
                                                                 double *__restrict__ partials)
{
    __shared__ double lds[KDE_TILE][4];
    const int j0 = blockIdx.x * KDE_TILE;
    double g[KDE_TILE], acc[KDE_TILE];
#pragma unroll
    for (int j = 0; j < KDE_TILE; ++j) {
        g[j] = points[(j0 + j < m) ? j0 + j : m - 1];                 // the last tile repeats the last point: read in bounds, not stored
        acc[j] = 0.0;
    }
    const double inv_h = 1.0 / stats[KdeLayout<WEIGHTED>::H];
    const size_t begin = static_cast<size_t>(blockIdx.y) * chunk_len;
    const size_t end = (begin + chunk_len < n) ? begin + chunk_len : n;
    for (size_t p = begin + threadIdx.x; p < end; p += KDE_BLOCK) {
        const double v = a[p] / divisor;
        const double w = kde_weight<WEIGHTED>(wt, p);
        const bool kept = (v == v) && !(v > limit) && !(v < -limit) && kde_weight_kept<WEIGHTED>(w);
#pragma unroll
        for (int j = 0; j < KDE_TILE; ++j) {
            const double d = (g[j] - v) * inv_h;
            const double e = exp_full((-0.5 * d) * d);                // <= 0: +0 below -746
            acc[j] += kept ? kde_times_weight<WEIGHTED>(w, e) : 0.0;
        }
    }
    block_sum_rows<KDE_TILE>(acc, lds);
    if (threadIdx.x < KDE_TILE && j0 + static_cast<int>(threadIdx.x) < m)
        partials[static_cast<size_t>(blockIdx.y) * m + j0 + threadIdx.x] = rows_total(lds, threadIdx.x);
}

template <bool WEIGHTED>
__global__ __launch_bounds__(KDE_BLOCK) void kde_finish_kernel(const double *__restrict__ partials, int n_chunks, int m,
                                                               const double *__restrict__ stats, double *__restrict__ density)
{
    using L = KdeLayout<WEIGHTED>;
    const int j = blockIdx.x * KDE_BLOCK + threadIdx.x;
    if (j >= m) return;
    double s = 0.0;
#pragma unroll 16
    for (int c = 0; c < n_chunks; ++c) s += partials[static_cast<size_t>(c) * m + j];
    density[j] = s / (stats[L::NORM] * stats[L::H] * 2.5066282746310002);                      // sqrt(2 pi)
}

// host side of both entry points: `fn` names the entry in every message, `ws_fn` its workspace function
template <bool WEIGHTED>
int kde_workspace_bytes(const char *fn, size_t n, size_t *bytes, size_t *chunk_length)
{
    SVMC_REQUIRE(bytes, std::string(fn) + ": null pointer");
    SVMC_REQUIRE(n >= 1 && n < (static_cast<size_t>(1) << 40), std::string(fn) + ": n must be in 1 .. 2^40 - 1");
    const size_t len = kde_chunk_length(n), n_chunks = (n + len - 1) / len;
    *bytes = sizeof(double) * (KdeLayout<WEIGHTED>::ROWS * KDE_MOMENT_BLOCKS + n_chunks * SVMC_KDE_MAX_POINTS);
    if (chunk_length) *chunk_length = len;
    return SVMC_OK;
}

template <bool WEIGHTED>
int kde_launch(const char *fn, const char *ws_fn, const double *values, KdeWeight wt, size_t n, double divisor, double limit,
               const double *points, int n_points, double bandwidth_factor, double *density, double *stats, void *workspace,
               size_t workspace_bytes, svmc_stream_t stream)
{
    constexpr size_t MOMENT_DOUBLES = KdeLayout<WEIGHTED>::ROWS * KDE_MOMENT_BLOCKS;
    SVMC_REQUIRE(values && points && density && stats && workspace, std::string(fn) + ": null pointer");
    SVMC_REQUIRE(n >= 1 && n < (static_cast<size_t>(1) << 40), std::string(fn) + ": n must be in 1 .. 2^40 - 1");
    SVMC_REQUIRE(n_points >= 1, std::string(fn) + ": n_points must be at least 1");
    SVMC_REQUIRE(n_points <= SVMC_KDE_MAX_POINTS, std::string(fn) + ": n_points above SVMC_KDE_MAX_POINTS");
    SVMC_REQUIRE(divisor > 0.0 && divisor < HUGE_VAL, std::string(fn) + ": divisor must be positive and finite");
    SVMC_REQUIRE(limit > 0.0 && limit < HUGE_VAL, std::string(fn) + ": limit must be positive and finite");
    SVMC_REQUIRE(bandwidth_factor == bandwidth_factor && bandwidth_factor < HUGE_VAL, std::string(fn) + ": bandwidth factor must be finite");
    if constexpr (WEIGHTED) SVMC_REQUIRE(wt.gamma > -HUGE_VAL && wt.gamma < HUGE_VAL, std::string(fn) + ": gamma must be finite");
    const size_t len = kde_chunk_length(n), n_chunks = (n + len - 1) / len;
    if (workspace_bytes < sizeof(double) * (MOMENT_DOUBLES + n_chunks * static_cast<size_t>(n_points)))
        return fail(SVMC_ERR_WORKSPACE, std::string(fn) + ": workspace too small (" + ws_fn + ")");
    double *moment_partials = static_cast<double *>(workspace), *partials = moment_partials + MOMENT_DOUBLES;
    const unsigned mb = kde_moment_blocks(n);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL((kde_moments_kernel<WEIGHTED, 1>), dim3(mb), dim3(KDE_BLOCK), 0, s, values, wt, n, divisor, limit, stats,
                       moment_partials);
    hipLaunchKernelGGL((kde_moments_finish_kernel<WEIGHTED, 1>), dim3(1), dim3(KDE_BLOCK), 0, s, moment_partials, static_cast<int>(mb),
                       bandwidth_factor, stats);
    hipLaunchKernelGGL((kde_moments_kernel<WEIGHTED, 2>), dim3(mb), dim3(KDE_BLOCK), 0, s, values, wt, n, divisor, limit, stats,
                       moment_partials);
    hipLaunchKernelGGL((kde_moments_finish_kernel<WEIGHTED, 2>), dim3(1), dim3(KDE_BLOCK), 0, s, moment_partials, static_cast<int>(mb),
                       bandwidth_factor, stats);
    hipLaunchKernelGGL(kde_gaussian_kernel<WEIGHTED>, dim3((n_points + KDE_TILE - 1) / KDE_TILE, static_cast<unsigned>(n_chunks)),
                       dim3(KDE_BLOCK), 0, s, values, wt, n, len, divisor, limit, points, n_points, stats, partials);
    hipLaunchKernelGGL(kde_finish_kernel<WEIGHTED>, dim3((n_points + KDE_BLOCK - 1) / KDE_BLOCK), dim3(KDE_BLOCK), 0, s, partials,
                       static_cast<int>(n_chunks), n_points, stats, density);
    return check_launch(fn);
}


}  // namespace svmc

using namespace svmc;

extern "C" {

int svmc_mgf_pdf_slice_batch(const double *var_grid, const double *log_mgf, size_t n_grid, int n_sets, const double *space,
                             size_t n_space, const double *shifts_host, const double *scales_host, int is_simpson, double *pdf,
                             svmc_stream_t stream)
{
    SVMC_REQUIRE(var_grid && log_mgf && pdf, "svmc_mgf_pdf_slice_batch: null pointer");
    SVMC_REQUIRE(n_grid >= 3 && n_grid < (1u << 30), "svmc_mgf_pdf_slice_batch: grid too short or too long");
    SVMC_REQUIRE(n_sets >= 1 && n_sets <= 65535, "svmc_mgf_pdf_slice_batch: n_sets out of range");
    SVMC_REQUIRE(n_space == 0 || (space && shifts_host && scales_host), "svmc_mgf_pdf_slice_batch: null space grid, shifts or scales");
    SVMC_REQUIRE(n_space == 0 || (n_space >= 2 && n_space < (1u << 30)), "svmc_mgf_pdf_slice_batch: a space grid needs two points (dx)");
    if (n_space == 0) return SVMC_OK;
    for (int s = 0; s < n_sets; ++s)
        SVMC_REQUIRE(scales_host[s] != 0.0 && scales_host[s] == scales_host[s], "svmc_mgf_pdf_slice_batch: scale must be non-zero");
    for (int s0 = 0; s0 < n_sets; s0 += MAX_PDF_SETS) {
        const int m = (n_sets - s0 < MAX_PDF_SETS) ? (n_sets - s0) : MAX_PDF_SETS;
        PdfSets ps;
        for (int i = 0; i < MAX_PDF_SETS; ++i) {
            ps.shift[i] = (i < m) ? shifts_host[s0 + i] : 0.0;
            ps.scale[i] = (i < m) ? scales_host[s0 + i] : 1.0;
        }
        const size_t goff = static_cast<size_t>(s0) * n_grid, soff = static_cast<size_t>(s0) * n_space;
        hipLaunchKernelGGL(mgf_pdf_slice_kernel, dim3(static_cast<unsigned>(n_space), static_cast<unsigned>(m)),
                           dim3(MGF_SLICE_BLOCK), 0, as_stream(stream), reinterpret_cast<const cd *>(var_grid) + goff,
                           reinterpret_cast<const cd *>(log_mgf) + goff, static_cast<int>(n_grid), space + soff,
                           static_cast<int>(n_space), ps, is_simpson ? 1 : 0, pdf + soff);
    }
    return check_launch("svmc_mgf_pdf_slice_batch");
}

int svmc_mgf_digital_slice_batch(const double *phi, const double *log_mgf, size_t n_grid, int n_sets, double forward,
                                 const double *strikes_host, size_t n_strikes, int negative_contour, int is_simpson,
                                 double *sums, svmc_stream_t stream)
{
    SVMC_REQUIRE(phi && log_mgf && sums, "svmc_mgf_digital_slice_batch: null pointer");
    SVMC_REQUIRE(n_grid >= 3 && n_grid < (1u << 30), "svmc_mgf_digital_slice_batch: grid too short or too long");
    SVMC_REQUIRE(n_strikes == 0 || strikes_host, "svmc_mgf_digital_slice_batch: null strikes");
    SVMC_REQUIRE(n_strikes < (1u << 30), "svmc_mgf_digital_slice_batch: too many strikes");
    SVMC_REQUIRE(n_sets >= 1 && n_sets <= 65535, "svmc_mgf_digital_slice_batch: n_sets out of range");
    SVMC_REQUIRE(forward > 0.0 && forward < HUGE_VAL, "svmc_mgf_digital_slice_batch: forward must be positive and finite");
    for (size_t k = 0; k < n_strikes; ++k)           // log(forward / strike) of any other strike is NaN or inf: every term dropped, a silent 0
        SVMC_REQUIRE(strikes_host[k] > 0.0 && strikes_host[k] < HUGE_VAL,
                     "svmc_mgf_digital_slice_batch: strikes must be positive and finite");
    for (size_t k0 = 0; k0 < n_strikes; k0 += MGF_SLICE_STRIKES) {
        SliceStrikes da;
        const int k_here = fill_strike_chunk(da.x, strikes_host, k0, n_strikes,
                                             [&](double strike) { return log(forward / strike); });           // :249
        hipLaunchKernelGGL(mgf_digital_slice_kernel, dim3(k_here, static_cast<unsigned>(n_sets)), dim3(MGF_SLICE_BLOCK), 0,
                           as_stream(stream), reinterpret_cast<const cd *>(phi), reinterpret_cast<const cd *>(log_mgf),
                           static_cast<int>(n_grid), da, negative_contour ? 1 : 0, is_simpson ? 1 : 0, sums + k0,
                           static_cast<int>(n_strikes));
    }
    return check_launch("svmc_mgf_digital_slice_batch");
}

int svmc_mgf_il_slice_batch(const double *phi, const double *log_mgf, size_t n_grid, int n_sets, const double *x_host,
                            const double *xa_host, const double *xb_host, size_t n_cases, int is_simpson, double *sums,
                            svmc_stream_t stream)
{
    SVMC_REQUIRE(phi && log_mgf && sums, "svmc_mgf_il_slice_batch: null pointer");
    SVMC_REQUIRE(n_grid >= 3 && n_grid < (1u << 30), "svmc_mgf_il_slice_batch: grid too short or too long");
    SVMC_REQUIRE(n_cases == 0 || (x_host && xa_host && xb_host), "svmc_mgf_il_slice_batch: null cases");
    SVMC_REQUIRE(n_cases < (1u << 28), "svmc_mgf_il_slice_batch: too many cases");
    SVMC_REQUIRE(n_sets >= 1 && n_sets <= 65535, "svmc_mgf_il_slice_batch: n_sets out of range");
    for (size_t k = 0; k < n_cases; ++k)             // the logarithm of any price that is not positive and finite: every term dropped, a silent 0
        SVMC_REQUIRE(std::isfinite(x_host[k]) && std::isfinite(xa_host[k]) && std::isfinite(xb_host[k]) && xa_host[k] < xb_host[k],
                     "svmc_mgf_il_slice_batch: log p1, log pa < log pb must be finite");
    for (size_t k0 = 0; k0 < n_cases; k0 += MGF_SLICE_STRIKES) {
        IlSliceCases ca;
        const auto same = [](double v) { return v; };
        const int k_here = fill_strike_chunk(ca.x, x_host, k0, n_cases, same);
        fill_strike_chunk(ca.xa, xa_host, k0, n_cases, same);
        fill_strike_chunk(ca.xb, xb_host, k0, n_cases, same);
        hipLaunchKernelGGL(mgf_il_slice_kernel, dim3(k_here, static_cast<unsigned>(n_sets)), dim3(MGF_SLICE_BLOCK), 0,
                           as_stream(stream), reinterpret_cast<const cd *>(phi), reinterpret_cast<const cd *>(log_mgf),
                           static_cast<int>(n_grid), ca, is_simpson ? 1 : 0, sums + IL_SLICE_SUMS * k0,
                           static_cast<int>(IL_SLICE_SUMS * n_cases));
    }
    return check_launch("svmc_mgf_il_slice_batch");
}

int svmc_histogram_uniform(const double *values, size_t n, double divisor, const double *edges, int n_bins, uint64_t *counts,
                           svmc_stream_t stream)
{
    SVMC_REQUIRE(edges && counts, "svmc_histogram_uniform: null pointer");
    SVMC_REQUIRE(n == 0 || values, "svmc_histogram_uniform: null values");
    SVMC_REQUIRE(n_bins >= 1 && n_bins <= HIST_MAX_BINS, "svmc_histogram_uniform: n_bins must be in 1 .. 8192");
    SVMC_REQUIRE(divisor != 0.0 && divisor == divisor, "svmc_histogram_uniform: divisor must be non-zero");
    SVMC_HIP_TRY(hipMemsetAsync(counts, 0, sizeof(uint64_t) * static_cast<size_t>(n_bins), as_stream(stream)));
    if (n == 0) return SVMC_OK;
    const size_t want = (n + HIST_BLOCK - 1) / HIST_BLOCK;
    const unsigned blocks = static_cast<unsigned>(want < HIST_MAX_BLOCKS ? want : HIST_MAX_BLOCKS);
    hipLaunchKernelGGL(histogram_uniform_kernel, dim3(blocks), dim3(HIST_BLOCK), sizeof(unsigned int) * static_cast<size_t>(n_bins),
                       as_stream(stream), values, n, divisor, edges, n_bins, reinterpret_cast<unsigned long long *>(counts));
    return check_launch("svmc_histogram_uniform");
}

int svmc_kde_workspace_bytes(size_t n, size_t *bytes, size_t *chunk_length)
{
    return kde_workspace_bytes<false>("svmc_kde_workspace_bytes", n, bytes, chunk_length);
}

int svmc_kde_gaussian(const double *values, size_t n, double divisor, double limit, const double *points, int n_points,
                      double bandwidth_factor, double *density, double *stats, void *workspace, size_t workspace_bytes,
                      svmc_stream_t stream)
{
    return kde_launch<false>("svmc_kde_gaussian", "svmc_kde_workspace_bytes", values, KdeWeight{nullptr, nullptr, 0.0}, n, divisor, limit,
                             points, n_points, bandwidth_factor, density, stats, workspace, workspace_bytes, stream);
}

int svmc_kde_weighted_workspace_bytes(size_t n, size_t *bytes, size_t *chunk_length)
{
    return kde_workspace_bytes<true>("svmc_kde_weighted_workspace_bytes", n, bytes, chunk_length);
}

int svmc_kde_gaussian_weighted(const double *values, const double *weights, const double *tilt, double gamma, size_t n,
                               double divisor, double limit, const double *points, int n_points, double bandwidth_factor,
                               double *density, double *stats, void *workspace, size_t workspace_bytes, svmc_stream_t stream)
{
    return kde_launch<true>("svmc_kde_gaussian_weighted", "svmc_kde_weighted_workspace_bytes", values, KdeWeight{weights, tilt, gamma}, n,
                            divisor, limit, points, n_points, bandwidth_factor, density, stats, workspace, workspace_bytes, stream);
}

}  // extern "C"
