// svmc_mgf_slice.h -- what the six transform-inversion slice kernels share (mgf_vanilla_slice_kernel, mgf_qvar_slice_kernel:
// svmc_analytic.hip; mgf_gamma_slice_kernel: svmc_hawkes.hip; mgf_pdf_slice_kernel, mgf_digital_slice_kernel,
// mgf_il_slice_kernel: svmc_density.hip).
// A block handles one strike (or space point) of one parameter set (blockIdx.y), MGF_SLICE_BLOCK threads stride the transform
// grid and NaN terms are dropped, as the reference's np.nansum does.  The order of the sum depends on the grid length alone --
// thread t adds j = t, t + 256, ... in order, the 64 lanes of a wave meet in one shuffle tree and the four waves are added in
// order -- so a set of a batch is bit-equal to the set alone.  A kernel keeps its prologue, its term and its store.
#pragma once
#include <hip/hip_runtime.h>

#include "svmc_complex.h"
#include "svmc_slice.h"

namespace svmc {

constexpr double PI = 3.14159265358979323846;
constexpr int MGF_SLICE_BLOCK = 256;         // threads per block of the six kernels
constexpr int MGF_SLICE_STRIKES = 32;        // strikes per launch (kernel-argument block)
static_assert(MGF_SLICE_BLOCK == 256, "block_sum adds four waves");

// w_j of the legacy pricer weights (utils/mgf_pricer.py:157-171), BEFORE the division by pi: Simpson 1,4,2,... with every odd
// index 4, or for is_simpson = 0 half the first step on the first point and the local step on the others
__device__ __forceinline__ double legacy_weight(const cd *__restrict__ u, int j, int n_grid, double h, int is_simpson)
{
    if (is_simpson) {
        double w = 2.0;
        if (j == 0 || j == n_grid - 1) w = 1.0;
        if (j & 1) w = 4.0;
        return (h / 3.0) * w;
    }
    return (j == 0) ? 0.5 * h : u[j].im - u[j - 1].im;
}

// (a + 0i) / b as NumPy divides (Smith's form: the larger component of b scales the other)
__device__ __forceinline__ cd real_over_complex(double a, cd b)
{
    if (fabs(b.re) >= fabs(b.im)) {
        const double rat = b.im / b.re, scl = 1.0 / (b.re + b.im * rat);
        return cd{a * scl, -(a * rat) * scl};
    }
    const double rat = b.re / b.im, scl = 1.0 / (b.im + b.re * rat);
    return cd{(a * rat) * scl, -a * scl};
}

// a / b of two complex numbers, the same form
__device__ __forceinline__ cd complex_over_complex(cd a, cd b)
{
    if (fabs(b.re) >= fabs(b.im)) {
        const double rat = b.im / b.re, scl = 1.0 / (b.re + b.im * rat);
        return cd{(a.re + a.im * rat) * scl, (a.im - a.re * rat) * scl};
    }
    const double rat = b.re / b.im, scl = 1.0 / (b.im + b.re * rat);
    return cd{(a.re * rat + a.im) * scl, (a.im * rat - a.re) * scl};
}

// the block's sum in its fixed order; thread 0 holds it
__device__ __forceinline__ double block_sum(double s, double *lds)
{
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// thread t adds term(j) for j = t, t + 256, ... in order, skipping NaN (inf is kept); then block_sum: thread 0 holds the total
template <class Term>
__device__ __forceinline__ double mgf_slice_nansum(int n_grid, double *lds, Term &&term)
{
    double s = 0.0;
    for (int j = threadIdx.x; j < n_grid; j += MGF_SLICE_BLOCK) {
        const double t = term(j);
        if (t == t) s += t;
    }
    return block_sum(s, lds);
}

struct SliceStrikes {
    double x[MGF_SLICE_STRIKES];             // log(forward / strike); strike * ttm for the quadratic variance
};

// x[k] = value(strike) of the chunk's live strikes k0 .. k0 + live - 1, 0.0 beyond; -> live
template <class Value>
inline int fill_strike_chunk(double (&x)[MGF_SLICE_STRIKES], const double *strikes_host, size_t k0, size_t n_strikes, Value &&value)
{
    const int live = static_cast<int>((n_strikes - k0 < MGF_SLICE_STRIKES) ? (n_strikes - k0) : MGF_SLICE_STRIKES);
    for (int k = 0; k < MGF_SLICE_STRIKES; ++k) x[k] = (k < live) ? value(strikes_host[k0 + k]) : 0.0;
    return live;
}

}  // namespace svmc
