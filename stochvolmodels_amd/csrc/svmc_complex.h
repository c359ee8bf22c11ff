// svmc_complex.h -- the complex double of the transform grids (svmc_analytic.hip, svmc_hawkes.hip) and its helpers.
//
// The ring operations are host-compilable (svmc_ode.h builds on them, tests/native/ode_probe.cpp compiles that with g++).
// The elementary functions below them are device-only: they call the device libm's hypot, exp, sincos, log and atan2.
// Accuracy of the device build (tests/test_gpu_device_math.py against mpmath, componentwise, relative to |result|):
//   cabs_      <= 2.5e-16 (measured 2.2e-16)
//   operator/  <= 6e-16 (measured 3.5e-16), asserted for |b| in [1e-100, 1e100]: the naive |b|^2 form overflows to inf / NaN
//              above about 1e154 and underflows to 0 / NaN below about 1e-154.  The kernels' denominators (Heston's 2 zeta
//              and volvol^2 den, Hawkes's 1 + mean z) lie far inside that range.
//   cexp_      <= 5e-16 (measured 2.2e-16) for |Im z| <= 1e5 (the argument reduction of sincos)
//   csqrt_     <= 5e-16 (measured 2.2e-16), principal branch; on the negative real axis the sign of Im z picks the side,
//              as NumPy's sqrt
//   clog_      <= 5e-16 of max(|result|, 1) (measured 2.2e-16: near |z| = 1 the real part's error is absolute), principal
//              branch; atan2 gives +pi / -pi for Im z = +0 / -0, as NumPy's log
#pragma once
#include "svmc_math.h"

namespace svmc {

struct cd {
    double re, im;
};
SVMC_HD cd C(double re, double im = 0.0) { return cd{re, im}; }
SVMC_HD cd operator+(cd a, cd b) { return cd{a.re + b.re, a.im + b.im}; }
SVMC_HD cd operator-(cd a, cd b) { return cd{a.re - b.re, a.im - b.im}; }
SVMC_HD cd operator-(cd a) { return cd{-a.re, -a.im}; }
SVMC_HD cd operator*(cd a, cd b) { return cd{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
SVMC_HD cd operator*(double s, cd a) { return cd{s * a.re, s * a.im}; }
SVMC_HD cd operator+(cd a, double s) { return cd{a.re + s, a.im}; }
SVMC_HD cd operator+(double s, cd a) { return cd{a.re + s, a.im}; }
SVMC_HD cd operator-(cd a, double s) { return cd{a.re - s, a.im}; }
SVMC_HD cd operator-(double s, cd a) { return cd{s - a.re, -a.im}; }

#if defined(__HIPCC__)
__device__ __forceinline__ double cabs_(cd a) { return hypot(a.re, a.im); }
__device__ __forceinline__ cd operator/(cd a, cd b)
{
    const double d = b.re * b.re + b.im * b.im;
    return cd{(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}
__device__ __forceinline__ cd cexp_(cd z)
{
    double s, c;
    sincos(z.im, &s, &c);
    const double e = exp(z.re);
    return cd{e * c, e * s};
}
__device__ __forceinline__ cd csqrt_(cd z)   // principal branch
{
    const double r = cabs_(z);
    if (r == 0.0) return cd{0.0, 0.0};
    const double t = sqrt(0.5 * (r + fabs(z.re)));
    if (z.re >= 0.0) return cd{t, z.im / (2.0 * t)};
    return cd{fabs(z.im) / (2.0 * t), copysign(t, z.im)};
}
__device__ __forceinline__ cd clog_(cd z) { return cd{log(cabs_(z)), atan2(z.im, z.re)}; }
#endif

}  // namespace svmc
