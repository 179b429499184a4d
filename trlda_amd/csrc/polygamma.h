// polygamma.h -- psi^(n)(x) for host code and a gfx950 kernel (reference src/utils.cpp:107-123:
// polygamma(n, x) = digamma(x) for n < 1, (-1)^(n+1) n! zeta(n+1, x) for n >= 1).
//
// Every function is __host__ __device__ and built from +, -, *, /, floor, ceil and frexp only, with
// no product or sum contracted into an FMA: the host scalar (trlda_polygamma) and a device element
// (polygamma_kernel) run the same operations in the same order and agree to the last bit, for every
// n.  (psi.h's device digamma is not used: its log is the device library's, so it could not be
// bitwise equal to a host value.)
//
// zeta(s, x) = sum_{i >= 0} (x + i)^-s, integer s >= 2:
//   x a non-positive integer (-inf included): +inf; x = +inf: 0; nan: nan
//   x < kPolygammaMinX (a fractional part): nan -- the direct sum below would take 2^20+ terms (the
//       reference's zeta sums them one by one)
//   w = sum_{i < N} (x + i)^-s, added from i = 0 up, N the least with a = x + N >= A(s),
//       A(s) = 16 + min(s, 1024); a negative non-integer x takes the same sum (the Hurwitz series)
//   zeta = w + [ a^(1-s) / (s-1) + ( a^-s / 2 + sum_{k=10..1} B_2k / (2k)! (s)_(2k-1) a^(-s-2k+1) ) ]
//       (Euler-Maclaurin; (s)_j the rising factorial; the ten terms added from the smallest up).
//       From a >= A(s) the first omitted term is below 2^-56 of the sum.
//   Integer powers are products: r^e by binary exponentiation of r = 1/a (or 1/(x + i)).
//
// psi(x):
//   x a non-positive integer (-inf included): +inf; nan: nan
//   x < kPolygammaMinX (a fractional part): reflection, psi(x) = psi(1 - x) - pi cot(pi x), with
//       f = x - floor(x) (exact) moved into (-1/2, 1/2] and pi cot(pi f) = pi cos(t) / sin(t), t = pi f,
//       from the Taylor series through t^23 / t^24 (f = 1/2: 0)
//   w = sum_{i < N} 1/(x + i) (from i = 0 up), N the least with s = x + N >= 10
//   psi = ((log s - 1/(2s)) - sum_{k=1..7} B_2k / (2k s^2k)) - w
//   log s: frexp, the mantissa folded into [sqrt(1/2), sqrt(2)), 2 atanh(u), u = (m-1)/(m+1), as the
//   odd series through u^21, and the exponent times ln 2 in two parts.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace trlda {

constexpr double kPolygammaMinX = -1048576.0;          // -2^20
constexpr int kPolygammaThreads = 256;

// r^e, e >= 1, by binary exponentiation
__host__ __device__ inline double pg_ipow(double r, unsigned e)
{
#pragma clang fp contract(off)
    double acc = 1.0, p = r;
    bool first = true;
    while (e) {
        if (e & 1u) {
            acc = first ? p : acc * p;
            first = false;
        }
        e >>= 1;
        if (e)
            p = p * p;
    }
    return acc;
}

// log(s) for s >= 1 (normal) or +inf
__host__ __device__ inline double pg_log(double s)
{
#pragma clang fp contract(off)
    if (!(s < INFINITY))
        return s;
    int e = 0;
    double m = frexp(s, &e);                              // m in [1/2, 1)
    if (m < 0.70710678118654752440) {
        m = m + m;
        e = e - 1;
    }
    const double f = m - 1.0;
    const double u = f / (2.0 + f);
    const double z = u * u;
    double p = 2.0 / 21.0;
    p = p * z + 2.0 / 19.0;
    p = p * z + 2.0 / 17.0;
    p = p * z + 2.0 / 15.0;
    p = p * z + 2.0 / 13.0;
    p = p * z + 2.0 / 11.0;
    p = p * z + 2.0 / 9.0;
    p = p * z + 2.0 / 7.0;
    p = p * z + 2.0 / 5.0;
    p = p * z + 2.0 / 3.0;
    p = p * z + 2.0;
    const double ed = (double)e;
    // ln 2 = 6.93147180369123816490e-01 (its low 28 bits zero: ed * hi is exact) + 1.90821492927058770002e-10
    return ed * 6.93147180369123816490e-01 + (ed * 1.90821492927058770002e-10 + u * p);
}

// pi cot(pi f) for f in (-1/2, 1/2], f != 0
__host__ __device__ inline double pg_pi_cot(double f)
{
#pragma clang fp contract(off)
    if (f == 0.5)
        return 0.0;
    const double pi = 3.141592653589793238462643383279502884;
    const double t = pi * f, t2 = t * t;
    double sp = -1.0 / 25852016738884976640000.0;        // -1/23!
    sp = sp * t2 + 1.0 / 51090942171709440000.0;         // 1/21!
    sp = sp * t2 - 1.0 / 121645100408832000.0;           // 1/19!
    sp = sp * t2 + 1.0 / 355687428096000.0;
    sp = sp * t2 - 1.0 / 1307674368000.0;
    sp = sp * t2 + 1.0 / 6227020800.0;
    sp = sp * t2 - 1.0 / 39916800.0;
    sp = sp * t2 + 1.0 / 362880.0;
    sp = sp * t2 - 1.0 / 5040.0;
    sp = sp * t2 + 1.0 / 120.0;
    sp = sp * t2 - 1.0 / 6.0;
    sp = sp * t2 + 1.0;
    double cp = 1.0 / 620448401733239439360000.0;        // 1/24!
    cp = cp * t2 - 1.0 / 1124000727777607680000.0;       // 1/22!
    cp = cp * t2 + 1.0 / 2432902008176640000.0;
    cp = cp * t2 - 1.0 / 6402373705728000.0;
    cp = cp * t2 + 1.0 / 20922789888000.0;
    cp = cp * t2 - 1.0 / 87178291200.0;
    cp = cp * t2 + 1.0 / 479001600.0;
    cp = cp * t2 - 1.0 / 3628800.0;
    cp = cp * t2 + 1.0 / 40320.0;
    cp = cp * t2 - 1.0 / 720.0;
    cp = cp * t2 + 1.0 / 24.0;
    cp = cp * t2 - 1.0 / 2.0;
    cp = cp * t2 + 1.0;
    return pi * cp / (t * sp);
}

__host__ __device__ inline double pg_digamma(double x)
{
#pragma clang fp contract(off)
    if (x <= 0.0 && x == floor(x))
        return INFINITY;
    if (x != x)
        return x;
    double reflect = 0.0;
    if (x < kPolygammaMinX) {
        double f = x - floor(x);
        if (f > 0.5)
            f = f - 1.0;
        reflect = pg_pi_cot(f);
        x = 1.0 - x;
    }
    const int N = x < 10.0 ? (int)ceil(10.0 - x) : 0;
    double w = 0.0;
    for (int i = 0; i < N; ++i)
        w = w + 1.0 / (x + (double)i);
    const double s = x + (double)N;
    const double z = 1.0 / (s * s);
    // B_2k / (2k): 1/12, -1/120, 1/252, -1/240, 1/132, -691/32760, 1/12
    double p = 1.0 / 12.0;
    p = p * z + -691.0 / 32760.0;
    p = p * z + 1.0 / 132.0;
    p = p * z + -1.0 / 240.0;
    p = p * z + 1.0 / 252.0;
    p = p * z + -1.0 / 120.0;
    p = p * z + 1.0 / 12.0;
    return (((pg_log(s) - 0.5 / s) - z * p) - w) - reflect;
}

// zeta(s, x), integer s >= 2 (the header's recipe)
__host__ __device__ inline double pg_zeta(unsigned s, double x)
{
#pragma clang fp contract(off)
    if (x <= 0.0 && x == floor(x))
        return INFINITY;
    if (x != x)
        return x;
    if (x == INFINITY)
        return 0.0;
    if (x < kPolygammaMinX)
        return NAN;
    const double A = 16.0 + (double)(s < 1024u ? s : 1024u);
    const int N = x < A ? (int)ceil(A - x) : 0;
    double w = 0.0;
    for (int i = 0; i < N; ++i)
        w = w + pg_ipow(1.0 / (x + (double)i), s);
    const double a = x + (double)N;
    const double r = 1.0 / a, r2 = r * r;
    const double ds = (double)s;
    const double p = pg_ipow(r, s - 1u);                  // a^(1-s)
    const double t = p * r;                               // a^-s
    // B_2k / (2k)!, k = 1 .. 10
    const double c[10] = {8.333333333333333e-02,  -1.388888888888889e-03, 3.306878306878307e-05,
                          -8.267195767195768e-07, 2.08767569878681e-08,   -5.284190138687493e-10,
                          1.3382536530684679e-11, -3.3896802963225827e-13, 8.586062056277845e-15,
                          -2.174868698558062e-16};
    double f[10];
    f[0] = ds * t * r;                                    // (s)_1 a^(-s-1)
#pragma unroll
    for (int k = 1; k < 10; ++k)                          // (s)_(2k+1) a^(-s-2k-1)
        f[k] = f[k - 1] * ((ds + (double)(2 * k - 1)) * (ds + (double)(2 * k))) * r2;
    double tail = c[9] * f[9];
#pragma unroll
    for (int k = 8; k >= 0; --k)
        tail = tail + c[k] * f[k];
    return w + (p / (ds - 1.0) + (0.5 * t + tail));
}

__host__ __device__ inline double pg_polygamma(int n, double x)
{
#pragma clang fp contract(off)
    if (n < 1)
        return pg_digamma(x);
    double fact = 1.0;                                    // n! (inf from n = 171 on)
    for (int i = 2; i <= n && fact < INFINITY; ++i)
        fact = fact * (double)i;
    const double sign = (n & 1) ? 1.0 : -1.0;             // (-1)^(n+1)
    return sign * fact * pg_zeta((unsigned)n + 1u, x);
}

// y[i] = psi^(n)(x[i]), i < count; the grid strides
__global__ __launch_bounds__(kPolygammaThreads) void polygamma_kernel(int n, int64_t count,
                                                                      const double *__restrict__ x,
                                                                      double *__restrict__ y)
{
    const int64_t stride = (int64_t)gridDim.x * kPolygammaThreads;
    for (int64_t i = (int64_t)blockIdx.x * kPolygammaThreads + threadIdx.x; i < count; i += stride)
        y[i] = pg_polygamma(n, x[i]);
}

}  // namespace trlda
