// philox.h -- the library's counter-based random stream, shared by host code and kernels: Philox4x32-10
// (Salmon et al., SC'11; Random123's constants), the two uniform mappings and the Marsaglia-Tsang
// log-gamma recipe.  Every function is __host__ __device__, so the host (trlda_sample_lengths) and
// the kernels (gibbs_kernels.h, sample_kernels.h, dirichlet_kernels.h, marginal_kernels.h, l2r_kernels.h)
// run the same code.
//
// A draw is one Philox block of the counter (c0, c1, c2, c3) under the call's 64-bit key (k0, k1),
// c3 being the draw's purpose.  The purposes in use, and what the other three words hold:
//
//   purpose  draw                                          counter (c0, c1, c2)
//   0        Gibbs: Dirichlet(1) initial theta              (topic k, document d, 0)
//   1        Gibbs: initial topic of a token                (token t of d, d, 0)
//   2        Gibbs: topic of a token in a sweep             (token t of d, d, sweep s)
//   3 / 4 / 5 Gibbs theta gamma: normal / accept / boost    (topic k, document d, attempt; boost 0)
//   8 / 9 / 10 sample: beta gamma: normal / accept / boost  (word w, topic k, attempt; boost 0)
//   11 / 12 / 13 sample: theta gamma: normal / accept / boost (topic k, document d, attempt; boost 0)
//   14       sample: document length                       (document d, 0, 0)
//   15       sample: token; x0,x1 the topic uniform,       (token t within d, d, 0)
//            x2,x3 the word uniform
//   16 / 17 / 18 sample_dirichlet: normal / accept / boost  (row i, column j, attempt; boost 0)
//   19 / 20 / 21 document likelihood: theta gamma:          (sample s * K + topic k, document d,
//            normal / accept / boost                         attempt; boost 0)
//   22       left-to-right: a prefix token's redraw         (token t of d, position n, d * R + particle r)
//   23       left-to-right: a new token's draw              (position n, n, d * R + particle r)
//
// The output words (x0, x1, x2, x3) become uniforms through x = x1 * 2^32 + x0 (and x3 * 2^32 + x2):
//     u      = (x >> 11) * 2^-53           in [0, 1)    histogram draws
//     u_open = ((x >> 12) + 0.5) * 2^-52   in (0, 1)    every draw that takes a logarithm
//
// log of a Gamma(a) draw (Marsaglia & Tsang 2000), philox_log_gamma: a <= 0 or not finite gives
// -inf.  For a < 1 the shape a + 1 and then log G += log(u_open of the boost purpose) / a.
// d = a' - 1/3, c = 1/sqrt(9d); attempt n = 0, 1, ..: x = sqrt(-2 log u_open) cos(2 pi u) from the
// normal purpose's two uniforms, v = (1 + c x)^3 (rejected if 1 + c x <= 0), accepted when
// log(u_open of the accept purpose) < x^2/2 + d - d v + d log v; log G = log d + log v.  After
// kGammaTries attempts (acceptance is above 0.95 per attempt) log d is taken.  No product or sum
// is contracted into an FMA.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace trlda {

constexpr int kGammaTries = 64;

// Philox4x32-10 in place on the counter
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = (uint32_t)p1;
        c[2] = n2;
        c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

__host__ __device__ __forceinline__ void philox_block(uint32_t (&c)[4], uint32_t c0, uint32_t c1, uint32_t c2,
                                                      uint32_t purpose, uint32_t k0, uint32_t k1)
{
    c[0] = c0; c[1] = c1; c[2] = c2; c[3] = purpose;
    philox4x32_10(c, k0, k1);
}

__host__ __device__ __forceinline__ double philox_u(uint32_t lo, uint32_t hi)
{
    const uint64_t x = ((uint64_t)hi << 32) | lo;
    return (double)(x >> 11) * 0x1.0p-53;
}

__host__ __device__ __forceinline__ double philox_u_open(uint32_t lo, uint32_t hi)
{
    const uint64_t x = ((uint64_t)hi << 32) | lo;
    return ((double)(x >> 12) + 0.5) * 0x1.0p-52;
}

// log of a Gamma(a) draw (the header's recipe) of counter words (c0, c1) and the three purposes
__host__ __device__ inline double philox_log_gamma(double a, uint32_t c0, uint32_t c1, uint32_t p_normal,
                                                   uint32_t p_accept, uint32_t p_boost, uint32_t k0, uint32_t k1)
{
#pragma clang fp contract(off)
    if (!(a > 0.0) || !(a <= 1.0e300))
        return -INFINITY;
    const bool boost = a < 1.0;
    const double sh = boost ? a + 1.0 : a;
    const double d = sh - 1.0 / 3.0;
    const double c = 1.0 / sqrt(9.0 * d);
    double lg = log(d);
    for (int n = 0; n < kGammaTries; ++n) {
        uint32_t w[4];
        philox_block(w, c0, c1, (uint32_t)n, p_normal, k0, k1);
        const double x = sqrt(-2.0 * log(philox_u_open(w[0], w[1]))) * cos(6.283185307179586 * philox_u(w[2], w[3]));
        const double v1 = 1.0 + c * x;
        if (v1 <= 0.0)
            continue;
        const double v = v1 * v1 * v1;
        philox_block(w, c0, c1, (uint32_t)n, p_accept, k0, k1);
        const double lu = log(philox_u_open(w[0], w[1]));
        const double lv = log(v);
        if (lu < 0.5 * x * x + d - d * v + d * lv) {
            lg = log(d) + lv;
            break;
        }
    }
    if (boost) {
        uint32_t w[4];
        philox_block(w, c0, c1, 0u, p_boost, k0, k1);
        lg = lg + log(philox_u_open(w[0], w[1])) / a;
    }
    return lg;
}

}  // namespace trlda
