// sample_kernels.h -- HIP kernels for gfx950 (MI355X) implementing LDA::sample (reference
// src/lda.cpp:88-115): documents drawn from the model.  Host side: trlda_hip.hip, sample_device.
//
// Semantics (the reference's, with the deviations DESIGN.md section 3.11 lists): topics
// beta_k ~ Dirichlet(lambda_k) are drawn once per call; per document d, theta_d ~ Dirichlet(alpha)
// and, for each of its n_d tokens (n_d ~ Poisson(length), drawn on the host: trlda_sample_lengths),
// a topic z ~ theta_d and then a word w ~ beta_z.  The random stream is philox.h's (purposes 8 to
// 15), so nothing of a draw depends on the launch geometry, the CU count or B.
//
// Launch sequence of one call:
//   1. sample_topics_kernel         K x V log-gamma draws of lambda_kw into the table, per chunk the max
//   2. sample_topics_scan_kernel    W_kw = exp(lg_kw - max_k), the prefix within each chunk
//   3. sample_topics_offset_kernel  the chunks' offsets added: C_kw, the inclusive prefix of row k
//   4. sample_theta_kernel          per document theta_d and its prefix P_d (K x B scratch)
//   5. sample_tokens_kernel         one thread per token: its topic, then its word
//
// ---- the beta table: C, K x V doubles, TOPIC-MAJOR (row k contiguous) --------------------------
// Row k is cut into chunks of kSampleChunk = 4096 words, a chunk into 4 waves x 64 lanes x 16 words;
// lane l of wave v holds the 16 consecutive words chunk * 4096 + (v * 64 + l) * 16 + j, j = 0 .. 15
// (words >= V weigh 0).  The summation order is a function of (K, V) only:
//   W   = exp(lg - max_k), lg = log Gamma(lambda_kw) (-inf for lambda_kw = 0 or not finite: W = 0)
//   q_j = q_{j-1} + W_j, q_0 = W_0                  (the lane's 16 words, in order)
//   L1  = e_l + q_j,  e_0 = 0, e_{l+1} = e_l + q_15 of lane l       (the lanes of a wave, in order)
//   L2  = g_v + L1,   g_0 = 0, g_{v+1} = g_v + L1 of wave v's last word  (the 4 waves, in order)
//   C   = o_c + L2,   o_0 = 0, o_{c+1} = o_c + L2 of chunk c's last word (the chunks, in order)
// Each level adds the running offset to a prefix that rises, and the next offset is that sum at
// the level's last word, so C never falls.  A row whose total C_{k,V-1} is not > 0 or not finite
// sets `flag`: the call fails with "Something went wrong while sampling from histogram."
// (utils.cpp:198).
//
// ---- theta and its prefix: one wave per document --------------------------------------------
// KPL = ceil(K / 64); lane l holds topics l * KPL .. l * KPL + KPL - 1 (topics >= K weigh 0).
//   lg_k = log Gamma(alpha_k) (purposes 11 / 12 / 13, counter (k, d, attempt)), mx = max over k
//   W_k  = exp(lg_k - mx); S = the lane-blocked sum below of W; theta_k = W_k / S
//   P_k  = E_l + p_j,  p_j = p_{j-1} + theta_k over the lane's topics in order, E_0 = 0,
//          E_{l+1} = E_l + p_{KPL-1} of lane l  (S: the same two levels over W, at k = K - 1)
// P (K x B, column d contiguous) stays in a scratch buffer; theta (K x B, F-order) is written
// when asked for.  S not > 0 or not finite sets `flag`.
//
// ---- a token ------------------------------------------------------------------------------
// Token t of the flat range [0, nnz): d = the last document with indptr[d] <= t, j = t - indptr[d];
// the Philox block of (j, d, 0, 15) gives u1 from (x0, x1) and u2 from (x2, x3) (u: [0, 1)).
//   topic  r = u1 * P_{K-1}; z = the first k with P_k > r
//   word   r = u2 * C_{z,V-1}; w = the first v with C_{z,v} > r
// When r rounds up to the total the draw takes the first index whose prefix equals the total, so
// a draw never falls off the end (nor picks an entry of weight 0).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "estep_kernels.h"
#include "philox.h"

namespace trlda {

enum : uint32_t {
    kSampleBetaNormal = 8,
    kSampleBetaAccept = 9,
    kSampleBetaBoost = 10,
    kSampleThetaNormal = 11,
    kSampleThetaAccept = 12,
    kSampleThetaBoost = 13,
    kSampleLength = 14,
    kSampleToken = 15,
};

constexpr int kSampleThreads = 256;                       // 4 waves
constexpr int kSamplePerLane = 16;                        // words of a chunk per lane
constexpr int kSampleChunk = kSampleThreads * kSamplePerLane;
constexpr int kSampleWaves = kSampleThreads / kWave;

__device__ __forceinline__ double sample_readlane(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// e_l of the header: the sum of lanes 0 .. l-1's `last`, added one lane after the other; `*total`
// gets e_64
__device__ __forceinline__ double sample_lane_offsets(double last, double *total)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    double acc = 0.0, mine = 0.0;
    for (int l = 0; l < kWave; ++l) {
        if (lane == l)
            mine = acc;
        acc = acc + sample_readlane(last, l);
    }
    *total = acc;
    return mine;
}

__device__ __forceinline__ double sample_wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = fmax(v, __shfl_xor(v, off, kWave));
    return v;
}

// the first i < n with c[i] > r; none (r rounded up to the total): the first i with c[i] >= total.
// Clamped to n - 1, so that a table the flag has already condemned is never read past its end.
__device__ __forceinline__ int sample_search(const double *__restrict__ c, int n, double r, double total)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (c[mid] > r)
            hi = mid;
        else
            lo = mid + 1;
    }
    if (lo == n) {
        lo = 0;
        hi = n;
        while (lo < hi) {
            const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
            if (c[mid] >= total)
                hi = mid;
            else
                lo = mid + 1;
        }
    }
    return min(lo, n - 1);
}

// 1. workgroup b: topic k = b % K, chunk b / K (neighbouring workgroups read neighbouring topics of
// lambda's columns); lg into the table, the chunk's max into cmax[k * nchunk + chunk]
__global__ __launch_bounds__(kSampleThreads) void sample_topics_kernel(int K, int V, int nchunk, uint32_t key0,
                                                                      uint32_t key1, const double *__restrict__ lambda,
                                                                      double *__restrict__ table,
                                                                      double *__restrict__ cmax)
{
    __shared__ double red[kSampleWaves];
    const int k = (int)(blockIdx.x % (unsigned)K), chunk = (int)(blockIdx.x / (unsigned)K);
    const int w0 = chunk * kSampleChunk;
    double *row = table + (size_t)k * V;
    double mx = -INFINITY;
    for (int i = threadIdx.x; i < kSampleChunk; i += kSampleThreads) {
        const int w = w0 + i;
        if (w >= V)
            break;
        double lg;
        [[clang::always_inline]] lg = philox_log_gamma(lambda[(size_t)w * K + k], (uint32_t)w, (uint32_t)k,
                                                       kSampleBetaNormal, kSampleBetaAccept, kSampleBetaBoost, key0,
                                                       key1);
        row[w] = lg;
        mx = fmax(mx, lg);
    }
    mx = sample_wave_max(mx);
    if ((threadIdx.x & (kWave - 1)) == 0)
        red[threadIdx.x / kWave] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = red[0];
        for (int v = 1; v < kSampleWaves; ++v)
            m = fmax(m, red[v]);
        cmax[(size_t)k * nchunk + chunk] = m;
    }
}

// 2. W = exp(lg - max_k) and the chunk's prefix L2 (header) in place; L2 at the chunk's last word
// into ctot[k * nchunk + chunk]
__global__ __launch_bounds__(kSampleThreads) void sample_topics_scan_kernel(int K, int V, int nchunk,
                                                                           double *__restrict__ table,
                                                                           const double *__restrict__ cmax,
                                                                           double *__restrict__ ctot)
{
#pragma clang fp contract(off)
    __shared__ double wtot[kSampleWaves];
    const int k = (int)(blockIdx.x % (unsigned)K), chunk = (int)(blockIdx.x / (unsigned)K);
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    double mx = -INFINITY;
    for (int c = 0; c < nchunk; ++c)
        mx = fmax(mx, cmax[(size_t)k * nchunk + c]);
    double *row = table + (size_t)k * V;
    const int w0 = chunk * kSampleChunk + threadIdx.x * kSamplePerLane;
    double q[kSamplePerLane];
    double run = 0.0;
#pragma unroll
    for (int j = 0; j < kSamplePerLane; ++j) {
        const int w = w0 + j;
        const double W = w < V ? exp(row[w] - mx) : 0.0;
        run = j ? run + W : W;
        q[j] = run;
    }
    double wave_total;
    const double e = sample_lane_offsets(q[kSamplePerLane - 1], &wave_total);
    if (lane == 0)
        wtot[wv] = wave_total;
    __syncthreads();
    double g = 0.0;
    for (int v = 0; v < wv; ++v)
        g = g + wtot[v];
#pragma unroll
    for (int j = 0; j < kSamplePerLane; ++j) {
        const int w = w0 + j;
        const double l2 = g + (e + q[j]);
        if (w < V)
            row[w] = l2;
        if (threadIdx.x == kSampleThreads - 1 && j == kSamplePerLane - 1)
            ctot[(size_t)k * nchunk + chunk] = l2;
    }
}

// 3. C = o_c + L2 (header); the row's last chunk checks the total
__global__ __launch_bounds__(kSampleThreads) void sample_topics_offset_kernel(int K, int V, int nchunk,
                                                                             double *__restrict__ table,
                                                                             const double *__restrict__ ctot,
                                                                             int *__restrict__ flag)
{
#pragma clang fp contract(off)
    const int k = (int)(blockIdx.x % (unsigned)K), chunk = (int)(blockIdx.x / (unsigned)K);
    double o = 0.0;
    for (int c = 0; c < chunk; ++c)
        o = o + ctot[(size_t)k * nchunk + c];
    if (chunk == nchunk - 1 && threadIdx.x == 0) {
        const double total = o + ctot[(size_t)k * nchunk + chunk];
        if (!(total > 0.0) || !(total <= 1.7976931348623157e308))
            atomicOr(flag, 1);
    }
    if (chunk == 0)
        return;
    double *row = table + (size_t)k * V;
    const int w0 = chunk * kSampleChunk;
    for (int i = threadIdx.x; i < kSampleChunk; i += kSampleThreads) {
        const int w = w0 + i;
        if (w >= V)
            break;
        row[w] = o + row[w];
    }
}

// 4. one wave per document, kSampleWaves documents per workgroup; pre: K x B, column d contiguous
__global__ __launch_bounds__(kSampleThreads) void sample_theta_kernel(int K, int B, int kpl, uint32_t key0,
                                                                     uint32_t key1, const double *__restrict__ alpha,
                                                                     double *__restrict__ pre,
                                                                     double *__restrict__ theta,
                                                                     int *__restrict__ flag)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    const int d = blockIdx.x * kSampleWaves + threadIdx.x / kWave;
    if (d >= B)
        return;
    const int k0 = lane * kpl, k1 = min(K, k0 + kpl);
    double *col = pre + (size_t)d * K;
    double mx = -INFINITY;
    for (int k = k0; k < k1; ++k) {
        double lg;
        [[clang::always_inline]] lg = philox_log_gamma(alpha[k], (uint32_t)k, (uint32_t)d, kSampleThetaNormal,
                                                       kSampleThetaAccept, kSampleThetaBoost, key0, key1);
        col[k] = lg;
        mx = fmax(mx, lg);
    }
    mx = sample_wave_max(mx);
    double run = 0.0;
    for (int k = k0; k < k1; ++k) {
        const double W = exp(col[k] - mx);
        col[k] = W;
        run = k > k0 ? run + W : W;
    }
    double S;
    const double es = sample_lane_offsets(run, &S);
    (void)es;
    if (!(S > 0.0) || !(S <= 1.7976931348623157e308)) {
        if (lane == 0)
            atomicOr(flag, 1);
    }
    run = 0.0;
    for (int k = k0; k < k1; ++k) {
        const double th = col[k] / S;
        if (theta)
            theta[(size_t)d * K + k] = th;
        run = k > k0 ? run + th : th;
        col[k] = run;                      // p_j for now; E_l is added below
    }
    double tot;
    const double E = sample_lane_offsets(run, &tot);
    for (int k = k0; k < k1; ++k)
        col[k] = E + col[k];
}

// 5. one thread per token of [0, nnz), nnz = indptr[B]; the grid strides
__global__ __launch_bounds__(kSampleThreads) void sample_tokens_kernel(int K, int V, int B, uint32_t key0,
                                                                      uint32_t key1,
                                                                      const int32_t *__restrict__ indptr,
                                                                      const double *__restrict__ pre,
                                                                      const double *__restrict__ table,
                                                                      int32_t *__restrict__ ids)
{
    const int64_t nnz = indptr[B];
    const int64_t stride = (int64_t)gridDim.x * kSampleThreads;
    for (int64_t t = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x; t < nnz; t += stride) {
        int lo = 0, hi = B;                  // indptr[lo] <= t < indptr[hi]
        while (hi - lo > 1) {
            const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
            if ((int64_t)indptr[mid] <= t)
                lo = mid;
            else
                hi = mid;
        }
        const int d = lo;
        uint32_t x[4];
        philox_block(x, (uint32_t)(t - indptr[d]), (uint32_t)d, 0u, kSampleToken, key0, key1);
        const double *P = pre + (size_t)d * K;
        const double pt = P[K - 1];
        const int z = sample_search(P, K, philox_u(x[0], x[1]) * pt, pt);
        const double *row = table + (size_t)z * V;
        const double ct = row[V - 1];
        ids[t] = sample_search(row, V, philox_u(x[2], x[3]) * ct, ct);
    }
}

}  // namespace trlda
