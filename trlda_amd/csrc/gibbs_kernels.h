// gibbs_kernels.h -- HIP kernels for gfx950 (MI355X) implementing LDA::updateVariablesGibbs
// (reference src/lda.cpp:224-293): collapsed Gibbs sampling of the topic assignments of a
// mini-batch's tokens, one wave64 per document.  Host side: trlda_hip.hip, gibbs_device.
//
// Launch sequence of one call:
//   1. rowsum_partial_kernel (+ rowsum_combine_kernel), exp_elog_beta_kernel (estep_kernels.h):
//      e = exp(psi(lambda) - psi(rowsum(lambda))), NORMALISED, for the batch's active words, in
//      a table of the Gibbs path's own (the VI path's buffers are not touched)      lda.cpp:238-239
//   2. gibbs_tokens_kernel  tokens per document (sum of the counts > 0); the host turns them
//      into int64 token offsets and a longest-first document order, once per batch
//   3. gibbs_docs_kernel<KPL>  per document: init, burn_in + num_samples sweeps, theta
//                                                                                  lda.cpp:241-290
//   4. gibbs_finish_kernel  sstats = count * unit over K x V, the counts back to 0
// Inside the update loops (trlda_model_online_update_gibbs / _batch_update_gibbs)
// 3 is followed by gibbs_mstep_kernel over the batch's active words instead of 4, and the table of
// 1 comes from the row sums the M-step left behind (exp_elog_beta_kernel's combined form).
//
// Semantics (the reference's, with the deviations DESIGN.md section 3.10 lists):
//   init    each token of entry j draws z from e[:, w] * theta[:, i] (theta0 column i -- the
//           reference reads column j, lda.cpp:254); counts = alpha + n
//   sweeps  s = 0 .. burn_in + num_samples - 1, entries in order, tokens in order:
//           counts[z] -= 1; z ~ e[:, w] * counts; counts[z] += 1; for s >= burn_in the token
//           adds one to the uint32 count of (z, w)
//   theta   Dirichlet(counts) of the final state; sstats = count / num_samples
//
// ---- the random stream (the contract tests/gibbs_host.py restates; the code is philox.h's) --
// Philox4x32-10 (Salmon et al., SC'11; Random123's constants), key = (k0, k1), the two 32-bit
// halves of the call's 64-bit key (trlda_model_gibbs_host takes them as two draws of the
// library's libc-compatible stream; those are 31-bit values, so there bits 31 and 63 of the key are
// always 0 and 62 bits vary).  Every draw is one Philox block of the counter
//     (c0, c1, c2, c3) = (index, document index in the batch, step, purpose)
// with
//     purpose 0  Dirichlet(1) initial theta      index = topic k, step 0
//     purpose 1  initial topic of a token        index = token t of the document, step 0
//     purpose 2  topic of a token in a sweep     index = token t, step = sweep s
//     purpose 3  gamma draw: the normal          index = topic k, step = attempt
//     purpose 4  gamma draw: the acceptance      index = topic k, step = attempt
//     purpose 5  gamma draw: the boost (a < 1)   index = topic k, step 0
// A token's index t counts the document's tokens in entry order, then token order.  The output
// words (x0, x1, x2, x3) become uniforms through x = x1 * 2^32 + x0 (and x3 * 2^32 + x2):
//     u      = (x >> 11) * 2^-53           in [0, 1)    histogram draws
//     u_open = ((x >> 12) + 0.5) * 2^-52   in (0, 1)    every draw that takes a logarithm
// Nothing of a draw depends on the launch geometry, the wave a document lands on, the order of
// the documents, the stream or the KPL variant.
//
// ---- one histogram draw (sweeps), in this order -----------------------------------------
// Lane l holds topics l*KPL .. l*KPL + KPL - 1 (topics >= K weigh 0):
//   p_j  = e_k * counts_k                         (one rounded product each)
//   q_j  = q_{j-1} + p_j, q_0 = p_0                (lane-local sequential prefix)
//   x_l  = q_{KPL-1}; Hillis-Steele over the 64 lanes, offsets 1, 2, 4, .., 32:
//          x_l = x_l + x_{l-off} for l >= off
//   total = x_63; r = u * total; excl_l = x_{l-1} (0 for lane 0)
//   the first lane L with x_L > r; in it the first j with excl_L + q_j > r, else its last
//   topic with p_j > 0.  No lane with x_l > r (u * total rounded up to total): the last topic
//   with p > 0 overall.  total not > 0 or not finite: the call fails with the reference's
//   "Something went wrong while sampling from histogram." (utils.cpp:198), through `flag`.
// Init draws (one lane per entry, the lanes in parallel): P_k = P_{k-1} + e_k * theta_k
// sequentially over k = 0 .. K-1, r = u * P_{K-1}, the first k with P_k > r, else the last
// k with a product > 0 (a P_{K-1} that is not > 0 or not finite fails the call as above; the
// tokens then take topic 0).  The tokens of an entry share walks of P, eight at a time.  No
// product or sum here is contracted into an FMA.
//
// ---- theta: Dirichlet(counts) ------------------------------------------------------------
// Per topic, log G with G ~ Gamma(a), a = counts_k (Marsaglia & Tsang 2000): for a < 1 the
// shape a + 1 and then log G += log(u_open) / a (purpose 5).  d = a' - 1/3, c = 1/sqrt(9d);
// attempt n = 0, 1, ..: x = sqrt(-2 log u_open) cos(2 pi u) from purpose 3's two uniforms,
// v = (1 + c x)^3 (rejected if 1 + c x <= 0), accepted when
// log(u_open of purpose 4) < x^2/2 + d - d v + d log v; log G = log d + log v.  After
// kGammaTries attempts (acceptance is above 0.95 per attempt) log d is taken.
// theta_k = exp(log G_k - max) / sum over the topics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "estep_kernels.h"
#include "philox.h"

namespace trlda {

constexpr int kGibbsMaxK = 1024;      // KPL <= 16 topics per lane
constexpr int kGibbsWaves = 4;        // documents (waves) per workgroup
constexpr int kGibbsInitBatch = 8;   // init: tokens of one entry that share a walk of the prefix

enum : uint32_t {
    kGibbsInitTheta = 0,
    kGibbsInitToken = 1,
    kGibbsSweep = 2,
    kGibbsGammaNormal = 3,
    kGibbsGammaAccept = 4,
    kGibbsGammaBoost = 5,
};

struct GibbsArgs {
    int K, B, sweeps, burn_in;
    uint32_t key0, key1;
    const int32_t *indptr, *ids, *cnts;
    const int32_t *order;        // documents, most tokens first
    const int64_t *tok_off;      // B: first token of each document in `z`
    const double *eeb;           // K x V, normalised; the batch's active columns
    const double *alpha;         // K
    const double *theta0;        // K x B, or nullptr: Dirichlet(1)
    double *theta;               // K x B
    uint16_t *z;                 // topic of every token
    uint32_t *cnt;               // K x V: tokens per (topic, word), summed over the samples
    int *flag;                   // set to 1 by a histogram that sums to 0 or is not finite
};

__device__ __forceinline__ double readlane_d(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_allsum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, kWave);
    return v;
}

__device__ __forceinline__ double wave_allmax(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = fmax(v, __shfl_xor(v, off, kWave));
    return v;
}

// One histogram draw in the order of the header ("one histogram draw"): lane l holds the weights
// p_0 .. p_{KPL-1} of topics l*KPL .. (0 for topics >= K), u is the draw's uniform, the same in every
// lane.  Returns the topic, the same in every lane, or -1 when the histogram's total is not > 0 or
// not finite; `total` is x_63.  Shared with l2r_kernels.h.
template <int KPL>
__device__ __forceinline__ int histogram_draw(const double (&p)[KPL], double u, int lane, double &total)
{
    double qv[KPL];
    int lastnz = -1;
#pragma unroll
    for (int q = 0; q < KPL; ++q) {
        qv[q] = q ? __dadd_rn(qv[q - 1], p[q]) : p[q];
        if (p[q] > 0.0)
            lastnz = q;
    }
    double x = qv[KPL - 1];
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const double y = __shfl_up(x, off, kWave);
        if (lane >= off)
            x = __dadd_rn(x, y);
    }
    total = readlane_d(x, kWave - 1);
    double excl = __shfl_up(x, 1, kWave);
    if (lane == 0)
        excl = 0.0;
    const double r = __dmul_rn(u, total);
    if (!(total > 0.0) || !(total <= 1.7976931348623157e308))
        return -1;
    const unsigned long long hit = __ballot(x > r);
    int pick = -1, L = 0;
    if (hit) {
        L = __ffsll((long long)hit) - 1;
#pragma unroll
        for (int q = KPL - 1; q >= 0; --q)
            if (__dadd_rn(excl, qv[q]) > r)
                pick = q;
        if (pick < 0)
            pick = lastnz;
        pick = __builtin_amdgcn_readlane(pick, L);
    }
    if (pick < 0) {
        const unsigned long long nz = __ballot(lastnz >= 0);
        L = 63 - __clzll((long long)nz);
        pick = __builtin_amdgcn_readlane(lastnz, L);
    }
    return L * KPL + pick;
}

// log of a Gamma(a) draw of topic k of document `doc` (philox.h's recipe, purposes 3 / 4 / 5)
__device__ inline double gibbs_log_gamma(double a, uint32_t k, uint32_t doc, uint32_t k0, uint32_t k1)
{
    return philox_log_gamma(a, k, doc, kGibbsGammaNormal, kGibbsGammaAccept, kGibbsGammaBoost, k0, k1);
}

// tokens per document: the counts > 0 of its entries (lda.cpp:251-262 draws `wordcount` topics)
template <int T>
__global__ __launch_bounds__(T) void gibbs_tokens_kernel(int B, const int32_t *__restrict__ indptr,
                                                         const int32_t *__restrict__ cnts,
                                                         int64_t *__restrict__ tokens)
{
    const int d = blockIdx.x * T + threadIdx.x;
    if (d >= B)
        return;
    int64_t n = 0;
    for (int j = indptr[d]; j < indptr[d + 1]; ++j)
        n += max(cnts[j], 0);
    tokens[d] = n;
}

// sstats = count * unit (unit = 1 / num_samples; 0 when there are no samples), counts reset
template <int T>
__global__ __launch_bounds__(T) void gibbs_finish_kernel(size_t total, double unit, uint32_t *__restrict__ cnt,
                                                         double *__restrict__ sstats)
{
    const size_t stride = (size_t)gridDim.x * T;
    for (size_t i = (size_t)blockIdx.x * T + threadIdx.x; i < total; i += stride) {
        const uint32_t c = cnt[i];
        sstats[i] = (double)c * unit;
        if (c)
            cnt[i] = 0u;
    }
}

// ---- inside the update loops (trlda_model_online_update_gibbs / _batch_update_gibbs) ------
// Per E-step of a trust-region iteration or epoch, over the batch's ACTIVE columns only (a word
// outside the batch has no tokens: its lambda was given its final value once per call):
//   s      = count * unit                               (unit = 1 / num_samples, 0 without samples)
//   lambda = omr * lambda' + rho * (eta + scale * s)    onlinelda.cpp:99-100 (omr = 1 - rho,
//            scale = D / B), batchlda.cpp:60 (omr = 0 without reading lambda', rho = 1, scale = 1)
// evaluated in that order without contraction; the counts go back to 0 (they are zero between
// calls), s is kept only where `sstats` is given, and each workgroup leaves the row sums of the
// columns it wrote as one row of `partial` (its columns in order, then its column slots in order).
// Workgroup g takes positions [n g / G, n (g + 1) / G) of the active list.  K <= 256 (KPT = 1):
// K threads per column, T / K column slots; K > 256 (KPT = 4): one column at a time, topic
// k = thread + q T.
constexpr int kGibbsMstepThreads = 256;
constexpr int kGibbsMstepMaxBlocks = 1024;

template <int T, int KPT>
__global__ __launch_bounds__(T) void gibbs_mstep_kernel(int K, int n_active, int cpb,
                                                        const int32_t *__restrict__ active, double omr,
                                                        double rho, double eta, double scale, double unit,
                                                        const double *lambda_prime /* or nullptr */,
                                                        uint32_t *__restrict__ cnt, double *lambda,
                                                        double *__restrict__ sstats /* or nullptr */,
                                                        double *__restrict__ partial)
{
#pragma clang fp contract(off)
    __shared__ double scratch[T];
    const int P = KPT == 1 ? K : T;
    const int slot = threadIdx.x / P, kp = threadIdx.x - slot * P;
    const int j0 = (int)((long long)n_active * blockIdx.x / gridDim.x);
    const int j1 = (int)((long long)n_active * (blockIdx.x + 1) / gridDim.x);
    double acc[KPT];
#pragma unroll
    for (int q = 0; q < KPT; ++q)
        acc[q] = 0.0;
    if (slot < cpb) {
        for (int j = j0 + slot; j < j1; j += cpb) {
            const size_t col = (size_t)active[j] * K;
#pragma unroll
            for (int q = 0; q < KPT; ++q) {
                const int k = kp + q * T;
                if (KPT == 1 || k < K) {
                    const size_t i = col + k;
                    const uint32_t c = cnt[i];
                    if (c)
                        cnt[i] = 0u;
                    const double s = (double)c * unit;
                    const double hat = eta + scale * s;
                    const double lp = lambda_prime ? omr * lambda_prime[i] : 0.0;
                    const double y = lp + rho * hat;
                    lambda[i] = y;
                    if (sstats)
                        sstats[i] = s;
                    acc[q] += y;
                }
            }
        }
    }
    double *row = partial + (size_t)blockIdx.x * K;
    if constexpr (KPT == 1) {
        if (slot < cpb)
            scratch[slot * K + kp] = acc[0];
        __syncthreads();
        for (int k = threadIdx.x; k < K; k += T) {
            double s = scratch[k];
            for (int sl = 1; sl < cpb; ++sl)
                s += scratch[sl * K + k];
            row[k] = s;
        }
    } else {
#pragma unroll
        for (int q = 0; q < KPT; ++q) {
            const int k = kp + q * T;
            if (k < K)
                row[k] = acc[q];
        }
    }
}

// flag = 1 when an element of lambda is not > 0 (NaN included): what trlda_model_set_lambda
// learns from a host copy, for the lambda an update left behind
template <int T>
__global__ __launch_bounds__(T) void gibbs_nonpositive_kernel(size_t total, const double *__restrict__ lambda,
                                                              int *__restrict__ flag)
{
    const size_t stride = (size_t)gridDim.x * T;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * T + threadIdx.x; i < total; i += stride)
        bad |= !(lambda[i] > 0.0);
    if (__any(bad) && (threadIdx.x & (kWave - 1)) == 0)
        atomicOr(flag, 1);
}

// One wave per document, kGibbsWaves documents per workgroup; the waves never wait for each other.
// LDS per wave: the initial theta column (K doubles) and the init histogram (K ints).
template <int KPL>
__global__ __launch_bounds__(kGibbsWaves * kWave) void gibbs_docs_kernel(GibbsArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double gibbs_lds[];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int slot = blockIdx.x * kGibbsWaves + wv;
    if (slot >= a.B)
        return;
    const int K = a.K;
    double *th = gibbs_lds + (size_t)wv * K;
    int *hist = reinterpret_cast<int *>(gibbs_lds + (size_t)kGibbsWaves * K) + (size_t)wv * K;
    const int doc = a.order[slot];
    const uint32_t udoc = (uint32_t)doc;
    const int e0 = a.indptr[doc], e1 = a.indptr[doc + 1];
    const int64_t zbase = a.tok_off[doc];
    const uint32_t k0 = a.key0, k1 = a.key1;

    // 1. the initial theta column: the caller's, or Dirichlet(1) = normalised Exp(1) draws
    if (a.theta0) {
        for (int k = lane; k < K; k += kWave)
            th[k] = a.theta0[(size_t)doc * K + k];
    } else {
        double part = 0.0;
        for (int k = lane; k < K; k += kWave) {
            uint32_t w[4];
            philox_block(w, (uint32_t)k, udoc, 0u, kGibbsInitTheta, k0, k1);
            const double x = -log(philox_u_open(w[0], w[1]));
            th[k] = x;
            part += x;
        }
        const double s = wave_allsum(part);
        for (int k = lane; k < K; k += kWave)
            th[k] = th[k] / s;
    }
    for (int k = lane; k < K; k += kWave)
        hist[k] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

    // 2. init (lda.cpp:244-262): the lanes take 64 entries at a time, each its entry's tokens
    uint32_t ntok = 0;
    bool bad = false;
    for (int c0 = e0; c0 < e1; c0 += kWave) {
        const int j = c0 + lane;
        const int c = j < e1 ? max(a.cnts[j], 0) : 0;
        int incl = c;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const int y = __shfl_up(incl, off, kWave);
            if (lane >= off)
                incl += y;
        }
        const uint32_t t0 = ntok + (uint32_t)(incl - c);
        ntok += (uint32_t)__shfl(incl, kWave - 1, kWave);
        if (c > 0) {
            const double *col = a.eeb + (size_t)a.ids[j] * K;
            double tot = 0.0;
            for (int k = 0; k < K; ++k)
                tot = __dadd_rn(tot, __dmul_rn(col[k], th[k]));
            const bool ok = tot > 0.0 && tot <= 1.7976931348623157e308;
            bad |= !ok;
            // the entry's tokens kGibbsInitBatch at a time, each group in ONE walk of the prefix:
            // P_k is formed once per walk and compared with every token of the group (the same
            // P_k and the same draws as one walk per token; the walk ends once P_k exceeds the
            // group's largest r, by when every token of the group has its topic)
            for (int t1 = 0; t1 < c; t1 += kGibbsInitBatch) {
                const int n = min(kGibbsInitBatch, c - t1);
                double r[kGibbsInitBatch];
                int z[kGibbsInitBatch];
                double rmax = 0.0;
#pragma unroll
                for (int u = 0; u < kGibbsInitBatch; ++u) {
                    uint32_t w[4];
                    philox_block(w, t0 + (uint32_t)(t1 + u), udoc, 0u, kGibbsInitToken, k0, k1);
                    r[u] = __dmul_rn(philox_u(w[0], w[1]), tot);
                    z[u] = u < n ? -1 : 0;
                    if (u < n)
                        rmax = fmax(rmax, r[u]);
                }
                int last = 0;
                if (ok) {
                    double P = 0.0;
                    for (int k = 0; k < K; ++k) {
                        const double p = __dmul_rn(col[k], th[k]);
                        P = __dadd_rn(P, p);
                        if (p > 0.0)
                            last = k;
#pragma unroll
                        for (int u = 0; u < kGibbsInitBatch; ++u)
                            if (z[u] < 0 && P > r[u])
                                z[u] = k;
                        if (P > rmax)
                            break;
                    }
                }
#pragma unroll
                for (int u = 0; u < kGibbsInitBatch; ++u) {
                    if (u < n) {
                        const int zz = z[u] < 0 ? last : z[u];
                        a.z[zbase + t0 + t1 + u] = (uint16_t)zz;
                        atomicAdd(&hist[zz], 1);
                    }
                }
            }
        }
    }
    if (__any(bad))
        atomicOr(a.flag, 1);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

    // counts = alpha + n, lane l holding topics l*KPL .. l*KPL + KPL - 1
    double cnt_r[KPL];
#pragma unroll
    for (int q = 0; q < KPL; ++q) {
        const int k = lane * KPL + q;
        cnt_r[q] = k < K ? a.alpha[k] + (double)hist[k] : 0.0;
    }

    // 3. sweeps (lda.cpp:264-285).  The document's topics are read and written 64 tokens at a
    // time: lane l holds token base + l's topic, word and uniform of this sweep.
    if (a.sweeps > 0 && ntok > 0) {
        // (the init's stores came from other lanes of this wave: drained before the reads)
        stores_acknowledged();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        for (int s = 0; s < a.sweeps; ++s) {
            const bool collect = s >= a.burn_in;
            uint32_t tk = 0;
            int zc = 0, wc = 0;
            double uc = 0.0;
            bool sweep_bad = false;
            // e[:, w] of an entry is loaded once for its c tokens, and the next entry's column is
            // loaded while this one's tokens run (an L2 hit costs about as much as a token step)
            double e_r[KPL], e_nx[KPL];
#pragma unroll
            for (int q = 0; q < KPL; ++q) {
                const int k = lane * KPL + q;
                e_nx[q] = k < K ? a.eeb[(size_t)a.ids[e0] * K + k] : 0.0;
            }
            for (int j = e0; j < e1; ++j) {
                const int c = max(a.cnts[j], 0);
                const int w = a.ids[j];
#pragma unroll
                for (int q = 0; q < KPL; ++q)
                    e_r[q] = e_nx[q];
                if (j + 1 < e1) {
                    const double *nx = a.eeb + (size_t)a.ids[j + 1] * K;
#pragma unroll
                    for (int q = 0; q < KPL; ++q) {
                        const int k = lane * KPL + q;
                        e_nx[q] = k < K ? nx[k] : 0.0;
                    }
                }
                if (c == 0)
                    continue;
                for (int t = 0; t < c; ++t, ++tk) {
                    const int ql = (int)(tk & (kWave - 1));
                    if (ql == 0) {
                        if (tk > 0) {                   // the chunk behind: topics back, statistics out
                            const uint32_t idx = tk - kWave + lane;
                            a.z[zbase + idx] = (uint16_t)zc;
                            if (collect)
                                atomicAdd(&a.cnt[(size_t)wc * K + zc], 1u);
                        }
                        const uint32_t idx = tk + lane;
                        uint32_t rw[4];
                        philox_block(rw, idx, udoc, (uint32_t)s, kGibbsSweep, k0, k1);
                        uc = philox_u(rw[0], rw[1]);
                        zc = idx < ntok ? (int)a.z[zbase + idx] : 0;
                    }
                    const int zold = __builtin_amdgcn_readlane(zc, ql);
#pragma unroll
                    for (int q = 0; q < KPL; ++q)
                        if (lane * KPL + q == zold)
                            cnt_r[q] = cnt_r[q] - 1.0;
                    double p[KPL];
#pragma unroll
                    for (int q = 0; q < KPL; ++q)
                        p[q] = __dmul_rn(e_r[q], cnt_r[q]);
                    double total;
                    int znew = histogram_draw<KPL>(p, readlane_d(uc, ql), lane, total);
                    if (znew < 0) {
                        sweep_bad = true;
                        znew = zold;
                    }
#pragma unroll
                    for (int q = 0; q < KPL; ++q)
                        if (lane * KPL + q == znew)
                            cnt_r[q] = cnt_r[q] + 1.0;
                    if (lane == ql) {
                        zc = znew;
                        wc = w;
                    }
                }
            }
            // the last chunk
            {
                const uint32_t cbase = (tk - 1) & ~(uint32_t)(kWave - 1);
                const uint32_t idx = cbase + lane;
                if (idx < ntok) {
                    a.z[zbase + idx] = (uint16_t)zc;
                    if (collect)
                        atomicAdd(&a.cnt[(size_t)wc * K + zc], 1u);
                }
            }
            if (sweep_bad)
                atomicOr(a.flag, 1);
        }
    }

    // 4. theta = Dirichlet(counts) (lda.cpp:288)
    double lg[KPL];
    double mx = -INFINITY;
#pragma unroll
    for (int q = 0; q < KPL; ++q) {
        const int k = lane * KPL + q;
        lg[q] = k < K ? gibbs_log_gamma(cnt_r[q], (uint32_t)k, udoc, k0, k1) : -INFINITY;
        mx = fmax(mx, lg[q]);
    }
    mx = wave_allmax(mx);
    double part = 0.0;
#pragma unroll
    for (int q = 0; q < KPL; ++q) {
        lg[q] = exp(lg[q] - mx);
        part += lg[q];
    }
    const double s = wave_allsum(part);
#pragma unroll
    for (int q = 0; q < KPL; ++q) {
        const int k = lane * KPL + q;
        if (k < K)
            a.theta[(size_t)doc * K + k] = lg[q] / s;
    }
}

}  // namespace trlda
