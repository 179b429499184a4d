// trlda_amd/csrc/relevance_kernels.h -- topic words ranked by relevance (Sievert & Shirley 2014) and
// corpus terms ranked by saliency (Chuang, Manning & Heer 2012), and the topic prevalence of a corpus
// that both can be weighted by.  No reference counterpart.
//
// The contract.
//   R_k = sum_w lambda_kw,  beta_kw = lambda_kw / R_k.
//   Topic weights pi: none given, pi_k = R_k / sum_j R_j (each topic's share of lambda's mass); a
//     given length-K array must be finite and strictly positive and is normalised to sum 1 on the host.
//   p_w = sum_k c_k lambda_kw,  c_k = pi_k / R_k: the marginal word probability.  The sum over k runs
//     in an order that depends on K alone.
//   Relevance  r_kw(l) = l log beta_kw + (1 - l) log(beta_kw / p_w), evaluated as
//     log lambda_kw - log R_k - (1 - l) log p_w,  l = weight in [0, 1].  Row k of the result is
//     np.lexsort((arange(V), -r_k))[:top_n]: larger r first, equal values by smaller word id (the tie
//     rule and the 64-bit keys of coherence_kernels.h, which order negative doubles too).
//   Distinctiveness  D_w = sum_k q_kw (log q_kw - log pi_k),  q_kw = c_k lambda_kw / p_w = p(k | w):
//     KL(p(k | w) || pi) >= 0.
//   Saliency  S_w = p_w D_w;  sum_w S_w is the mutual information of topic and word, <= log K.
//     Salient words: np.lexsort((arange(V), -S))[:top_n].
//   1 <= top_n <= min(V, 100).
//   A lambda with an element <= 0 or not finite: the column pass raises a device flag, the call fails
//     (TRLDA_ERR_VALUE) and nothing is written to the outputs.
//   Prevalence over a corpus  pi_k ~ sum_d N_d gamma_dk / sum_j gamma_dj,  N_d = the sum of document
//     d's positive counts (1 with weight_by_length off); a document without a positive count is
//     skipped.  One addition per document per topic, in stream order; each document's sum_j gamma_dj
//     in an order that depends on K alone: bitwise independent of how the stream is cut into batches.
//     Normalised on the host.
// No float atomics; nothing depends on the launch geometry; every result repeats bitwise.
//
// The kernels.  lambda is column-major: a word's K values are contiguous.
//   relevance_coef_kernel     one wave: S = sum_k R_k (lane-local in ascending k, then the butterfly),
//                             then c_k, log R_k, log pi_k;
//   relevance_column_kernel   a wave per word: p_w over the column (lane-local in ascending k, then
//                             the butterfly), then D_w from a second read of the column (it is in
//                             L2 / L1: 8 K bytes), S_w, log p_w, and the bad-lambda flag;
//   relevance_tile_kernel     topn_tile_kernel with the key of r_kw computed while staging: the
//                             tile's 8 log R_k and 1024 log p_w are staged in LDS beside the keys;
//   relevance_final_kernel    topn_merge_kernel's last level that also gives the scores, by
//                             inverting the keys.
//   (the levels between are topn_merge_kernel itself; the salient words are topn_tile_kernel over
//   the 1 x V vector S, then the same levels.)
//   prevalence_docs_kernel    a wave per document: N_d and 1 / sum_j gamma_dj;
//   prevalence_add_kernel     a thread per topic walks the batch's documents in order and adds
//                             (N_d gamma_dk) (1 / sum gamma_d) to its fp64 sum.
#pragma once

#include "coherence_kernels.h"
#include "gibbs_kernels.h"

namespace trlda {

constexpr int kRelevanceThreads = 256;                 // the column pass: 4 words per workgroup
constexpr int kRelevanceTileLds =                      // the keys, then 8 log R_k, then 1024 log p_w
    (kTopnTileTopics * kTopnTileStride + kTopnTileTopics + kTopnTileWords) * (int)sizeof(uint64_t);

// the double a key of topn_key came from (+0 for either zero; a NaN for a NaN)
__device__ __forceinline__ double topn_unkey(uint64_t key)
{
    const uint64_t u = (key >> 63) ? (key ^ 0x8000000000000000ull) : ~key;
    return __longlong_as_double((long long)u);
}

// Grid 1, one wave.  pi_in: the normalised weights, or nullptr for R_k / S.  coef: c | log R | log pi,
// K each.
__global__ __launch_bounds__(kWave) void relevance_coef_kernel(int K, const double *__restrict__ rs,
                                                               const double *__restrict__ pi_in,
                                                               double *__restrict__ coef)
{
    const int lane = threadIdx.x;
    double S = 0.0;
    if (!pi_in) {
        double part = 0.0;
        for (int k = lane; k < K; k += kWave)
            part += rs[k];
        S = wave_allsum(part);
    }
    for (int k = lane; k < K; k += kWave) {
        const double R = rs[k];
        const double pi = pi_in ? pi_in[k] : R / S;
        coef[k] = pi / R;
        coef[K + k] = log(R);
        coef[2 * (size_t)K + k] = log(pi);
    }
}

// Grid ceil(V / 4), a wave per word.  stats: p | D | S | log p, V each.  *bad is set to 1 by a
// lambda <= 0 or not finite (every writer stores the same value).
__global__ __launch_bounds__(kRelevanceThreads) void relevance_column_kernel(int K, int V,
                                                                             const double *__restrict__ lambda,
                                                                             const double *__restrict__ coef,
                                                                             double *__restrict__ stats,
                                                                             int *__restrict__ bad)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int w = blockIdx.x * (kRelevanceThreads / kWave) + threadIdx.x / kWave;
    if (w >= V)
        return;
    const double *col = lambda + (size_t)w * K;
    const double *logpi = coef + 2 * (size_t)K;
    double part = 0.0;
    bool wrong = false;
    for (int k = lane; k < K; k += kWave) {
        const double l = col[k];
        wrong |= !(l > 0.0) || l > 1.79769313486231570815e+308;
        part += coef[k] * l;
    }
    const double p = wave_allsum(part);
    part = 0.0;
    for (int k = lane; k < K; k += kWave) {
        const double q = coef[k] * col[k] / p;
        part += q * (log(q) - logpi[k]);
    }
    const double D = wave_allsum(part);
    if (wrong)
        *bad = 1;
    if (lane == 0) {
        stats[w] = p;
        stats[(size_t)V + w] = D;
        stats[2 * (size_t)V + w] = p * D;
        stats[3 * (size_t)V + w] = log(p);
    }
}

// topn_tile_kernel's grid and candidates; the value of (k, w) is
// log lambda_kw - log R_k - om log p_w, om = 1 - weight.  Dynamic LDS: kRelevanceTileLds.
__global__ __launch_bounds__(kTopnThreads) void relevance_tile_kernel(int K, int V, int n, double om,
                                                                      const double *__restrict__ lambda,
                                                                      const double *__restrict__ logR,
                                                                      const double *__restrict__ logp,
                                                                      uint64_t *__restrict__ ckey,
                                                                      int32_t *__restrict__ cid)
{
    extern __shared__ uint64_t tile[];       // [8][kTopnTileStride], then the logs
    double *slogR = reinterpret_cast<double *>(tile + kTopnTileTopics * kTopnTileStride);
    double *slogp = slogR + kTopnTileTopics;
    const int k0 = blockIdx.x * kTopnTileTopics, w0 = blockIdx.y * kTopnTileWords;
    const int kt = min(kTopnTileTopics, K - k0);
    const int wt = min(kTopnTileWords, V - w0);
    for (int e = threadIdx.x; e < kTopnTileWords; e += kTopnThreads)
        if (e < wt)
            slogp[e] = logp[w0 + e];
    if (threadIdx.x < kt)
        slogR[threadIdx.x] = logR[k0 + threadIdx.x];
    __syncthreads();
    for (int e = threadIdx.x; e < kTopnTileTopics * kTopnTileWords; e += kTopnThreads) {
        const int kk = e % kTopnTileTopics, ww = e / kTopnTileTopics;
        if (kk < kt && ww < wt) {
            const double r = log(lambda[(size_t)(w0 + ww) * K + k0 + kk]) - slogR[kk] - om * slogp[ww];
            tile[kk * kTopnTileStride + ww] = topn_key(r);
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const size_t C = (size_t)gridDim.y * n;
    const int kk = wid;
    if (kk < kt) {
        uint64_t key[kTopnPerLane];
        int32_t id[kTopnPerLane];
#pragma unroll
        for (int j = 0; j < kTopnPerLane; ++j) {
            const int ww = lane + kWave * j;
            const bool in = ww < wt;
            key[j] = in ? tile[kk * kTopnTileStride + ww] : 0ull;
            id[j] = in ? w0 + ww : kTopnPadId;
        }
        uint64_t T;
        int32_t I;
        topn_threshold(key, id, n, T, I);
        const size_t at = (size_t)(k0 + kk) * C + (size_t)blockIdx.y * n;
        topn_emit(key, id, n, T, I, ckey + at, cid + at);
    }
}

// The last level: grid rows, one wave each; row k's C_in <= 1024 candidates give words_out[k * n + r]
// and scores_out[k * n + r], the word of rank r and the value its key came from.
__global__ __launch_bounds__(kWave) void relevance_final_kernel(int n, int C_in, const uint64_t *__restrict__ ikey,
                                                                const int32_t *__restrict__ iid,
                                                                int32_t *__restrict__ words_out,
                                                                double *__restrict__ scores_out)
{
    __shared__ uint64_t skey[kTopnMax];
    __shared__ int32_t sid[kTopnMax];
    const int lane = threadIdx.x;
    const int k = blockIdx.x;
    const uint64_t *ik = ikey + (size_t)k * C_in;
    const int32_t *ii = iid + (size_t)k * C_in;
    uint64_t key[kTopnPerLane];
    int32_t id[kTopnPerLane];
#pragma unroll
    for (int j = 0; j < kTopnPerLane; ++j) {
        const int p = lane + kWave * j;
        const bool in = p < C_in;
        key[j] = in ? ik[p] : 0ull;
        id[j] = in ? ii[p] : kTopnPadId;
    }
    uint64_t T;
    int32_t I;
    topn_threshold(key, id, n, T, I);
    topn_emit(key, id, n, T, I, skey, sid);
    __syncthreads();
    // the n selected pairs are distinct words: each one's rank is the number that beat it
    for (int p = lane; p < n; p += kWave) {
        const uint64_t kp = skey[p];
        const int32_t ip = sid[p];
        int r = 0;
        for (int q = 0; q < n; ++q)
            r += (skey[q] > kp || (skey[q] == kp && sid[q] < ip)) ? 1 : 0;
        words_out[(size_t)k * n + r] = ip;
        scores_out[(size_t)k * n + r] = topn_unkey(kp);
    }
}

// Grid ceil(B / 4), a wave per document of a batch: nd[d] = the sum of its positive counts (by_length)
// or 1 when it has one, 0 when it has none; inv[d] = 1 / sum_j gamma_dj (lane-local in ascending j,
// then the butterfly).  gamma: K x B, K contiguous.
__global__ __launch_bounds__(kRelevanceThreads) void prevalence_docs_kernel(int K, int B, int by_length,
                                                                            const int32_t *__restrict__ indptr,
                                                                            const int32_t *__restrict__ cnts,
                                                                            const double *__restrict__ gamma,
                                                                            double *__restrict__ nd,
                                                                            double *__restrict__ inv)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int d = blockIdx.x * (kRelevanceThreads / kWave) + threadIdx.x / kWave;
    if (d >= B)
        return;
    long long n = 0;
    for (int p = indptr[d] + lane; p < indptr[d + 1]; p += kWave) {
        const int c = cnts[p];
        n += c > 0 ? c : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        n += __shfl_xor(n, off, kWave);
    const double *g = gamma + (size_t)d * K;
    double part = 0.0;
    for (int k = lane; k < K; k += kWave)
        part += g[k];
    const double s = wave_allsum(part);
    if (lane == 0) {
        nd[d] = n > 0 ? (by_length ? (double)n : 1.0) : 0.0;
        inv[d] = 1.0 / s;
    }
}

// Grid ceil(K / 256), a thread per topic: sums[k] += (nd[d] gamma_dk) inv[d] for d = 0 .. B - 1 in
// order, documents with nd = 0 left out.  Thread 0 adds the number of documents that contributed.
__global__ __launch_bounds__(kRelevanceThreads) void prevalence_add_kernel(int K, int B,
                                                                           const double *__restrict__ gamma,
                                                                           const double *__restrict__ nd,
                                                                           const double *__restrict__ inv,
                                                                           double *__restrict__ sums,
                                                                           long long *__restrict__ docs)
{
    const int k = blockIdx.x * kRelevanceThreads + threadIdx.x;
    if (k >= K)
        return;
    double acc = sums[k];
    long long used = 0;
    for (int d = 0; d < B; ++d) {
        const double n = nd[d];
        if (n > 0.0) {
            acc += (n * gamma[(size_t)d * K + k]) * inv[d];
            ++used;
        }
    }
    sums[k] = acc;
    if (k == 0)
        *docs += used;
}

}  // namespace trlda
