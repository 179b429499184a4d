// trlda_amd/csrc/diagnostics_kernels.h -- per-topic quality diagnostics, the columns of MALLET's
// --diagnostics-file that need lambda or the documents' gamma.  No reference
// counterpart.
//
// The contract.  Notation of relevance_kernels.h: R_k = sum_w lambda_kw (lambda_rowsums),
// c_k = 1 / R_k, beta_kw = lambda_kw c_k (one rounded product), p_w and log p_w those
// relevance_column_kernel stores under the given or default topic weights, log beta_kw =
// log lambda_kw - log R_k.
//   Word side, per topic k:
//     Q_k = sum_w beta_kw^2                                   eff_num_words = 1 / Q_k
//     E_k = sum_w beta_kw log beta_kw                         word_entropy H_k = -E_k
//     C_k = sum_w beta_kw (log beta_kw - log p_w)             corpus_dist = KL(beta_k || p) >= 0
//     uniform_dist = log V - H_k = KL(beta_k || uniform), formed on the host from H_k
//     exclusivity = the mean over the topic's top_n listed words, in rank order, of beta_kw / u_w,
//       u_w = sum_j beta_jw: lane-local in ascending j, then the wave_allsum butterfly, over the same
//       rounded products beta_jw.  K = 1: u_w = beta_0w and every ratio, and the mean, is exactly 1.
//     The sums over w: the vocabulary is cut into chunks of kDiagChunk consecutive words; a chunk's
//     words are added in ascending order, then the chunks in ascending order.  The order is a function
//     of K and V alone.
//     A lambda with an element <= 0 or not finite: relevance_column_kernel's flag is raised, the call
//     fails (TRLDA_ERR_VALUE) and nothing is written to the outputs.
//   Document side, per document d with a positive count (the others are skipped), gamma K x B:
//     N_d = the sum of its positive counts (int64), 1 with weight_by_length off;
//     inv_d = 1 / sum_j gamma_dj, the sum formed as prevalence_docs_kernel forms it;
//     a_dk = (N_d gamma_dk) inv_d, the product prevalence_add_kernel adds, and as there the rounded
//       N_d gamma_dk times inv_d goes into T_k = sum_d a_dk through one fused multiply-add: T_k is
//       bitwise the prevalence sum of the same documents;
//     A_k = sum_d a_dk log a_dk, a_dk rounded;  document_entropy = log T_k - A_k / T_k (host, long double), the
//       entropy of p(d | k) = a_dk / T_k;
//     theta_dk = gamma_dk inv_d;  docs_high_k, docs_low_k count theta_dk > high and theta_dk > low;
//     rank_1_docs_k counts the documents whose largest gamma_dj is j = k, ties to the smaller j.
//     One fp64 addition per document per sum, in stream order: bitwise independent of how the stream
//     is cut into batches.
// No atomics; nothing depends on the launch geometry; every result repeats bitwise.
//
// The kernels.  lambda is column-major: a word's K values are contiguous.
//   diagnostics_scale_kernel        a thread per topic: c_k = 1 / R_k;
//   diagnostics_rows_kernel         a workgroup per (chunk of kDiagChunk words, kDiagThreads topics):
//                                   thread t owns one topic, walks the chunk's words in ascending
//                                   order with Q, E and C in registers (the reads across t
//                                   coalesce), and writes its three partials to the chunk's row of
//                                   3 K;
//   diagnostics_combine_kernel      a thread per (sum, topic): adds the chunk rows in ascending order;
//   diagnostics_exclusivity_kernel  a gather, a wave per (topic, rank): u_w and beta_kw / u_w;
//   diagnostics_mean_kernel         a thread per topic: the top_n ratios in rank order, / top_n;
//   topicdiag_docs_kernel           a wave per document: prevalence_docs_kernel's N_d and inv_d, and
//                                   the argmax as a wave reduction over (value, -k);
//   topicdiag_add_kernel            a thread per topic walks the batch's documents in order.
#pragma once

#include "relevance_kernels.h"

namespace trlda {

constexpr int kDiagChunk = 256;                        // words per workgroup of the row pass
constexpr int kDiagThreads = 64;                       // topics per workgroup of the row pass

// Grid ceil(K / 256).  cinv[k] = 1 / R_k.
__global__ __launch_bounds__(kRelevanceThreads) void diagnostics_scale_kernel(int K, const double *__restrict__ rs,
                                                                              double *__restrict__ cinv)
{
    const int k = blockIdx.x * kRelevanceThreads + threadIdx.x;
    if (k < K)
        cinv[k] = 1.0 / rs[k];
}

// Grid (ceil(V / kDiagChunk), ceil(K / kDiagThreads)).  part: [chunk][3][K] -- Q, E, C of the chunk's
// words for every topic.
__global__ __launch_bounds__(kDiagThreads) void diagnostics_rows_kernel(int K, int V,
                                                                        const double *__restrict__ lambda,
                                                                        const double *__restrict__ cinv,
                                                                        const double *__restrict__ logR,
                                                                        const double *__restrict__ logp,
                                                                        double *__restrict__ part)
{
    const int k = blockIdx.y * kDiagThreads + threadIdx.x;
    if (k >= K)
        return;
    const int w0 = blockIdx.x * kDiagChunk;
    const int w1 = min(V, w0 + kDiagChunk);
    const double c = cinv[k], lr = logR[k];
    double q = 0.0, e = 0.0, kl = 0.0;
    for (int w = w0; w < w1; ++w) {
        const double l = lambda[(size_t)w * K + k];
        const double beta = l * c;
        const double lb = log(l) - lr;
        q += beta * beta;
        e += beta * lb;
        kl += beta * (lb - logp[w]);
    }
    double *row = part + (size_t)blockIdx.x * 3 * K;
    row[k] = q;
    row[(size_t)K + k] = e;
    row[2 * (size_t)K + k] = kl;
}

// Grid ceil(3 K / 256).  sums[j] = part[0][j] + part[1][j] + ... in ascending chunk order, j over
// the 3 K (sum, topic) pairs.
__global__ __launch_bounds__(kRelevanceThreads) void diagnostics_combine_kernel(int K3, int chunks,
                                                                                const double *__restrict__ part,
                                                                                double *__restrict__ sums)
{
    const int j = blockIdx.x * kRelevanceThreads + threadIdx.x;
    if (j >= K3)
        return;
    double acc = part[j];
#pragma unroll 8                                         // (eight loads in flight; the additions stay in order)
    for (int g = 1; g < chunks; ++g)
        acc += part[(size_t)g * K3 + j];
    sums[j] = acc;
}

// Grid ceil(K n / 4), a wave per listed word: ratio[k * n + r] = beta_kw / u_w, w = words[k * n + r]
// (ids in [0, V): checked on the host).
__global__ __launch_bounds__(kRelevanceThreads) void diagnostics_exclusivity_kernel(int K, int n,
                                                                                    const double *__restrict__ lambda,
                                                                                    const double *__restrict__ cinv,
                                                                                    const int32_t *__restrict__ words,
                                                                                    double *__restrict__ ratio)
{
#pragma clang fp contract(off)                           // (u_w adds rounded products)
    const int lane = threadIdx.x & (kWave - 1);
    const long long item = (long long)blockIdx.x * (kRelevanceThreads / kWave) + threadIdx.x / kWave;
    if (item >= (long long)K * n)
        return;
    const int k = (int)(item / n);
    const double *col = lambda + (size_t)words[item] * K;
    double part = 0.0;
    for (int j = lane; j < K; j += kWave)
        part += col[j] * cinv[j];
    const double u = wave_allsum(part);
    if (lane == 0)
        ratio[item] = (col[k] * cinv[k]) / u;
}

// Grid ceil(K / 256), a thread per topic: the mean of its n ratios, added in rank order.
__global__ __launch_bounds__(kRelevanceThreads) void diagnostics_mean_kernel(int K, int n,
                                                                             const double *__restrict__ ratio,
                                                                             double *__restrict__ excl)
{
    const int k = blockIdx.x * kRelevanceThreads + threadIdx.x;
    if (k >= K)
        return;
    double acc = 0.0;
    for (int r = 0; r < n; ++r)
        acc += ratio[(size_t)k * n + r];
    excl[k] = acc / (double)n;
}

// Grid ceil(B / 4), a wave per document of a batch: nd and inv as prevalence_docs_kernel forms them,
// and top[d] = the smallest k with the largest gamma_dk.  gamma: K x B, K contiguous.
__global__ __launch_bounds__(kRelevanceThreads) void topicdiag_docs_kernel(int K, int B, int by_length,
                                                                           const int32_t *__restrict__ indptr,
                                                                           const int32_t *__restrict__ cnts,
                                                                           const double *__restrict__ gamma,
                                                                           double *__restrict__ nd,
                                                                           double *__restrict__ inv,
                                                                           int32_t *__restrict__ top)
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
    double best = -1.0;                                  // (gamma > 0: any topic beats it)
    int at = 0x7fffffff;
    for (int k = lane; k < K; k += kWave) {
        const double v = g[k];
        part += v;
        if (v > best) {                                  // (ascending k: an equal value keeps the smaller)
            best = v;
            at = k;
        }
    }
    const double s = wave_allsum(part);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(best, off, kWave);
        const int ok = __shfl_xor(at, off, kWave);
        if (ov > best || (ov == best && ok < at)) {
            best = ov;
            at = ok;
        }
    }
    if (lane == 0) {
        nd[d] = n > 0 ? (by_length ? (double)n : 1.0) : 0.0;
        inv[d] = 1.0 / s;
        top[d] = at;
    }
}

// Grid ceil(K / 256), a thread per topic, documents d = 0 .. B - 1 in order, those with nd = 0 left
// out.  sums: T | A, K each; counts: rank_1 | high | low, K each, then the contributing documents
// (thread 0).  The term of T is prevalence_add_kernel's.
__global__ __launch_bounds__(kRelevanceThreads) void topicdiag_add_kernel(int K, int B, double high, double low,
                                                                          const double *__restrict__ gamma,
                                                                          const double *__restrict__ nd,
                                                                          const double *__restrict__ inv,
                                                                          const int32_t *__restrict__ top,
                                                                          double *__restrict__ sums,
                                                                          long long *__restrict__ counts)
{
    const int k = blockIdx.x * kRelevanceThreads + threadIdx.x;
    if (k >= K)
        return;
    double acc = sums[k], ent = sums[(size_t)K + k];
    long long first = counts[k], above = counts[(size_t)K + k], present = counts[2 * (size_t)K + k];
    long long used = 0;
    for (int d = 0; d < B; ++d) {
        const double n = nd[d];
        if (n > 0.0) {
            const double g = gamma[(size_t)d * K + k];
            const double ng = n * g;
            const double a = ng * inv[d];
            const double theta = g * inv[d];
            acc = fma(ng, inv[d], acc);                  // (prevalence_add_kernel's one rounding)
            ent += a > 0.0 ? a * log(a) : 0.0;
            first += top[d] == k ? 1 : 0;
            above += theta > high ? 1 : 0;
            present += theta > low ? 1 : 0;
            ++used;
        }
    }
    sums[k] = acc;
    sums[(size_t)K + k] = ent;
    counts[k] = first;
    counts[(size_t)K + k] = above;
    counts[2 * (size_t)K + k] = present;
    if (k == 0)
        counts[3 * (size_t)K] += used;
}

}  // namespace trlda
