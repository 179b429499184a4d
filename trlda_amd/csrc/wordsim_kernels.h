// trlda_amd/csrc/wordsim_kernels.h -- the words nearest a word in topic space: every word of the
// vocabulary as the distribution p(k | w) over the topics, compared by the two measures of the
// document index and ranked per query word (trlda_model_similar_words*).
// No reference counterpart.
//
// The contract.
//   R_k = sum_v lambda_kv, formed from lambda itself (rowsum_partial_kernel,
//     rowsum_combine_wave_kernel), as in recommend_kernels.h and relevance_kernels.h.
//   Topic weights pi, the rule of relevance_kernels.h: none given, pi_k = R_k / sum_j R_j; a given
//     length-K array must be finite and strictly positive and is normalised to sum 1 on the host in
//     long double.
//   c_k = pi_k / R_k (relevance_coef_kernel),  a_kw = c_k lambda_kw (one rounding),
//   p(k | w) = a_kw / p_w,  p_w = sum_k a_kw.
//   The row of word w:
//     hellinger:  r_wk = sqrt(p(k | w));          s(q, w) = sum_k r_qk r_wk is the Bhattacharyya
//                 coefficient, the distance sqrt(max(0, 1 - s));
//     cosine:     r_wk = a_kw / sqrt(sum_j a_jw^2);  s is the cosine, the distance max(0, 1 - s).
//   Ranking: the total order (s descending, word id ascending) over the candidate words; with
//     exclude_self the query word is left out by its id -- another word with an equal column stays
//     in, at distance 0.
//   A lambda with an element <= 0 or not finite: the column pass raises a device flag, the call
//     fails (TRLDA_ERR_VALUE) and nothing is written to the outputs.
//
// The order of operations.  No V x K table of rows exists: a row is never formed.  Instead
//   t_wk = sqrt(a_kw) (hellinger) or a_kw (cosine)           the staged element: one multiply, and
//                                                            for hellinger one IEEE square root;
//   n_w  = sum_k a_kw (hellinger) or sum_k fl(a_kw^2) (cosine)   lane l adds k = l, l + 64, ... in
//                                                            ascending order, then the butterfly
//                                                            (wave_allsum): the order of
//                                                            relevance_column_kernel;
//   z_w  = 1 / sqrt(n_w)                                     the word's scale: an IEEE square root,
//                                                            then an IEEE division;
//   d(q, w) = sum_k t_qk t_wk                                the tile product of tile_product.h: one
//                                                            chain of ceil(K / 4) MFMAs over k = 0, 4,
//                                                            8, ..., topics past K adding +0;
//   s(q, w) = d(q, w) * (z_q * z_w)                          two multiplies, in the epilogue.
// (sqrt(a / p) = sqrt(a) / sqrt(p) in exact arithmetic: the division leaves the inner loop.)
// No contraction outside the MFMA chain.  s(q, w) depends on columns q and w of lambda, on c and on K
// alone -- not on the batch, the tile, the slab or the workgroup.  The gathered query row
// (wordsim_rows_kernel) and the staged word row (wordsim_query_kernel) apply the identical
// transform, products and the product of the two scales commute, and the MFMA adds the four
// products of a step in an order that does not depend on which operand holds which row: s(q, w) and
// s(w, q) are the same bits.
// A query given as topic proportions (K values, finite and > 0) becomes a unit row through
// docindex_rows_kernel as it is (sqrt(theta_k), or theta_k / |theta|) with scale 1 and no id.
//
// The kernels.  lambda is column-major: a word's K values are contiguous.
//   wordsim_norm_kernel    a wave per word: z_w and the bad-lambda flag; no log, one read;
//   wordsim_rows_kernel    a wave per query word: its t row (B x Kp, the tail zero) and its scale;
//   wordsim_props_kernel   a wave per query word: p(k | w) itself, the sum in the order of the
//                          norm pass (trlda_model_word_topic_proportions);
//   wordsim_query_kernel   recommend_query_kernel with the transform applied while the lambda chunk
//                          goes from registers to LDS and the scales applied before the selection;
//   the merge is recommend_merge_kernel as it is.
// No atomics; every result repeats bitwise.
#pragma once

#include <climits>

#include "recommend_kernels.h"
#include "relevance_kernels.h"

namespace trlda {

constexpr int kWordSimThreads = kDocIndexThreads;      // 4 waves
constexpr int kWordSimMaxTop = kRecommendMaxTop;       // top_n <= min(V - e, 100)
constexpr int kWordSimSlabWords = 2048;                // default slab: words per workgroup
constexpr int kWordSimWideMaxTop = kDocIndexWideMaxTop;    // up to here 128 queries per workgroup, beyond 64

// LDS of wordsim_query_kernel<SW>: docindex_query_kernel's, the 64 word scales of a pass, and the
// tile's query scales and ids
constexpr size_t wordsim_query_lds(int sw, int top_n)
{
    return docindex_query_lds(sw, top_n) + (size_t)(kDocIndexGroup + 64 * sw) * sizeof(double) +
           (size_t)64 * sw * sizeof(int);
}
static_assert(wordsim_query_lds(1, kWordSimMaxTop) <= 160 * 1024, "the lists of top_n = 100 fit in LDS");
static_assert(wordsim_query_lds(2, kWordSimWideMaxTop) <= 160 * 1024, "the wide tile's lists fit in LDS");

// the staged element of a_kw = c_k lambda_kw
__device__ __forceinline__ double wordsim_element(int measure, double c, double l)
{
#pragma clang fp contract(off)
    const double a = c * l;
    return measure == 0 ? sqrt(a) : a;
}

// Grid ceil(V / 4), a wave per word.  scale[w] = 1 / sqrt(sum_k a_kw) (measure 0) or
// 1 / sqrt(sum_k a_kw^2) (measure 1).  *bad is set to 1 by a lambda <= 0 or not finite (every writer
// stores the same value).
__global__ __launch_bounds__(kWordSimThreads) void wordsim_norm_kernel(int K, int V, int measure,
                                                                       const double *__restrict__ lambda,
                                                                       const double *__restrict__ coef,
                                                                       double *__restrict__ scale,
                                                                       int *__restrict__ bad)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    const int w = blockIdx.x * (kWordSimThreads / kWave) + threadIdx.x / kWave;
    if (w >= V)                                          // (the whole wave)
        return;
    const double *col = lambda + (size_t)w * K;
    double part = 0.0;
    bool wrong = false;
    for (int k = lane; k < K; k += kWave) {
        const double l = col[k];
        wrong |= !(l > 0.0) || l > 1.79769313486231570815e+308;
        const double a = coef[k] * l;
        part += measure == 0 ? a : a * a;
    }
    const double n = wave_allsum(part);
    if (wrong)
        *bad = 1;
    if (lane == 0)
        scale[w] = 1.0 / sqrt(n);
}

// Grid ceil(B / 4), a wave per query word: rows (B x Kp row-major) = the t row of word ids[b], the
// tail zero; qscale[b] = scale[ids[b]].  The ids have been checked on the host.
__global__ __launch_bounds__(kWordSimThreads) void wordsim_rows_kernel(int K, int Kp, int B, int measure,
                                                                       const double *__restrict__ lambda,
                                                                       const double *__restrict__ coef,
                                                                       const int32_t *__restrict__ ids,
                                                                       const double *__restrict__ scale,
                                                                       double *__restrict__ rows,
                                                                       double *__restrict__ qscale)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long b = (long long)blockIdx.x * (kWordSimThreads / kWave) + threadIdx.x / kWave;
    if (b >= B)
        return;
    const int w = ids[b];
    const double *col = lambda + (size_t)w * K;
    double *r = rows + (size_t)b * Kp;
    for (int k = lane; k < K; k += kWave)
        r[k] = wordsim_element(measure, coef[k], col[k]);
    for (int k = K + lane; k < Kp; k += kWave)
        r[k] = 0.0;
    if (lane == 0)
        qscale[b] = scale[w];
}

// Grid ceil(B / 4), a wave per query word: out (K x B column-major) = a_kw / p_w, p_w summed in the
// order of wordsim_norm_kernel.
__global__ __launch_bounds__(kWordSimThreads) void wordsim_props_kernel(int K, int B,
                                                                        const double *__restrict__ lambda,
                                                                        const double *__restrict__ coef,
                                                                        const int32_t *__restrict__ ids,
                                                                        double *__restrict__ out)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    const long long b = (long long)blockIdx.x * (kWordSimThreads / kWave) + threadIdx.x / kWave;
    if (b >= B)
        return;
    const double *col = lambda + (size_t)ids[b] * K;
    double part = 0.0;
    for (int k = lane; k < K; k += kWave)
        part += coef[k] * col[k];
    const double p = wave_allsum(part);
    for (int k = lane; k < K; k += kWave)
        out[(size_t)b * K + k] = (coef[k] * col[k]) / p;
}

// Grid (tile of 64 SW queries, slab of slab_words words), 4 waves: recommend_query_kernel's structure
// -- wave w owns the 16 SW queries w * 16 SW ... of the tile, their products and their lists; the
// multiply step, its layout and the selection are those of tile_product.h, X the query rows and Y the
// words' t rows; the staging is this kernel's own, through registers a chunk ahead; words past V and
// queries past B are read as word V - 1 / query B - 1 and kept out of the selection.
// What differs: a thread's 8 lambda values of a chunk share one k (256 threads, 32 columns), so it
// holds that chunk's c_k in one register, and the element is transformed (wordsim_element) on its
// way from the register to LDS; the 64 word scales of a pass are fetched with its first chunk and
// sit in LDS; the tile's query scales (qscale == nullptr: 1) and ids (qid == nullptr: -1, no self)
// sit in LDS from the start.  In the selection the accumulator is scaled once,
// s = d * (z_q * z_w), and a candidate whose word id is the query's own is passed over.
// out_s / out_id: (slabs x B x top_n), the pad written as (-inf, INT_MAX).
// (two waves per SIMD asked for: the accumulators stay in VGPRs, below 256)
template <int SW>
__global__ __launch_bounds__(kWordSimThreads, 2) void wordsim_query_kernel(
    int K, int Kp, int V, int B, int top_n, int slab_words, int measure, const double *__restrict__ lambda,
    const double *__restrict__ coef, const double *__restrict__ scale, const double *__restrict__ qrows,
    const double *__restrict__ qscale, const int32_t *__restrict__ qid, double *__restrict__ out_s,
    int *__restrict__ out_id)
{
#pragma clang fp contract(off)
    constexpr int QT = 64 * SW, WQ = 16 * SW, S = kDocIndexStride;
    extern __shared__ __attribute__((aligned(16))) double wordsim_lds[];
    double *q_lds = wordsim_lds;                            // QT x S
    double *r_lds = q_lds + QT * S;                         // 64 x S
    double *w_scale = r_lds + kDocIndexGroup * S;           // 64
    double *q_scale = w_scale + kDocIndexGroup;             // QT
    double *ls = q_scale + QT;                              // QT x top_n
    int *li = reinterpret_cast<int *>(ls + QT * top_n);     // QT x top_n
    int *q_id = li + QT * top_n;                            // QT
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int m = lane & 15, kq = lane >> 4;
    const int q0 = blockIdx.x * QT;
    const int slab0 = blockIdx.y * slab_words;              // (below V: the host's grid)
    const int nwords = min(slab_words, V - slab0);

    select_init(ls, li, QT * top_n, tid, kWordSimThreads);
    for (int i = tid; i < QT; i += kWordSimThreads) {
        const int qr = min(q0 + i, B - 1);
        q_scale[i] = qscale ? qscale[qr] : 1.0;
        q_id[i] = qid ? qid[qr] : -1;
    }
    // (the first barrier of the loop below stands between this and the first use)

    // Two empty asm statements make the thread's index opaque where the query rows' addresses and
    // the lists' addresses are formed: both are loop invariants, and hoisted out of the k loop they
    // would cost 30 VGPRs beside the accumulators (SW = 2 then spills under 256); they are formed
    // again per chunk and per pass instead, a few VALU instructions under the MFMAs.
    // What a thread holds a chunk ahead: NQ double2 of the query rows, NL doubles of lambda, the
    // c_k of its column, and (the first 64 threads, with a pass's first chunk) a word's scale.
    constexpr int NQ = QT * (kDocIndexChunk / 2) / kWordSimThreads;
    constexpr int NL = kDocIndexGroup * kDocIndexChunk / kWordSimThreads;
    static_assert(kWordSimThreads % kDocIndexChunk == 0, "a thread's lambda values share one column");
    const int lc = tid % kDocIndexChunk;                    // the thread's column of the lambda chunk
    double2 qreg[NQ];
    double lreg[NL];
    double creg = 0.0, sreg = 0.0;
    auto fetch = [&](int g0, int k0) {
        const int cl = min(kDocIndexChunk, Kp - k0);        // a multiple of 4
        int ft = tid;                                       // (opaque: below)
        asm volatile("" : "+v"(ft));
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            const int i = ft + u * kWordSimThreads;
            const int row = i / (kDocIndexChunk / 2), c = (i % (kDocIndexChunk / 2)) * 2;
            const int qr = min(q0 + row, B - 1);
            qreg[u] = c < cl ? *reinterpret_cast<const double2 *>(qrows + (size_t)qr * Kp + k0 + c)
                             : double2{0.0, 0.0};
        }
        const bool in = k0 + lc < K;
        creg = in ? coef[k0 + lc] : 0.0;
#pragma unroll
        for (int u = 0; u < NL; ++u) {
            const int row = (tid + u * kWordSimThreads) / kDocIndexChunk;
            const int w = min(slab0 + g0 + row, V - 1);
            lreg[u] = in ? lambda[(size_t)w * K + k0 + lc] : 0.0;
        }
        if (k0 == 0 && tid < kDocIndexGroup)
            sreg = scale[min(slab0 + g0 + tid, V - 1)];
    };
    fetch(0, 0);

    for (int g0 = 0; g0 < nwords; g0 += kDocIndexGroup) {
        docindex_f64x4 acc[SW][4] = {};

        for (int k0 = 0; k0 < Kp; k0 += kDocIndexChunk) {
            const int cl = min(kDocIndexChunk, Kp - k0);
            __syncthreads();                                // the previous chunk and pass have been read
#pragma unroll
            for (int u = 0; u < NQ; ++u) {
                const int i = tid + u * kWordSimThreads;
                const int row = i / (kDocIndexChunk / 2), c = (i % (kDocIndexChunk / 2)) * 2;
                *reinterpret_cast<double2 *>(q_lds + row * S + c) = qreg[u];
            }
#pragma unroll
            for (int u = 0; u < NL; ++u) {
                const int row = (tid + u * kWordSimThreads) / kDocIndexChunk;
                r_lds[row * S + lc] = wordsim_element(measure, creg, lreg[u]);     // (the tail: c = 0, l = 0)
            }
            if (k0 == 0 && tid < kDocIndexGroup)
                w_scale[tid] = sreg;
            __syncthreads();
            {
                const bool last = k0 + kDocIndexChunk >= Kp;
                const int ng = last ? g0 + kDocIndexGroup : g0, nk = last ? 0 : k0 + kDocIndexChunk;
                if (ng < nwords)                            // (uniform)
                    fetch(ng, nk);
            }
            if (cl == kDocIndexChunk) {                     // (a whole chunk, unrolled: the LDS reads of
#pragma unroll                                              //  a step are issued under the step before)
                for (int kk = 0; kk < kDocIndexChunk; kk += 4)
                    tile_step<SW>(acc, q_lds, r_lds, kk, wid, m, kq);
            } else {
                for (int kk = 0; kk < cl; kk += 4)
                    tile_step<SW>(acc, q_lds, r_lds, kk, wid, m, kq);
            }
        }

        // the selection: the wave's own queries against the 64 words of this pass
        int qw = wid * WQ + kq;                             // (opaque: below)
        asm volatile("" : "+v"(qw));
#pragma unroll
        for (int t = 0; t < SW; ++t) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double zw = w_scale[j * 16 + m];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ql = qw + t * 16 + 4 * r;                 // query in the tile
                    const int rl = g0 + j * 16 + m;                     // word in the slab
                    const double v = acc[t][j][r] * (q_scale[ql] * zw);
                    const double tv = ls[ql * top_n + top_n - 1];
                    const int ti = li[ql * top_n + top_n - 1];
                    const bool pass = rl < nwords && q0 + ql < B && slab0 + rl != q_id[ql] &&
                                      docindex_before(v, rl, tv, ti);
                    select_offer(pass, v, ls, li, top_n, lane,
                                 [&](int L) { return wid * WQ + t * 16 + (L >> 4) + 4 * r; },
                                 [&](int L) { return g0 + j * 16 + (L & 15); });
                }
            }
        }
    }

    // the wave's lists of queries below B
    const size_t o = ((size_t)blockIdx.y * B + q0 + wid * WQ) * top_n;
    select_write<WQ>(ls + wid * WQ * top_n, li + wid * WQ * top_n, top_n, B - q0 - wid * WQ, out_s + o, out_id + o,
                     slab0, INT_MAX, lane);
}

}  // namespace trlda
