// trlda_amd/csrc/recommend_kernels.h -- the words a document most likely holds next: p(w | d) for
// every word of the vocabulary, ranked per document, the words it has already seen left out
// (trlda_model_recommend*).  No reference counterpart.
//
// Contract.  Document d with variational parameter gamma_d (K values) and word w:
//   t_dk   = gamma_dk / S_d,  S_d = sum_j gamma_dj   in the order of wordtopics_kernels.h: lane l adds
//                                                    elements l, l + 64, ... and the 64 lane sums go
//                                                    through wave_sum_dpp
//   q_dk   = t_dk / rs_k,     rs_k = sum_v lambda_kv formed from lambda itself (rowsum_partial_kernel,
//                                                    rowsum_combine_wave_kernel)
//   s(d, w) = sum_k q_dk lambda_kw                   the tile product of tile_product.h: one chain
//                                                    of ceil(K / 4) MFMAs over k = 0, 4, 8, ...
// The two divisions are the IEEE ones (no contraction outside the MFMA chain); topics past K add +0.
// s(d, w) is p(w | d) under the point estimates of heldout_kernels.h.  It depends on gamma_d, column
// w of lambda, rs and K alone -- not on the batch, the tile, the slab or the workgroup.
//
// Seen words.  Document d has seen w when it has an entry (w, c) with c > 0 (the rule of
// cooc_bits_kernel): repeated entries count once, c <= 0 does not count.
//
// Ranking.  The total order (s descending, word id ascending) over the words that are not left out;
// per document the first top_n of it, a document with fewer candidates padded with (-1, 0.0).
// recommend_query_kernel keeps, per document and slab of words, the best top_n pairs in LDS;
// recommend_merge_kernel ranks the slabs' lists.  The order is total, so neither the slab partition
// nor the order of arrival shows in the result.  The only atomics are the ORs that set the seen
// bits, which carry no arithmetic and do not depend on their order.
#pragma once

#include <climits>

#include "docindex_kernels.h"

namespace trlda {

constexpr int kRecommendThreads = kDocIndexThreads;    // 4 waves
constexpr int kRecommendMaxTop = 100;                  // top_n <= min(V, 100): the cap of trlda_model_top_words
constexpr int kRecommendSlabWords = 2048;              // default slab: words per workgroup
constexpr int kRecommendWideMaxTop = kDocIndexWideMaxTop;   // up to here 128 documents per workgroup, beyond 64

// LDS of recommend_query_kernel<SW>: the document chunk, the word chunk, the lists (fp64 s, int32 word)
constexpr size_t recommend_query_lds(int sw, int top_n) { return docindex_query_lds(sw, top_n); }

// gamma (K x B column-major) -> q rows (B x Kp row-major, the tail zero).  One wave per document.
__global__ __launch_bounds__(kRecommendThreads) void recommend_rows_kernel(int K, int Kp, int B,
                                                                           const double *__restrict__ gamma,
                                                                           const double *__restrict__ rs,
                                                                           double *__restrict__ rows)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const long long d = (long long)blockIdx.x * (kRecommendThreads / kWave) + wid;
    if (d >= B)                                      // (the whole wave)
        return;
    const double *g = gamma + (size_t)d * K;
    double *r = rows + (size_t)d * Kp;
    double a = 0.0;
    for (int k = lane; k < K; k += kWave)
        a += g[k];
    const double S = wave_sum_dpp(a);
    for (int k = lane; k < K; k += kWave)
        r[k] = (g[k] / S) / rs[k];
    for (int k = K + lane; k < Kp; k += kWave)
        r[k] = 0.0;
}

// One bit per (document, word) into bits (B x nw uint32, nw = ceil(V / 32), zeroed before): a wave
// per document sets the bit of each entry with a count > 0.
__global__ __launch_bounds__(kRecommendThreads) void recommend_seen_kernel(int B, int V, int nw,
                                                                           const int32_t *__restrict__ indptr,
                                                                           const int32_t *__restrict__ ids,
                                                                           const int32_t *__restrict__ cnts,
                                                                           unsigned int *__restrict__ bits)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long d = (long long)blockIdx.x * (kRecommendThreads / kWave) + threadIdx.x / kWave;
    if (d >= B)
        return;
    for (int p = indptr[d] + lane; p < indptr[d + 1]; p += kWave) {
        const int w = ids[p];
        if (cnts[p] <= 0 || w < 0 || w >= V)
            continue;
        atomicOr(bits + (size_t)d * nw + (w >> 5), 1u << (w & 31));
    }
}

// Grid (tile of 64 SW documents, slab of slab_words words), 4 waves: docindex_query_kernel with
// lambda itself as the table.  Wave w owns the 16 SW documents w * 16 SW ... of the tile -- their
// products and their lists -- and multiplies them with every word of the slab, 64 at a time: the
// multiply step, its layout and the selection are those of tile_product.h, X the q rows and Y the
// words, Y[word][k] = lambda[k][word].  The staging is this kernel's own (through registers, a chunk
// ahead: below): the q rows have stride Kp; a word's column of lambda lies where the model keeps it, K
// contiguous doubles with stride K (any alignment of 8 bytes: read one double at a time), and the tail
// of the last chunk is filled with zeros while staging.  Words past V and documents past B are read
// as word V - 1 / document B - 1 and kept out of the selection.
// A list holds top_n (s, word in slab) pairs.  Only a candidate that is before the threshold has
// its seen bit read (seen != nullptr: B x nw uint32), and only an unseen one is inserted.
// out_s / out_id: (slabs x B x top_n), the pad written as (-inf, INT_MAX).
// (two waves per SIMD asked for: the compiler then keeps the accumulators in VGPRs and stays below 256)
template <int SW>
__global__ __launch_bounds__(kRecommendThreads, SW == 1 ? 2 : 1) void recommend_query_kernel(
    int K, int Kp, int V, int B, int top_n, int slab_words, const double *__restrict__ lambda,
    const double *__restrict__ qrows, const unsigned int *__restrict__ seen, int nw,
    double *__restrict__ out_s, int *__restrict__ out_id)
{
    constexpr int QT = 64 * SW, WQ = 16 * SW, S = kDocIndexStride;
    extern __shared__ __attribute__((aligned(16))) double recommend_lds[];
    double *q_lds = recommend_lds;                          // QT x S
    double *r_lds = q_lds + QT * S;                         // 64 x S
    double *ls = r_lds + kDocIndexGroup * S;                // QT x top_n
    int *li = reinterpret_cast<int *>(ls + QT * top_n);     // QT x top_n
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int m = lane & 15, kq = lane >> 4;
    const int q0 = blockIdx.x * QT;
    const int slab0 = blockIdx.y * slab_words;              // (below V: the host's grid)
    const int nwords = min(slab_words, V - slab0);

    select_init(ls, li, QT * top_n, tid, kRecommendThreads);
    // (the first barrier of the loop below stands between this and the lists' first use)

    // The staging of a chunk goes through registers, a chunk ahead: the loads of chunk i + 1 (the
    // next k chunk, or the first one of the next 64 words) are issued before chunk i is multiplied
    // and are in flight meanwhile; with one workgroup per CU nothing else would hide their latency.
    // What a thread holds: NQ double2 of the q rows, NL doubles of lambda.  Columns past the chunk's
    // length are staged as zeros and never read.
    constexpr int NQ = QT * (kDocIndexChunk / 2) / kRecommendThreads;
    constexpr int NL = kDocIndexGroup * kDocIndexChunk / kRecommendThreads;
    double2 qreg[NQ];
    double lreg[NL];
    auto fetch = [&](int g0, int k0) {
        const int cl = min(kDocIndexChunk, Kp - k0);        // a multiple of 4
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            const int i = tid + u * kRecommendThreads;
            const int row = i / (kDocIndexChunk / 2), c = (i % (kDocIndexChunk / 2)) * 2;
            const int qr = min(q0 + row, B - 1);
            qreg[u] = c < cl ? *reinterpret_cast<const double2 *>(qrows + (size_t)qr * Kp + k0 + c)
                             : double2{0.0, 0.0};
        }
#pragma unroll
        for (int u = 0; u < NL; ++u) {
            const int i = tid + u * kRecommendThreads;
            const int row = i / kDocIndexChunk, c = i % kDocIndexChunk;
            const int w = min(slab0 + g0 + row, V - 1);
            lreg[u] = k0 + c < K ? lambda[(size_t)w * K + k0 + c] : 0.0;
        }
    };
    fetch(0, 0);

    for (int g0 = 0; g0 < nwords; g0 += kDocIndexGroup) {
        docindex_f64x4 acc[SW][4] = {};

        for (int k0 = 0; k0 < Kp; k0 += kDocIndexChunk) {
            const int cl = min(kDocIndexChunk, Kp - k0);
            __syncthreads();                                // the previous chunk has been read
#pragma unroll
            for (int u = 0; u < NQ; ++u) {
                const int i = tid + u * kRecommendThreads;
                const int row = i / (kDocIndexChunk / 2), c = (i % (kDocIndexChunk / 2)) * 2;
                *reinterpret_cast<double2 *>(q_lds + row * S + c) = qreg[u];
            }
#pragma unroll
            for (int u = 0; u < NL; ++u) {
                const int i = tid + u * kRecommendThreads;
                r_lds[(i / kDocIndexChunk) * S + i % kDocIndexChunk] = lreg[u];
            }
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

        // the selection: the wave's own documents against the 64 words of this pass
#pragma unroll
        for (int t = 0; t < SW; ++t) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double v = acc[t][j][r];
                    const int ql = wid * WQ + t * 16 + kq + 4 * r;      // document in the tile
                    const int rl = g0 + j * 16 + m;                     // word in the slab
                    const double tv = ls[ql * top_n + top_n - 1];
                    const int ti = li[ql * top_n + top_n - 1];
                    bool pass = rl < nwords && q0 + ql < B && docindex_before(v, rl, tv, ti);
                    if (pass && seen) {                                 // (few get here: one global read)
                        const int w = slab0 + rl;
                        pass = !((seen[(size_t)(q0 + ql) * nw + (w >> 5)] >> (w & 31)) & 1u);
                    }
                    select_offer(pass, v, ls, li, top_n, lane,
                                 [&](int L) { return wid * WQ + t * 16 + (L >> 4) + 4 * r; },
                                 [&](int L) { return g0 + j * 16 + (L & 15); });
                }
            }
        }
    }

    // the wave's lists of documents below B
    const size_t o = ((size_t)blockIdx.y * B + q0 + wid * WQ) * top_n;
    select_write<WQ>(ls + wid * WQ * top_n, li + wid * WQ * top_n, top_n, B - q0 - wid * WQ, out_s + o, out_id + o,
                     slab0, INT_MAX, lane);
}

// One workgroup per document ranks the slabs' lists as docindex_merge_kernel does: top_n passes, each
// taking the first candidate in the order that lies strictly after the previous pick (a word occurs
// in one slab only, so the order is total and the pick unique).  The row of words (int32) and the
// row of s leave as one store each; where the candidates ran out, (-1, 0.0).
__global__ __launch_bounds__(kRecommendThreads) void recommend_merge_kernel(
    int B, int top_n, int slabs, const double *__restrict__ cand_s, const int *__restrict__ cand_id,
    int32_t *__restrict__ words, double *__restrict__ probs)
{
    constexpr int W = kRecommendThreads / kWave;
    __shared__ double wave_v[W], pick_v[kRecommendMaxTop];
    __shared__ int wave_i[W], pick_i[kRecommendMaxTop];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int C = slabs * top_n;
    double pv = __builtin_huge_val();
    int pi = -1;
    for (int r = 0; r < top_n; ++r) {
        double bv = -__builtin_huge_val();
        int bi = INT_MAX;                                // (the pad: nothing lies after it)
        for (int c = tid; c < C; c += kRecommendThreads) {
            const size_t o = ((size_t)(c / top_n) * B + q) * top_n + c % top_n;
            const double v = cand_s[o];
            const int i = cand_id[o];
            if (docindex_before(pv, pi, v, i) && docindex_before(v, i, bv, bi)) {
                bv = v;
                bi = i;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(bv, off, kWave);
            const int oi = __shfl_xor(bi, off, kWave);
            if (docindex_before(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (lane == 0) {
            wave_v[wid] = bv;
            wave_i[wid] = bi;
        }
        __syncthreads();
        bv = wave_v[0];
        bi = wave_i[0];
#pragma unroll
        for (int w = 1; w < W; ++w)
            if (docindex_before(wave_v[w], wave_i[w], bv, bi)) {
                bv = wave_v[w];
                bi = wave_i[w];
            }
        pv = bv;
        pi = bi;
        if (tid == 0) {
            pick_v[r] = bv;
            pick_i[r] = bi;
        }
        __syncthreads();
    }
    if (tid < top_n) {
        const bool pad = pick_i[tid] == INT_MAX;
        words[(size_t)q * top_n + tid] = pad ? -1 : pick_i[tid];
        probs[(size_t)q * top_n + tid] = pad ? 0.0 : pick_v[tid];
    }
}

}  // namespace trlda
