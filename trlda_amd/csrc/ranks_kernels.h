// trlda_amd/csrc/ranks_kernels.h -- where a document's held-out words stand in the ranking of the whole
// vocabulary that recommend_kernels.h defines: the rank of each, without a sort and without a list
// (trlda_model_heldout_ranks*).  No reference counterpart.
//
// Contract.  s(d, w) is that of recommend_kernels.h, bit for bit: q_dk = (gamma_dk / S_d) / rs_k from
// recommend_rows_kernel unchanged, rs formed from lambda itself (rowsum_partial_kernel,
// rowsum_combine_wave_kernel), and s one chain of ceil(K / 4) v_mfma_f64_16x16x4_f64 in ascending k
// from tile_step of tile_product.h.  With before((v, i), (w, j)) := v > w or (v == w and i < j)
// (docindex_before), a held-out word h of document d has
//   rank(d, h) = 1 + #{ w in [0, V) : w != h, w not seen by d, before((s(d, w), w), (s(d, h), h)) },
// its 1-based position in the list trlda_model_recommend would return for d were top_n unbounded.
// The other held-out words of d are candidates like any word; a seen word (an entry (w, c) of the
// observed document with c > 0: recommend_seen_kernel) is never counted and never ranked.  The rank
// depends on gamma_d, lambda, rs, K and d's seen set alone -- not on B, the other documents, the
// tile, the slab of words, the threshold chunk or the launch -- and two calls agree bitwise.
//
// Entries.  The results are aligned with the entries (h, c) of the held-out batch in its stored order:
// an entry with c <= 0, or whose word the observed document has seen, is no candidate and gets rank 0
// and score 0.0; a word listed twice gets its rank twice.
//
// The count is of integers: a word adds 1 to a histogram in LDS (integer atomics, which cannot depend
// on their order), the slabs' counts are added to the entry's rank with integer atomics, and the seen
// bits are ORed.  No floating-point atomic is used anywhere.
//
// Kernels.
//   ranks_thresholds_kernel  s(d, h) of every held-out entry by a gather product: 64 entries per
//                            workgroup, X row i the q row of entry i's document and Y row i the column
//                            of lambda of entry i's word; the diagonal of the 64 x 64 product is kept.
//                            It marks the entries that are no candidate and starts every rank at 1 / 0.
//   ranks_order_kernel       per document, each chunk of T entries ordered by docindex_before (the
//                            entries that are no candidate first, as (+inf, -1)), and candidates_d =
//                            V - popcount(seen row d).
//   ranks_count_kernel<SW>   the grid and the staged product of recommend_query_kernel; in place of
//                            the selection, per accumulator element a binary search among the
//                            document's ordered thresholds and one histogram increment.
#pragma once

#include <climits>

#include "recommend_kernels.h"

namespace trlda {

constexpr int kRanksThreads = kRecommendThreads;       // 4 waves
constexpr int kRanksChunk = 32;                        // thresholds of a document one sweep holds (the LDS slots)
constexpr int kRanksEntries = 64;                      // entries per workgroup of ranks_thresholds_kernel

// LDS of ranks_count_kernel<SW>: the two operands, and per document kRanksChunk thresholds (fp64 s,
// int32 word) and int32 histogram cells
constexpr size_t ranks_count_lds(int sw)
{
    return tile_operands_lds(64 * sw) + (size_t)64 * sw * kRanksChunk * (sizeof(double) + 2 * sizeof(int));
}

// Grid: ceil(nnz / 64) workgroups of 4 waves.  Entry p = 64 blockIdx.x + i is row i of both operands:
// X row i is the q row of p's document (found in indptr by bisection), Y row i the column of lambda of
// p's word, K contiguous doubles read one at a time as recommend_query_kernel reads them, the tail of
// the last chunk zero.  Wave w multiplies its 16 X rows with the four Y tiles (tile_step) and keeps
// from tile w the diagonal: the element (X row 16 w + kq + 4 r, Y row 16 w + m) with m = kq + 4 r.
// Entries past nnz are read as entry nnz - 1 and not written.
// thr[p]: s, or +inf where p is no candidate; ranks[p]: 1 or 0; scores[p] (unless nullptr): s or 0.0.
__global__ __launch_bounds__(kRanksThreads) void ranks_thresholds_kernel(
    int K, int Kp, int V, int B, int nnz, const int32_t *__restrict__ indptr, const int32_t *__restrict__ ids,
    const int32_t *__restrict__ cnts, const double *__restrict__ lambda, const double *__restrict__ qrows,
    const unsigned int *__restrict__ seen, int nw, double *__restrict__ thr, int32_t *__restrict__ ranks,
    double *__restrict__ scores)
{
    constexpr int S = kDocIndexStride;
    __shared__ __attribute__((aligned(16))) double q_lds[kRanksEntries * S];
    __shared__ __attribute__((aligned(16))) double r_lds[kRanksEntries * S];
    __shared__ int doc_of[kRanksEntries], word_of[kRanksEntries];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int m = lane & 15, kq = lane >> 4;
    const int e0 = blockIdx.x * kRanksEntries;             // (below nnz: the host's grid)

    if (tid < kRanksEntries) {
        const int p = min(e0 + tid, nnz - 1);
        int lo = 0, hi = B;                                 // indptr[lo] <= p < indptr[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (indptr[mid] <= p)
                lo = mid;
            else
                hi = mid;
        }
        doc_of[tid] = lo;
        word_of[tid] = min(max(ids[p], 0), V - 1);
    }

    docindex_f64x4 acc[1][4] = {};
    for (int k0 = 0; k0 < Kp; k0 += kDocIndexChunk) {
        const int cl = min(kDocIndexChunk, Kp - k0);        // a multiple of 4
        __syncthreads();                                    // the rows are known; the previous chunk has been read
        tile_stage<kRanksEntries, kRanksThreads>(q_lds, qrows, Kp, k0, cl, tid, [&](int row) { return doc_of[row]; });
        for (int i = tid; i < kRanksEntries * kDocIndexChunk; i += kRanksThreads) {
            const int row = i / kDocIndexChunk, c = i % kDocIndexChunk;
            if (c < cl)
                r_lds[row * S + c] = k0 + c < K ? lambda[(size_t)word_of[row] * K + k0 + c] : 0.0;
        }
        __syncthreads();
        for (int kk = 0; kk < cl; kk += 4)
            tile_step<1>(acc, q_lds, r_lds, kk, wid, m, kq);
    }

    double v = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (j == wid && r == (m >> 2))
                v = acc[0][j][r];
    const int p = e0 + wid * 16 + m;
    if ((m & 3) == kq && p < nnz) {
        const int w = ids[p];
        bool cand = cnts[p] > 0 && w >= 0 && w < V;
        if (cand && seen)
            cand = !((seen[(size_t)doc_of[wid * 16 + m] * nw + (w >> 5)] >> (w & 31)) & 1u);
        thr[p] = cand ? v : __builtin_huge_val();
        ranks[p] = cand ? 1 : 0;
        if (scores)
            scores[p] = cand ? v : 0.0;
    }
}

// One wave per document.  Each chunk of T <= kRanksChunk consecutive entries of the document is put
// in the order of docindex_before, an entry that is no candidate as (+inf, -1) and so before every
// candidate; equal pairs (a word listed twice) keep their stored order.  sorted_s / sorted_h /
// sorted_p (nnz each): the chunk's pairs and the entries they came from, at the chunk's own
// positions.  candidates[d] = V - popcount(seen row d), V without seen bits.
__global__ __launch_bounds__(kRanksThreads) void ranks_order_kernel(
    int B, int V, int nw, int T, const int32_t *__restrict__ indptr, const int32_t *__restrict__ ids,
    const double *__restrict__ thr, const unsigned int *__restrict__ seen, double *__restrict__ sorted_s,
    int32_t *__restrict__ sorted_h, int32_t *__restrict__ sorted_p, int32_t *__restrict__ candidates)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long d = (long long)blockIdx.x * (kRanksThreads / kWave) + threadIdx.x / kWave;
    if (d >= B)                                             // (the whole wave)
        return;
    int have = 0;
    if (seen)
        for (int i = lane; i < nw; i += kWave)
            have += __popc(seen[(size_t)d * nw + i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        have += __shfl_xor(have, off, kWave);
    if (lane == 0)
        candidates[d] = V - have;
    const int end = indptr[d + 1];
    for (int base = indptr[d]; base < end; base += T) {     // (uniform)
        const int n = min(T, end - base);
        double s = __builtin_huge_val();
        int h = -1;
        if (lane < n) {
            s = thr[base + lane];
            h = s == __builtin_huge_val() ? -1 : ids[base + lane];
        }
        int pos = 0;
        for (int j = 0; j < n; ++j) {
            const double sj = __shfl(s, j, kWave);
            const int hj = __shfl(h, j, kWave);
            pos += docindex_before(sj, hj, s, h) || (sj == s && hj == h && j < lane);
        }
        if (lane < n) {
            sorted_s[base + pos] = s;
            sorted_h[base + pos] = h;
            sorted_p[base + pos] = base + lane;
        }
    }
}

// Grid (tile of 64 SW documents, slab of slab_words words), 4 waves: the staged product of
// recommend_query_kernel -- the same operands, the same layout, the same register-prefetched staging
// a chunk ahead (one workgroup per CU: nothing else would hide the loads' latency), the same chains
// of tile_step -- with a counting epilogue.  Sweep `chunk` holds, per document d of the tile, the
// ordered thresholds of its entries indptr[d] + chunk T ... (at most T of them) at the END of the
// document's kRanksChunk LDS slots; the slots before them hold (+inf, -1), which no word is before.
// In that order "word (v, w) is before slot i, and w is not slot i's word" is false up to some slot
// and true from it on.  Per accumulator element: slot 31 first (most words that are before no
// threshold end here), then a bisection to the first slot the word is before, then the seen bit
// (seen != nullptr: one global read), then one integer add to that slot's histogram cell.
// At the end slot i's count is the sum of the cells 0 ... i; it is added to the entry's rank.
// A tile whose documents have no candidate entry in this sweep returns before any product.
template <int SW>
__global__ __launch_bounds__(kRanksThreads, 1) void ranks_count_kernel(
    int K, int Kp, int V, int B, int T, int chunk, int slab_words, const double *__restrict__ lambda,
    const double *__restrict__ qrows, const unsigned int *__restrict__ seen, int nw,
    const int32_t *__restrict__ indptr, const double *__restrict__ sorted_s, const int32_t *__restrict__ sorted_h,
    const int32_t *__restrict__ sorted_p, int32_t *__restrict__ ranks)
{
    constexpr int QT = 64 * SW, WQ = 16 * SW, S = kDocIndexStride, C = kRanksChunk;
    extern __shared__ __attribute__((aligned(16))) double ranks_lds[];
    __shared__ int live;
    double *q_lds = ranks_lds;                              // QT x S
    double *r_lds = q_lds + QT * S;                         // 64 x S
    double *ts = r_lds + kDocIndexGroup * S;                // QT x C
    int *th = reinterpret_cast<int *>(ts + QT * C);         // QT x C
    int *hist = th + QT * C;                                // QT x C
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int m = lane & 15, kq = lane >> 4;
    const int q0 = blockIdx.x * QT;
    const int slab0 = blockIdx.y * slab_words;              // (below V: the host's grid)
    const int nwords = min(slab_words, V - slab0);

    if (tid == 0)
        live = 0;
    __syncthreads();
    for (int i = tid; i < QT * C; i += kRanksThreads) {
        const int ql = i / C, slot = i % C;
        double s = __builtin_huge_val();
        int h = -1;
        if (q0 + ql < B) {
            const int base = indptr[q0 + ql] + chunk * T;
            const int n = max(0, min(T, indptr[q0 + ql + 1] - base));
            if (slot >= C - n) {
                s = sorted_s[base + slot - (C - n)];
                h = sorted_h[base + slot - (C - n)];
            }
        }
        ts[i] = s;
        th[i] = h;
        hist[i] = 0;
        if (h >= 0)
            live = 1;
    }
    __syncthreads();
    if (!live)                                              // (uniform)
        return;

    // the staging of recommend_query_kernel: through registers, a chunk ahead
    constexpr int NQ = QT * (kDocIndexChunk / 2) / kRanksThreads;
    constexpr int NL = kDocIndexGroup * kDocIndexChunk / kRanksThreads;
    double2 qreg[NQ];
    double lreg[NL];
    auto fetch = [&](int g0, int k0) {
        const int cl = min(kDocIndexChunk, Kp - k0);        // a multiple of 4
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            const int i = tid + u * kRanksThreads;
            const int row = i / (kDocIndexChunk / 2), c = (i % (kDocIndexChunk / 2)) * 2;
            const int qr = min(q0 + row, B - 1);
            qreg[u] = c < cl ? *reinterpret_cast<const double2 *>(qrows + (size_t)qr * Kp + k0 + c)
                             : double2{0.0, 0.0};
        }
#pragma unroll
        for (int u = 0; u < NL; ++u) {
            const int i = tid + u * kRanksThreads;
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
                const int i = tid + u * kRanksThreads;
                const int row = i / (kDocIndexChunk / 2), c = (i % (kDocIndexChunk / 2)) * 2;
                *reinterpret_cast<double2 *>(q_lds + row * S + c) = qreg[u];
            }
#pragma unroll
            for (int u = 0; u < NL; ++u) {
                const int i = tid + u * kRanksThreads;
                r_lds[(i / kDocIndexChunk) * S + i % kDocIndexChunk] = lreg[u];
            }
            __syncthreads();
            {
                const bool last = k0 + kDocIndexChunk >= Kp;
                const int ng = last ? g0 + kDocIndexGroup : g0, nk = last ? 0 : k0 + kDocIndexChunk;
                if (ng < nwords)                            // (uniform)
                    fetch(ng, nk);
            }
            if (cl == kDocIndexChunk) {
#pragma unroll
                for (int kk = 0; kk < kDocIndexChunk; kk += 4)
                    tile_step<SW>(acc, q_lds, r_lds, kk, wid, m, kq);
            } else {
                for (int kk = 0; kk < cl; kk += 4)
                    tile_step<SW>(acc, q_lds, r_lds, kk, wid, m, kq);
            }
        }

        // the count: the wave's own documents against the 64 words of this pass
#pragma unroll
        for (int t = 0; t < SW; ++t) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double v = acc[t][j][r];
                    const int ql = wid * WQ + t * 16 + kq + 4 * r;      // document in the tile
                    const int rl = g0 + j * 16 + m;                     // word in the slab
                    const int w = slab0 + rl;
                    const double *s_of = ts + ql * C;
                    const int *h_of = th + ql * C;
                    auto hit = [&](int slot) {
                        const int h = h_of[slot];
                        return w != h && docindex_before(v, w, s_of[slot], h);
                    };
                    if (!(rl < nwords && q0 + ql < B && hit(C - 1)))
                        continue;
                    int pos = 0;                                        // the first slot that is hit
#pragma unroll
                    for (int step = C / 2; step > 0; step >>= 1)
                        if (!hit(pos + step - 1))
                            pos += step;
                    if (seen && ((seen[(size_t)(q0 + ql) * nw + (w >> 5)] >> (w & 31)) & 1u))
                        continue;
                    atomicAdd(hist + ql * C + pos, 1);
                }
            }
        }
    }

    __syncthreads();
    for (int i = tid; i < QT * C; i += kRanksThreads) {
        const int ql = i / C, slot = i % C;
        if (q0 + ql >= B)
            continue;
        const int base = indptr[q0 + ql] + chunk * T;
        const int n = max(0, min(T, indptr[q0 + ql + 1] - base));
        if (slot < C - n)
            continue;
        int count = 0;
        for (int j = C - n; j <= slot; ++j)
            count += hist[ql * C + j];
        if (count > 0)
            atomicAdd(ranks + sorted_p[base + slot - (C - n)], count);
    }
}

}  // namespace trlda
