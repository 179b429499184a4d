// trlda_amd/csrc/docindex_kernels.h -- nearest documents in topic space: a device-resident table of
// the documents' topic proportions and the ranked search over it (trlda_docindex_*).
// No reference counterpart.
//
// Rows.  Document d with variational parameter gamma_d (K values) gives the row
//   hellinger:  r_k = sqrt(gamma_k / S),                        S = sum_k gamma_k
//   cosine:     t_k = gamma_k / S,  r_k = t_k / sqrt(T),        T = sum_k t_k^2
// S and T are added in the order of wordtopics_kernels.h: lane l adds elements l, l + 64, ... in that
// order and the 64 lane sums go through wave_sum_dpp.  Division and square root are the IEEE ones,
// t_k^2 is rounded once before it is added (no contraction).  A row therefore depends on its gamma
// column and K alone.  Rows are stored row-major with Kp = ceil(K / 4) * 4 doubles, the tail zero.
//
// Similarities.  s(q, d) = sum_k r_qk r_dk, the staged tile product of tile_product.h: one chain of
// Kp / 4 MFMAs per pair, so s depends on the two rows and K alone.
//
// Ranking.  The total order (s descending, id ascending).  docindex_query_kernel keeps, per query row
// and slab of index rows, the best top_n pairs in LDS; docindex_merge_kernel ranks the slabs' lists.
// The order is total, so neither the slab partition nor the order of arrival shows in the result.
// No atomics.
#pragma once

#include <climits>

#include "tile_product.h"

namespace trlda {

constexpr int kDocIndexThreads = 256;      // 4 waves
constexpr int kDocIndexMaxTop = 100;       // top_n <= min(N, 100): the cap of trlda_model_top_words
constexpr int kDocIndexGroup = 64;         // index rows a workgroup multiplies at a time: 4 tiles of 16
constexpr int kDocIndexSlabRows = 2048;    // default slab: index rows per workgroup
constexpr int kDocIndexWideMaxTop = 32;    // up to here a workgroup takes 128 query rows, beyond 64
constexpr int kDocIndexMeasures = 2;       // 0: hellinger, 1: cosine

// LDS of docindex_query_kernel<SW>: the query chunk, the index chunk, the lists (fp64 s, int32 row)
constexpr size_t docindex_query_lds(int sw, int top_n)
{
    return tile_operands_lds(64 * sw) + (size_t)64 * sw * top_n * (sizeof(double) + sizeof(int));
}

// gamma (K x B column-major) -> rows (B x Kp row-major).  One wave per document.
__global__ __launch_bounds__(kDocIndexThreads) void docindex_rows_kernel(int K, int Kp, int B, int measure,
                                                                         const double *__restrict__ gamma,
                                                                         double *__restrict__ rows)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const long long d = (long long)blockIdx.x * (kDocIndexThreads / kWave) + wid;
    if (d >= B)                                      // (the whole wave)
        return;
    const double *g = gamma + (size_t)d * K;
    double *r = rows + (size_t)d * Kp;
    double a = 0.0;
    for (int k = lane; k < K; k += kWave)
        a += g[k];
    const double S = wave_sum_dpp(a);
    if (measure == 0) {
        for (int k = lane; k < K; k += kWave)
            r[k] = sqrt(g[k] / S);
    } else {
        double b = 0.0;
        for (int k = lane; k < K; k += kWave) {
            const double t = g[k] / S;
            b += t * t;
        }
        const double nrm = sqrt(wave_sum_dpp(b));
        for (int k = lane; k < K; k += kWave)
            r[k] = (g[k] / S) / nrm;
    }
    for (int k = K + lane; k < Kp; k += kWave)
        r[k] = 0.0;
}

// Grid (tile of 64 SW query rows, slab of slab_rows index rows), 4 waves.  Wave w owns the 16 SW
// query rows w * 16 SW ... of the tile -- their products and their lists -- and multiplies them with
// every index row of the slab, 64 at a time: the product, its layout and the selection are those of
// tile_product.h, X the query rows and Y the index rows.  Rows past N and query rows past B are read
// as row N - 1 / B - 1 and kept out of the selection.
// A list holds top_n (s, row in slab) pairs.
// out_s / out_id: (slabs x B x top_n), the pad written as (-inf, int64 max).
template <int SW>
__global__ __launch_bounds__(kDocIndexThreads) void docindex_query_kernel(
    int Kp, long long N, int B, int top_n, int slab_rows, const double *__restrict__ table,
    const double *__restrict__ qrows, double *__restrict__ out_s, long long *__restrict__ out_id)
{
    constexpr int QT = 64 * SW, WQ = 16 * SW, S = kDocIndexStride;
    extern __shared__ __attribute__((aligned(16))) double docindex_lds[];
    double *q_lds = docindex_lds;                           // QT x S
    double *r_lds = q_lds + QT * S;                         // 64 x S
    double *ls = r_lds + kDocIndexGroup * S;                // QT x top_n
    int *li = reinterpret_cast<int *>(ls + QT * top_n);     // QT x top_n
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int m = lane & 15, kq = lane >> 4;
    const int q0 = blockIdx.x * QT;
    const long long slab0 = (long long)blockIdx.y * slab_rows;
    const int nrows = (int)min((long long)slab_rows, N - slab0);

    select_init(ls, li, QT * top_n, tid, kDocIndexThreads);
    // (the first barrier of the loop below stands between this and the lists' first use)

    for (int g0 = 0; g0 < nrows; g0 += kDocIndexGroup) {
        docindex_f64x4 acc[SW][4] = {};

        for (int k0 = 0; k0 < Kp; k0 += kDocIndexChunk) {
            const int cl = min(kDocIndexChunk, Kp - k0);    // a multiple of 4
            __syncthreads();                                // the previous chunk has been read
            tile_stage<QT, kDocIndexThreads>(q_lds, qrows, Kp, k0, cl, tid,
                                             [&](int row) { return min(q0 + row, B - 1); });
            tile_stage<kDocIndexGroup, kDocIndexThreads>(r_lds, table, Kp, k0, cl, tid,
                                                         [&](int row) { return min(slab0 + g0 + row, N - 1); });
            __syncthreads();
            for (int kk = 0; kk < cl; kk += 4)
                tile_step<SW>(acc, q_lds, r_lds, kk, wid, m, kq);
        }

        // the selection: the wave's own query rows against the 64 index rows of this pass
#pragma unroll
        for (int t = 0; t < SW; ++t) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double v = acc[t][j][r];
                    const int ql = wid * WQ + t * 16 + kq + 4 * r;      // query row in the tile
                    const int rl = g0 + j * 16 + m;                     // index row in the slab
                    const double tv = ls[ql * top_n + top_n - 1];
                    const int ti = li[ql * top_n + top_n - 1];
                    const bool pass = rl < nrows && q0 + ql < B && docindex_before(v, rl, tv, ti);
                    select_offer(pass, v, ls, li, top_n, lane,
                                 [&](int L) { return wid * WQ + t * 16 + (L >> 4) + 4 * r; },
                                 [&](int L) { return g0 + j * 16 + (L & 15); });
                }
            }
        }
    }

    // the wave's lists of query rows below B
    const size_t o = ((size_t)blockIdx.y * B + q0 + wid * WQ) * top_n;
    select_write<WQ>(ls + wid * WQ * top_n, li + wid * WQ * top_n, top_n, B - q0 - wid * WQ, out_s + o, out_id + o,
                     slab0, (long long)LLONG_MAX, lane);
}

// One workgroup per query row ranks the slabs' lists: top_n passes, each taking the first candidate
// in the order that lies strictly after the previous pick (ids are distinct, so the order is total
// and the pick unique); the row of ids and the row of s leave as one store each.
__global__ __launch_bounds__(kDocIndexThreads) void docindex_merge_kernel(
    int B, int top_n, int slabs, const double *__restrict__ cand_s, const long long *__restrict__ cand_id,
    long long *__restrict__ ids, double *__restrict__ sims)
{
    constexpr int W = kDocIndexThreads / kWave;
    __shared__ double wave_v[W], pick_v[kDocIndexMaxTop];
    __shared__ long long wave_i[W], pick_i[kDocIndexMaxTop];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int C = slabs * top_n;
    double pv = __builtin_huge_val();
    long long pi = -1;
    for (int r = 0; r < top_n; ++r) {
        double bv = -__builtin_huge_val();
        long long bi = LLONG_MAX;                        // (the pad: nothing lies after it)
        for (int c = tid; c < C; c += kDocIndexThreads) {
            const size_t o = ((size_t)(c / top_n) * B + q) * top_n + c % top_n;
            const double v = cand_s[o];
            const long long i = cand_id[o];
            if (docindex_before(pv, pi, v, i) && docindex_before(v, i, bv, bi)) {
                bv = v;
                bi = i;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(bv, off, kWave);
            const long long oi = __shfl_xor(bi, off, kWave);
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
        ids[(size_t)q * top_n + tid] = pick_i[tid];
        sims[(size_t)q * top_n + tid] = pick_v[tid];
    }
}

}  // namespace trlda
