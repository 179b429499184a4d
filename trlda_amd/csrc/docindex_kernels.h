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
// Similarities.  s(q, d) = sum_k r_qk r_dk, formed by v_mfma_f64_16x16x4_f64: every element of every
// 16 x 16 tile is the same chain of Kp / 4 instructions over k = 0, 4, 8, ..., each adding four
// products to the running value, whatever tile, slab or workgroup the pair lies in.  The zero tail
// adds +0 to a positive sum.  s depends on the two rows and K alone.
//
// Ranking.  The total order (s descending, id ascending).  docindex_query_kernel keeps, per query row
// and slab of index rows, the best top_n pairs in LDS; docindex_merge_kernel ranks the slabs' lists.
// The order is total, so neither the slab partition nor the order of arrival shows in the result.
// No atomics.
#pragma once

#include <climits>

#include "estep_kernels.h"

namespace trlda {

constexpr int kDocIndexThreads = 256;      // 4 waves
constexpr int kDocIndexMaxTop = 100;       // top_n <= min(N, 100): the cap of trlda_model_top_words
constexpr int kDocIndexGroup = 64;         // index rows a workgroup multiplies at a time: 4 tiles of 16
constexpr int kDocIndexChunk = 32;         // the k chunk staged in LDS
// LDS row stride in doubles: 2 mod 4, so the 16 rows x 2 columns that half a wave reads at once fall
// into 32 different 8-byte banks (row * 34 + c mod 32 = 2 row + c, c = 0, 1)
constexpr int kDocIndexStride = kDocIndexChunk + 2;
constexpr int kDocIndexSlabRows = 2048;    // default slab: index rows per workgroup
constexpr int kDocIndexWideMaxTop = 32;    // up to here a workgroup takes 128 query rows, beyond 64
constexpr int kDocIndexMeasures = 2;       // 0: hellinger, 1: cosine

typedef double docindex_f64x4 __attribute__((ext_vector_type(4)));

// LDS of docindex_query_kernel<SW>: the query chunk, the index chunk, the lists (fp64 s, int32 row)
constexpr size_t docindex_query_lds(int sw, int top_n)
{
    return (size_t)(64 * sw + kDocIndexGroup) * kDocIndexStride * sizeof(double) +
           (size_t)64 * sw * top_n * (sizeof(double) + sizeof(int));
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

// is (v, i) before (w, j) in the order (s descending, id ascending)?
template <typename I>
__device__ __forceinline__ bool docindex_before(double v, I i, double w, I j)
{
    return v > w || (v == w && i < j);
}

// Puts (cv, cr) into the wave's own sorted list of n entries (n <= 128; the last entry falls out).
// Every lane calls it with the same arguments; lane l looks after positions l and l + 64.  All reads
// come before all writes: the fences keep the compiler from moving either across.
__device__ __forceinline__ void docindex_insert(double *s, int *id, int n, double cv, int cr, int lane)
{
    const double ninf = -__builtin_huge_val();
    const int p0 = lane, p1 = lane + kWave;
    double e0 = ninf, e1 = ninf, f0 = ninf, f1 = ninf;      // the entries at p and at p - 1
    int i0 = INT_MAX, i1 = INT_MAX, j0 = INT_MAX, j1 = INT_MAX;
    if (p0 < n) {
        e0 = s[p0];
        i0 = id[p0];
        if (p0 > 0) {
            f0 = s[p0 - 1];
            j0 = id[p0 - 1];
        }
    }
    if (p1 < n) {
        e1 = s[p1];
        i1 = id[p1];
        f1 = s[p1 - 1];
        j1 = id[p1 - 1];
    }
    // (the list is sorted: the entries before the candidate are a prefix)
    const int pos = __popcll(__ballot(p0 < n && docindex_before(e0, i0, cv, cr))) +
                    __popcll(__ballot(p1 < n && docindex_before(e1, i1, cv, cr)));
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (p0 < n && p0 >= pos) {
        s[p0] = p0 == pos ? cv : f0;
        id[p0] = p0 == pos ? cr : j0;
    }
    if (p1 < n && p1 >= pos) {
        s[p1] = p1 == pos ? cv : f1;
        id[p1] = p1 == pos ? cr : j1;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Grid (tile of 64 SW query rows, slab of slab_rows index rows), 4 waves.  Wave w owns the 16 SW
// query rows w * 16 SW ... of the tile -- their products and their lists, so no list is shared
// between waves -- and multiplies them with every index row of the slab, 64 at a time.  Both
// operands are staged in LDS in k chunks of 32; the chunks are taken in ascending k for every K, so
// each s is one chain of MFMAs in one order.  Rows past N and query rows past B are read as row
// N - 1 / B - 1 (the product is formed) and kept out of the selection.
//   A operand: lane l holds Q[l & 15][k + (l >> 4)]; B operand: R[l & 15][k + (l >> 4)];
//   D: register r of lane l is s(query (l >> 4) + 4 r, index row l & 15).
// A list holds top_n (s, row in slab) pairs, sorted, filled with (-inf, INT_MAX) at the start: the
// last entry is the threshold a candidate must be before, and most are not.
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
    const double ninf = -__builtin_huge_val();

    for (int i = tid; i < QT * top_n; i += kDocIndexThreads) {
        ls[i] = ninf;
        li[i] = INT_MAX;
    }
    // (the first barrier of the loop below stands between this and the lists' first use)

    for (int g0 = 0; g0 < nrows; g0 += kDocIndexGroup) {
        docindex_f64x4 acc[SW][4];
#pragma unroll
        for (int t = 0; t < SW; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[t][j] = docindex_f64x4{0.0, 0.0, 0.0, 0.0};

        for (int k0 = 0; k0 < Kp; k0 += kDocIndexChunk) {
            const int cl = min(kDocIndexChunk, Kp - k0);    // a multiple of 4
            __syncthreads();                                // the previous chunk has been read
            for (int i = tid; i < QT * (kDocIndexChunk / 2); i += kDocIndexThreads) {
                const int row = i / (kDocIndexChunk / 2), c = (i % (kDocIndexChunk / 2)) * 2;
                if (c < cl) {
                    const int qr = min(q0 + row, B - 1);
                    *reinterpret_cast<double2 *>(q_lds + row * S + c) =
                        *reinterpret_cast<const double2 *>(qrows + (size_t)qr * Kp + k0 + c);
                }
            }
            for (int i = tid; i < kDocIndexGroup * (kDocIndexChunk / 2); i += kDocIndexThreads) {
                const int row = i / (kDocIndexChunk / 2), c = (i % (kDocIndexChunk / 2)) * 2;
                if (c < cl) {
                    const long long rr = min(slab0 + g0 + row, N - 1);
                    *reinterpret_cast<double2 *>(r_lds + row * S + c) =
                        *reinterpret_cast<const double2 *>(table + (size_t)rr * Kp + k0 + c);
                }
            }
            __syncthreads();
            for (int kk = 0; kk < cl; kk += 4) {
                double a[SW], b[4];
#pragma unroll
                for (int t = 0; t < SW; ++t)
                    a[t] = q_lds[(wid * WQ + t * 16 + m) * S + kk + kq];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    b[j] = r_lds[(j * 16 + m) * S + kk + kq];
#pragma unroll
                for (int t = 0; t < SW; ++t)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[t][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b[j], acc[t][j], 0, 0, 0);
            }
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
                    unsigned long long mask = __ballot(pass);
                    while (mask) {                                      // (uniform)
                        const int L = __builtin_ctzll(mask);
                        mask &= mask - 1;
                        const int lo = __builtin_amdgcn_readlane(__double2loint(v), L);
                        const int hi = __builtin_amdgcn_readlane(__double2hiint(v), L);
                        const int cq = wid * WQ + t * 16 + (L >> 4) + 4 * r;
                        docindex_insert(ls + cq * top_n, li + cq * top_n, top_n, __hiloint2double(hi, lo),
                                        g0 + j * 16 + (L & 15), lane);
                    }
                }
            }
        }
    }

    // the wave's lists, each as one run of top_n values
    for (int w = 0; w < WQ; ++w) {
        const int ql = wid * WQ + w;
        if (q0 + ql >= B)
            break;
        const size_t o = ((size_t)blockIdx.y * B + (q0 + ql)) * top_n;
        for (int p = lane; p < top_n; p += kWave) {
            const int id = li[ql * top_n + p];
            out_s[o + p] = ls[ql * top_n + p];
            out_id[o + p] = id == INT_MAX ? LLONG_MAX : slab0 + id;
        }
    }
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
