// trlda_amd/csrc/silhouette_kernels.h -- the exact silhouette (Rousseeuw 1987) of the documents of an
// index under a labelling, in the index's own distance (trlda_docindex_silhouette).
// No reference counterpart.
//
//   d(i, j)     docindex_distance of s_ij, the dot of the two stored rows by the staged tile product of
//               tile_product.h (one chain of Kp / 4 MFMAs per pair); the pair (i, i) is left out by id
//   a(i)        sum_{j in own, j != i} d(i, j) / (n_own - 1)
//   b(i)        the smallest of sum_{j in c} d(i, j) / n_c over the non-empty c != own; neighbour(i) the
//               first such c in the total order (mean ascending, c ascending)
//   s(i)        (b - a) / max(a, b); 0 where n_own = 1 (with a = 0) or max(a, b) = 0
//
// Columns.  The N ids are sorted by label with the stable counting sort of cluster_kernels.h, under a
// prefix step that starts every non-empty cluster at a multiple of 16 positions: the sequence has
// sum_c ceil(n_c / 16) * 16 <= N + 15 C positions (rounded up to 64 for the sweep), a padding position
// holds id -1, and a tile of 16 positions never holds two clusters.
//
// The order of additions.  Within a cluster the members go by ascending id, rank r; the lane that
// holds column r mod 16 adds d of the ranks r mod 16, r mod 16 + 16, ... in that order from 0.0 (a
// padding position and the row's own id add 0.0, which changes no bit of a sum that is never negative);
// at the cluster's last tile the 16 partial sums of a row go through the xor tree 1, 2, 4, 8.  So
// sum_{j in c} d(i, j) depends on row i, the member set of c and K alone: not on the other clusters,
// on c's number, on the slab setting, on which other rows are scored or on how the index was filled.
// No atomics in floating point (the sort's integer ones only count), nothing of size M x N or M x C.
#pragma once

#include "cluster_kernels.h"

namespace trlda {

constexpr int kSilhouetteThreads = 256;    // 4 waves
constexpr int kSilhouetteRows = 128;       // scored rows per workgroup: 2 tiles of 16 per wave
constexpr int kSilhouetteGroup = 64;       // column positions multiplied at a time: 4 tiles of 16

// the positions of the column sequence of a partition whose padded cluster sizes add up to `padded`
inline long long silhouette_positions(long long padded)
{
    return (padded + kSilhouetteGroup - 1) / kSilhouetteGroup * kSilhouetteGroup;
}

// LDS of silhouette_pairs_kernel: the scored rows' chunk, the columns' chunk, and the ids of both
constexpr size_t silhouette_pairs_lds()
{
    return tile_operands_lds(kSilhouetteRows) + (size_t)(kSilhouetteRows + kSilhouetteGroup) * sizeof(long long);
}

// The counting sort's second pass for the column sequence.  One workgroup; count[c * nb + b] from
// cluster_hist_kernel.  size[c] = n_c; a non-empty cluster starts at the sum of the padded sizes
// ceil(n / 16) * 16 of the clusters before it; off[c * nb + b] is where block b's ids of cluster c
// start (what cluster_scatter_kernel reads); flush[t] = c for the last tile t of cluster c (the caller
// has set every entry to -1).  Thread t takes a run of consecutive clusters.
__global__ __launch_bounds__(kClusterThreads) void silhouette_prefix_kernel(int C, long long nb,
                                                                            const int *__restrict__ count,
                                                                            long long *__restrict__ off,
                                                                            long long *__restrict__ size,
                                                                            int *__restrict__ flush)
{
    __shared__ long long part[kClusterThreads];
    const int tid = threadIdx.x;
    const int cper = (C + kClusterThreads - 1) / kClusterThreads;
    const int c0 = min(C, tid * cper), c1 = min(C, c0 + cper);
    long long padded = 0;
    for (int c = c0; c < c1; ++c) {
        long long n = 0;
        for (long long b = 0; b < nb; ++b)
            n += count[(size_t)c * nb + b];
        size[c] = n;
        padded += (n + 15) / 16 * 16;
    }
    part[tid] = padded;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int t = 0; t < kClusterThreads; ++t) {
            const long long v = part[t];
            part[t] = run;
            run += v;
        }
    }
    __syncthreads();
    long long run = part[tid];
    for (int c = c0; c < c1; ++c) {
        long long a = run;
        for (long long b = 0; b < nb; ++b) {
            off[(size_t)c * nb + b] = a;
            a += count[(size_t)c * nb + b];
        }
        const long long n = a - run;
        if (n > 0) {
            run += (n + 15) / 16 * 16;
            flush[run / 16 - 1] = c;
        }
    }
}

// Grid (block of 128 scored rows), 4 waves: wave w owns the rows 32 w ... 32 w + 31 of the block as
// two MFMA tiles and multiplies them with every column position, 64 at a time in ascending order: the
// product and its layout are those of tile_product.h.  The scored rows (X) are gathered through ids
// (NULL: row q is document q), the columns (Y) through pos (a padding position reads row 0: the product
// is formed and left out).  Rows past M are computed as row M - 1 and not written.
// label[N], size[C]; pos[P] (P a multiple of 64), flush[P / 16]: see silhouette_prefix_kernel.
// sil / a / b / nbr: one per scored row (a, b, nbr may be NULL).
__global__ __launch_bounds__(kSilhouetteThreads) void silhouette_pairs_kernel(
    int Kp, long long M, long long P, int measure, const double *__restrict__ docs,
    const long long *__restrict__ ids, const int *__restrict__ label, const long long *__restrict__ size,
    const long long *__restrict__ pos, const int *__restrict__ flush, double *__restrict__ sil,
    double *__restrict__ a_out, double *__restrict__ b_out, int *__restrict__ nbr_out)
{
#pragma clang fp contract(off)
    constexpr int SW = 2, QT = kSilhouetteRows, WQ = 16 * SW, G = kSilhouetteGroup, S = kDocIndexStride;
    extern __shared__ __attribute__((aligned(16))) double silhouette_lds[];
    double *x_lds = silhouette_lds;                         // QT x S
    double *y_lds = x_lds + QT * S;                         // G x S
    long long *rid_lds = reinterpret_cast<long long *>(y_lds + G * S);     // QT: the scored rows' ids
    long long *cid_lds = rid_lds + QT;                      // G: the group's column ids
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int m = lane & 15, kq = lane >> 4;
    const long long q0 = (long long)blockIdx.x * QT;
    const bool one_chunk = Kp <= kDocIndexChunk;            // the scored rows are staged once

    for (int i = tid; i < QT; i += kSilhouetteThreads) {
        const long long q = min(q0 + i, M - 1);
        rid_lds[i] = ids ? ids[q] : q;
    }
    __syncthreads();

    long long rid[SW][4];
    int own[SW][4], nbr[SW][4];
    double sum[SW][4], a[SW][4], b[SW][4];
#pragma unroll
    for (int t = 0; t < SW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            rid[t][r] = rid_lds[wid * WQ + t * 16 + kq + 4 * r];
            own[t][r] = label[rid[t][r]];
            nbr[t][r] = -1;
            sum[t][r] = 0.0;
            a[t][r] = 0.0;
            b[t][r] = __builtin_huge_val();
        }

    for (long long g0 = 0; g0 < P; g0 += G) {
        docindex_f64x4 acc[SW][4] = {};

        __syncthreads();                                    // the previous group's ids have been read
        if (tid < G)
            cid_lds[tid] = pos[g0 + tid];
        for (int k0 = 0; k0 < Kp; k0 += kDocIndexChunk) {
            const int cl = min(kDocIndexChunk, Kp - k0);    // a multiple of 4
            __syncthreads();                                // the previous chunk has been read
            if (!one_chunk || g0 == 0)
                tile_stage<QT, kSilhouetteThreads>(x_lds, docs, Kp, k0, cl, tid,
                                                   [&](int row) { return rid_lds[row]; });
            tile_stage<G, kSilhouetteThreads>(y_lds, docs, Kp, k0, cl, tid,
                                              [&](int row) { return max(cid_lds[row], 0LL); });
            __syncthreads();
            for (int kk = 0; kk < cl; kk += 4)
                tile_step<SW>(acc, x_lds, y_lds, kk, wid, m, kq);
        }

        // the group's four tiles in ascending order: the distances join the lane's running sums, and
        // the last tile of a cluster settles them (the same for every lane of the workgroup)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long cid = cid_lds[j * 16 + m];
#pragma unroll
            for (int t = 0; t < SW; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double d = docindex_distance(acc[t][j][r], measure);
                    if (cid < 0 || cid == rid[t][r])
                        d = 0.0;
                    sum[t][r] += d;
                }
            const int c = flush[g0 / 16 + j];
            if (c < 0)
                continue;
            const long long n = size[c];
#pragma unroll
            for (int t = 0; t < SW; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double v = sum[t][r];
#pragma unroll
                    for (int off = 1; off < 16; off <<= 1)
                        v += __shfl_xor(v, off, kWave);
                    if (c == own[t][r]) {
                        a[t][r] = n > 1 ? v / (double)(n - 1) : 0.0;
                    } else {
                        const double mean = v / (double)n;
                        // (clusters are met in ascending c: on a tie the smaller one stays)
                        if (mean < b[t][r]) {
                            b[t][r] = mean;
                            nbr[t][r] = c;
                        }
                    }
                    sum[t][r] = 0.0;
                }
        }
    }

    // lane (l & 15) = 0 writes its rows
#pragma unroll
    for (int t = 0; t < SW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long q = q0 + wid * WQ + t * 16 + kq + 4 * r;
            if (m == 0 && q < M) {
                const double top = fmax(a[t][r], b[t][r]);
                sil[q] = size[own[t][r]] > 1 && top > 0.0 ? (b[t][r] - a[t][r]) / top : 0.0;
                if (a_out)
                    a_out[q] = a[t][r];
                if (b_out)
                    b_out[q] = b[t][r];
                if (nbr_out)
                    nbr_out[q] = nbr[t][r];
            }
        }
}

}  // namespace trlda
