// trlda_amd/csrc/neighbors_kernels.h -- the radius join of an index: for every scored row the indexed
// documents within distance `radius` of it, as a CSR list (trlda_docindex_neighbors).
// No reference counterpart.
//
//   s(i, j)     the dot of the scored row i and the stored row j by the staged tile product of
//               tile_product.h: one chain of Kp / 4 MFMAs that depends on the two rows and K alone, so
//               s(i, j) and s(j, i) are the same bits.
//   d(i, j)     docindex_distance(s): sqrt(fmax(1 - s, 0)) (hellinger) or fmax(1 - s, 0) (cosine)
//   hit         d <= radius; the pair (i, i) is left out by id where the scored rows are stored rows
//               (nothing is left out for rows made from a gamma); columns past N are left out by position
//
// The result has no fixed size, so it is made in three steps.  neighbors_count_kernel counts the hits of
// every (scored row, slab of columns); neighbors_scan_kernel turns the counts, in (row, slab) row-major
// order, into the exclusive prefix off[] and the rows' indptr[]; neighbors_fill_kernel forms the same
// products again and puts every hit at off + (the row's hits in earlier tiles of the slab) + (its rank
// among the hits of the tile's 16 columns).  Both passes are neighbors_sweep, so the bits and the counts
// cannot differ.  A row's hits lie in ascending id, and the place of a hit depends on the data alone:
// not on the slab width, on the rows scored beside it or on how the index was filled.  No atomics,
// nothing of size M x N.
#pragma once

#include "docindex_kernels.h"

namespace trlda {

constexpr int kNeighborsThreads = 256;     // 4 waves
constexpr int kNeighborsRows = 128;        // scored rows per workgroup: 2 tiles of 16 per wave
constexpr int kNeighborsGroup = 64;        // columns multiplied at a time: 4 tiles of 16; a slab is a multiple
constexpr int kNeighborsScanThreads = 1024;
constexpr long long kNeighborsMaxSlab = 1LL << 30;      // (a slab's hits of one row are counted in an int)

// LDS of the two sweeps: the scored rows' chunk, the columns' chunk, and the scored rows' source rows
constexpr size_t neighbors_sweep_lds()
{
    return tile_operands_lds(kNeighborsRows) + (size_t)kNeighborsRows * sizeof(long long);
}

// The default slab for M scored rows against N columns: about 1024 workgroups (four per CU) where N
// allows it, so that a few scored rows still fill the chip, and one slab once the row blocks alone do.
inline long long neighbors_default_slab(long long M, long long N)
{
    const long long blocks = (M + kNeighborsRows - 1) / kNeighborsRows;
    const long long want = blocks >= 1024 ? 1 : (1024 + blocks - 1) / blocks;
    const long long slab = (N + want - 1) / want;
    return (slab + kNeighborsGroup - 1) / kNeighborsGroup * kNeighborsGroup;
}

// Grid (block of 128 scored rows, slab of `slab` columns), 4 waves: wave w owns the rows 32 w ...
// 32 w + 31 of the block as two MFMA tiles and multiplies them with the slab's columns, 64 at a time in
// ascending order: the product and its layout are those of tile_product.h.  The scored rows (X) are
// read from xrows through ids (NULL: scored row q is row q of xrows), the columns (Y) from docs by
// position (a column past N reads row N - 1: the product is formed and left out).  Rows past M are
// computed as row M - 1 and left out.
// The 16 lanes 16 (l >> 4) ... 16 (l >> 4) + 15 hold one row's 16 columns of a tile in ascending order:
// the row's hits of the tile are the 16-bit segment (l >> 4) of the wave's ballot, their number its
// popcount, and the rank of lane l's hit the popcount of the segment's bits below l & 15.
//   FILL = false: count[q * nslab + slab] = the hits of row q in the slab.
//   FILL = true:  the hit of rank r of row q in the slab goes to p = off[q * nslab + slab] + r:
//                 ids_out[p] = column, val_out[p] = d or s (val_out may be NULL); only where p < capacity.
template <bool FILL>
__device__ __forceinline__ void neighbors_sweep(int Kp, long long M, long long N, long long slab, int measure,
                                                double radius, int skip_self, int want_similarity,
                                                const double *__restrict__ xrows, const double *__restrict__ docs,
                                                const long long *__restrict__ ids, int *__restrict__ count,
                                                const long long *__restrict__ off, long long capacity,
                                                long long *__restrict__ ids_out, double *__restrict__ val_out)
{
#pragma clang fp contract(off)
    constexpr int SW = 2, QT = kNeighborsRows, WQ = 16 * SW, G = kNeighborsGroup, S = kDocIndexStride;
    extern __shared__ __attribute__((aligned(16))) double neighbors_lds[];
    double *x_lds = neighbors_lds;                          // QT x S
    double *y_lds = x_lds + QT * S;                         // G x S
    long long *src_lds = reinterpret_cast<long long *>(y_lds + G * S);     // QT: the scored rows' rows of xrows
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int m = lane & 15, kq = lane >> 4;
    const long long q0 = (long long)blockIdx.x * QT;
    const long long nslab = gridDim.y;
    const long long c0 = (long long)blockIdx.y * slab, c1 = min(N, c0 + slab);
    const bool one_chunk = Kp <= kDocIndexChunk;            // the scored rows are staged once

    for (int i = tid; i < QT; i += kNeighborsThreads) {
        const long long q = min(q0 + i, M - 1);
        src_lds[i] = ids ? ids[q] : q;
    }
    __syncthreads();

    // per (tile, register): the row's own id (-1: nothing is left out), whether it is a row at all,
    // and the hits so far (FILL: the place of the next hit)
    long long self[SW][4], at[SW][4];
    bool live[SW][4];
    int hits[SW][4];
#pragma unroll
    for (int t = 0; t < SW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = wid * WQ + t * 16 + kq + 4 * r;
            const long long q = q0 + i;
            live[t][r] = q < M;
            self[t][r] = skip_self ? src_lds[i] : -1;
            hits[t][r] = 0;
            at[t][r] = FILL && live[t][r] ? off[q * nslab + blockIdx.y] : 0;
        }

    for (long long g0 = c0; g0 < c1; g0 += G) {
        docindex_f64x4 acc[SW][4] = {};

        for (int k0 = 0; k0 < Kp; k0 += kDocIndexChunk) {
            const int cl = min(kDocIndexChunk, Kp - k0);    // a multiple of 4
            __syncthreads();                                // the previous chunk has been read
            if (!one_chunk || g0 == c0)
                tile_stage<QT, kNeighborsThreads>(x_lds, xrows, Kp, k0, cl, tid,
                                                  [&](int row) { return src_lds[row]; });
            tile_stage<G, kNeighborsThreads>(y_lds, docs, Kp, k0, cl, tid,
                                             [&](int row) { return min(g0 + row, N - 1); });
            __syncthreads();
            for (int kk = 0; kk < cl; kk += 4)
                tile_step<SW>(acc, x_lds, y_lds, kk, wid, m, kq);
        }

        // the group's four tiles in ascending order (every lane of the wave takes every ballot)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long col = g0 + j * 16 + m;
#pragma unroll
            for (int t = 0; t < SW; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double s = acc[t][j][r];
                    const double d = docindex_distance(s, measure);
                    const bool hit = d <= radius && col < c1 && col != self[t][r] && live[t][r];
                    const unsigned seg = (unsigned)(__ballot(hit) >> (16 * kq)) & 0xFFFFu;
                    if (FILL) {
                        const long long p = at[t][r] + __popc(seg & ((1u << m) - 1u));
                        if (hit && p < capacity) {
                            ids_out[p] = col;
                            if (val_out)
                                val_out[p] = want_similarity ? s : d;
                        }
                        at[t][r] += __popc(seg);
                    } else {
                        hits[t][r] += __popc(seg);
                    }
                }
        }
    }

    if (!FILL) {
        // lane (l & 15) = 0 writes its rows
#pragma unroll
        for (int t = 0; t < SW; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long q = q0 + wid * WQ + t * 16 + kq + 4 * r;
                if (m == 0 && q < M)
                    count[q * nslab + blockIdx.y] = hits[t][r];
            }
    }
}

__global__ __launch_bounds__(kNeighborsThreads) void neighbors_count_kernel(
    int Kp, long long M, long long N, long long slab, int measure, double radius, int skip_self,
    const double *__restrict__ xrows, const double *__restrict__ docs, const long long *__restrict__ ids,
    int *__restrict__ count)
{
    neighbors_sweep<false>(Kp, M, N, slab, measure, radius, skip_self, 0, xrows, docs, ids, count, nullptr, 0, nullptr,
                           nullptr);
}

__global__ __launch_bounds__(kNeighborsThreads) void neighbors_fill_kernel(
    int Kp, long long M, long long N, long long slab, int measure, double radius, int skip_self, int want_similarity,
    const double *__restrict__ xrows, const double *__restrict__ docs, const long long *__restrict__ ids,
    const long long *__restrict__ off, long long capacity, long long *__restrict__ ids_out,
    double *__restrict__ val_out)
{
    neighbors_sweep<true>(Kp, M, N, slab, measure, radius, skip_self, want_similarity, xrows, docs, ids, nullptr, off,
                          capacity, ids_out, val_out);
}

// The exclusive prefix of count[M * nslab] in (row, slab) row-major order: off[row * nslab + slab], and
// indptr[row] = off[row * nslab], indptr[M] = the total.  One workgroup; thread t takes a run of
// consecutive rows, thread 0 adds the runs' totals up.  Integers: the result is the same whatever the launch.
__global__ __launch_bounds__(kNeighborsScanThreads) void neighbors_scan_kernel(long long M, long long nslab,
                                                                               const int *__restrict__ count,
                                                                               long long *__restrict__ off,
                                                                               long long *__restrict__ indptr)
{
    __shared__ long long part[kNeighborsScanThreads];
    const int tid = threadIdx.x;
    const long long per = (M + kNeighborsScanThreads - 1) / kNeighborsScanThreads;
    const long long r0 = min(M, tid * per), r1 = min(M, r0 + per);
    long long sum = 0;
    for (long long i = r0 * nslab; i < r1 * nslab; ++i)
        sum += count[i];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int t = 0; t < kNeighborsScanThreads; ++t) {
            const long long v = part[t];
            part[t] = run;
            run += v;
        }
        indptr[M] = run;
    }
    __syncthreads();
    long long run = part[tid];
    for (long long row = r0; row < r1; ++row) {
        indptr[row] = run;
        for (long long b = 0; b < nslab; ++b) {
            off[row * nslab + b] = run;
            run += count[row * nslab + b];
        }
    }
}

}  // namespace trlda
