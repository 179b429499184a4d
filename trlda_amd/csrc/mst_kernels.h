// trlda_amd/csrc/mst_kernels.h -- the minimum spanning tree of an indexed corpus: the sweep of one round
// of Boruvka's algorithm over the complete graph on the N stored rows (trlda_docindex_mst_sweep,
// DESIGN.md 3.33).  No reference counterpart.
//
//   s(i, j)     the dot of the stored rows i and j by the staged tile product of tile_product.h: one
//               chain of Kp / 4 MFMAs that depends on the two rows and K alone, so s(i, j) and s(j, i)
//               are the same bits -- and the bits neighbors_within and nearest_neighbors see.
//   d(i, j)     docindex_distance(s): sqrt(fmax(1 - s, 0)) (hellinger) or fmax(1 - s, 0) (cosine)
//   w(i, j)     fmax(d, fmax(core[i], core[j])) -- the mutual-reachability distance of HDBSCAN* -- or d
//               itself without core distances.  fmax of the same three numbers: w(i, j) = w(j, i) bitwise.
//   candidate   column j of row i iff j < N, comp[j] != comp[i] and j != i
//   best(i)     the first candidate of row i in the order (w ascending, j ascending); -1 without one
//
// The edge order.  Edges are ordered by (w, min(i, j), max(i, j)), a strict total order because w is
// symmetric bit for bit.  For a fixed i, "smaller j first" among equal w IS that order: of two
// candidates j1 < j2, (min(i, j1), max(i, j1)) comes before (min(i, j2), max(i, j2)) whether both lie
// below i, both above, or i between them.  So best(i) is row i's lightest outgoing edge in the edge
// order, the lightest of a component's rows is the component's, and Boruvka's algorithm, which joins
// every component along its lightest outgoing edge, closes no cycle: a cycle of such choices would
// need an edge strictly lighter than itself.  Mutual reachability makes exact ties in bulk, so this is
// what the tree rests on.
//
// Every lane keeps the running best of its own columns in registers and the 16 lanes that share a row
// settle it once per pass, as cluster_assign_kernel does.  No atomics, no scratch in global memory,
// nothing of size N x N.  best(i) depends on the table, comp, core and K alone -- not on the slab, the
// launch or how the index was filled.
#pragma once

#include "tile_product.h"

namespace trlda {

constexpr int kMstThreads = 256;           // 4 waves
constexpr int kMstDocTiles = 2;            // tiles of 16 rows per wave: 128 rows per pass
constexpr int kMstGroup = 64;              // columns multiplied at a time: 4 tiles of 16

// LDS of mst_sweep_kernel: the rows' chunk and the columns' chunk
constexpr size_t mst_sweep_lds() { return tile_operands_lds(64 * kMstDocTiles); }

// The default slab for N rows: whole passes of 128 rows, one pass per workgroup until that makes more
// than about 1024 workgroups (four per CU), then as many passes as keep the grid there.
inline long long mst_default_slab(long long N)
{
    constexpr long long pass = 64 * kMstDocTiles;
    const long long passes = (N + pass - 1) / pass;
    return (passes + 1023) / 1024 * pass;
}

// is the candidate (w, j) before the running best (bw, bj) in the order (w ascending, j ascending)?
// j < 0: no candidate / no best yet
__device__ __forceinline__ bool mst_before(double w, int j, double bw, int bj)
{
    return j >= 0 && (bj < 0 || w < bw || (w == bw && j < bj));
}

// Grid (slab of slab_rows rows of the table), 4 waves.  The slab is taken 128 rows at a time: wave w
// owns the 32 rows w * 32 ... of a pass and multiplies them with every row of the table, 64 at a time
// in ascending order: the product and its layout are those of tile_product.h, X the slab's rows and
// Y the table.  Rows and columns past N are read as row N - 1 and kept out.  A lane meets its columns
// in ascending j, so a candidate replaces its running best only if strictly lighter; the 16 lanes
// (l & 15) that share a row compare theirs at the end of the pass, and lane (l & 15) = 0 writes
// best_j / best_w (-1 / +inf for a row without a candidate).  core may be NULL.
__global__ __launch_bounds__(kMstThreads) void mst_sweep_kernel(
    int Kp, int N, int slab_rows, int measure, const double *__restrict__ table, const int *__restrict__ comp,
    const double *__restrict__ core, long long *__restrict__ best_j, double *__restrict__ best_w)
{
#pragma clang fp contract(off)
    constexpr int SW = kMstDocTiles, QT = 64 * SW, WQ = 16 * SW, G = kMstGroup, S = kDocIndexStride;
    extern __shared__ __attribute__((aligned(16))) double mst_lds[];
    double *x_lds = mst_lds;                                // QT x S
    double *y_lds = x_lds + QT * S;                         // G x S
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int m = lane & 15, kq = lane >> 4;
    const long long slab0 = (long long)blockIdx.x * slab_rows;
    const int nrows = (int)min((long long)slab_rows, (long long)N - slab0);
    const bool one_chunk = Kp <= kDocIndexChunk;            // the slab's rows are staged once per pass
    const bool with_core = core != nullptr;
    const double inf = __builtin_huge_val();

    for (int q0 = 0; q0 < nrows; q0 += QT) {
        // per (tile, register): the row's id, component and core distance, and its running best
        int self[SW][4], ci[SW][4], bj[SW][4];
        double ri[SW][4], bw[SW][4];
#pragma unroll
        for (int t = 0; t < SW; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = (int)min(slab0 + q0 + wid * WQ + t * 16 + kq + 4 * r, (long long)N - 1);
                self[t][r] = i;
                ci[t][r] = comp[i];
                ri[t][r] = with_core ? core[i] : 0.0;
                bw[t][r] = inf;
                bj[t][r] = -1;
            }

        for (int g0 = 0; g0 < N; g0 += G) {
            // the lane's own columns of this group: their components and core distances
            int cj[4];
            double rj[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = min(g0 + j * 16 + m, N - 1);
                cj[j] = comp[col];
                rj[j] = with_core ? core[col] : 0.0;
            }
            docindex_f64x4 acc[SW][4] = {};

            for (int k0 = 0; k0 < Kp; k0 += kDocIndexChunk) {
                const int cl = min(kDocIndexChunk, Kp - k0);    // a multiple of 4
                __syncthreads();                                // the previous chunk has been read
                if (!one_chunk || g0 == 0)
                    tile_stage<QT, kMstThreads>(x_lds, table, Kp, k0, cl, tid, [&](int row) {
                        return min(slab0 + q0 + row, (long long)N - 1);
                    });
                tile_stage<G, kMstThreads>(y_lds, table, Kp, k0, cl, tid,
                                           [&](int row) { return min(g0 + row, N - 1); });
                __syncthreads();
                for (int kk = 0; kk < cl; kk += 4)
                    tile_step<SW>(acc, x_lds, y_lds, kk, wid, m, kq);
            }

            // the lane's own columns of this group, in ascending order
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = g0 + j * 16 + m;
#pragma unroll
                for (int t = 0; t < SW; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double d = docindex_distance(acc[t][j][r], measure);
                        const double w = with_core ? fmax(d, fmax(ri[t][r], rj[j])) : d;
                        const bool cand = col < N && cj[j] != ci[t][r] && col != self[t][r];
                        if (cand && (bj[t][r] < 0 || w < bw[t][r])) {
                            bw[t][r] = w;
                            bj[t][r] = col;
                        }
                    }
            }
        }

        // the 16 lanes of a row; lane (l & 15) = 0 writes
#pragma unroll
        for (int t = 0; t < SW; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double w = bw[t][r];
                int j = bj[t][r];
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) {
                    const double ow = __shfl_xor(w, off, kWave);
                    const int oj = __shfl_xor(j, off, kWave);
                    if (mst_before(ow, oj, w, j)) {
                        w = ow;
                        j = oj;
                    }
                }
                const int ql = q0 + wid * WQ + t * 16 + kq + 4 * r;     // row in the slab
                if (m == 0 && ql < nrows) {
                    best_j[slab0 + ql] = j;
                    best_w[slab0 + ql] = w;
                }
            }
    }
}

}  // namespace trlda
