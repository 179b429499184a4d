// trlda_amd/csrc/cluster_kernels.h -- the document groups of an indexed corpus: spherical k-means on
// the stored rows of a document index, which is Lloyd's algorithm for the index's own measure
// (trlda_docindex_assign, trlda_docindex_cluster).  No reference counterpart.
//
// Both measures store unit-length rows (docindex_kernels.h), so the squared Hellinger distance, like
// the cosine distance, is 1 - <row, row>: a document goes to the centroid row of largest inner
// product, and the centroid that minimises the summed distance of its members is
// (sum of members) / |sum of members|.
//
// Assignment.  s(n, c) = sum_k x_nk m_ck, the staged tile product of tile_product.h: one chain of
// Kp / 4 MFMAs per pair, so s depends on the two rows and K alone.  label(n) is the first c in
// the total order (s descending, c ascending): every lane keeps the running best of its D elements in
// registers and the 16 lanes that share a document row settle it once, at the end.  Nothing of size
// N x C exists.
//
// Update.  The ids are sorted by label with a stable counting sort (integer counts and prefix sums:
// within a cluster the ids ascend); a cluster's members are summed in chunks of kClusterChunkRows in
// that order, the rows of a chunk one after the other, then the chunks of the cluster in ascending
// order; |S|^2 is added as docindex_rows_kernel adds its sums (lane l adds elements l, l + 64, ...,
// then wave_sum_dpp) with every square rounded once.  S_c and m_c = S_c / |S_c| therefore depend on
// the cluster's member set and K alone -- not on the slab, the launch, how the index was filled or
// the other clusters.  No floating-point atomics; the integer ones only count.  A cluster without
// members keeps its row.
#pragma once

#include <climits>

#include "topicdocs_kernels.h"

#define TRLDA_CLUSTER_MAX_CLUSTERS 4096

namespace trlda {

constexpr int kClusterThreads = 256;       // 4 waves
constexpr int kClusterDocTiles = 2;        // tiles of 16 document rows per wave: 128 rows per pass
constexpr int kClusterGroup = 64;          // centroid rows multiplied at a time: 4 tiles of 16
constexpr int kClusterSortRows = 1024;     // ids per block of the counting sort
constexpr int kClusterChunkRows = 256;     // members per partial sum of the update
constexpr int kClusterMaxClusters = TRLDA_CLUSTER_MAX_CLUSTERS;

// LDS of cluster_assign_kernel: the documents' chunk and the centroids' chunk
constexpr size_t cluster_assign_lds()
{
    return tile_operands_lds(64 * kClusterDocTiles);
}

// blocks of the counting sort
inline long long cluster_sort_blocks(long long N) { return (N + kClusterSortRows - 1) / kClusterSortRows; }

// an upper bound of the chunks of any partition of N ids into C clusters: sum_c ceil(n_c / R)
inline long long cluster_max_chunks(long long N, int C) { return N / kClusterChunkRows + C; }

// Grid (slab of slab_rows document rows), 4 waves.  The slab is taken 128 rows at a time: wave w owns
// the 32 rows w * 32 ... of a pass and multiplies them with every centroid row, 64 at a time: the
// product and its layout are those of tile_product.h, X the document rows and Y the centroid rows.
// Rows past N and centroid rows past C are read as row N - 1 / C - 1 and kept out of the selection.
// A lane meets its centroids in ascending order, so its running best is the first in the total order
// among them; the 16 lanes (l & 15) that share a document row compare theirs at the end of the pass.
// label / sim: per document; changed[slab]: the slab's labels that differ from prev (0 without prev).
__global__ __launch_bounds__(kClusterThreads) void cluster_assign_kernel(
    int Kp, long long N, int C, int slab_rows, const double *__restrict__ docs, const double *__restrict__ crows,
    const int *__restrict__ prev, int *__restrict__ label, double *__restrict__ sim, int *__restrict__ changed)
{
    constexpr int SW = kClusterDocTiles, QT = 64 * SW, WQ = 16 * SW, S = kDocIndexStride;
    constexpr int W = kClusterThreads / kWave;
    extern __shared__ __attribute__((aligned(16))) double cluster_lds[];
    __shared__ int wave_diff[W];
    double *x_lds = cluster_lds;                            // QT x S
    double *m_lds = x_lds + QT * S;                         // 64 x S
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int m = lane & 15, kq = lane >> 4;
    const long long slab0 = (long long)blockIdx.x * slab_rows;
    const int nrows = (int)min((long long)slab_rows, N - slab0);
    const double ninf = -__builtin_huge_val();
    int diff = 0;

    for (int q0 = 0; q0 < nrows; q0 += QT) {
        double bs[SW][4];
        int bc[SW][4];
#pragma unroll
        for (int t = 0; t < SW; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                bs[t][r] = ninf;
                bc[t][r] = INT_MAX;
            }

        for (int g0 = 0; g0 < C; g0 += kClusterGroup) {
            docindex_f64x4 acc[SW][4] = {};

            for (int k0 = 0; k0 < Kp; k0 += kDocIndexChunk) {
                const int cl = min(kDocIndexChunk, Kp - k0);    // a multiple of 4
                __syncthreads();                                // the previous chunk has been read
                tile_stage<QT, kClusterThreads>(x_lds, docs, Kp, k0, cl, tid,
                                                [&](int row) { return min(slab0 + q0 + row, N - 1); });
                tile_stage<kClusterGroup, kClusterThreads>(m_lds, crows, Kp, k0, cl, tid,
                                                           [&](int row) { return min(g0 + row, C - 1); });
                __syncthreads();
                for (int kk = 0; kk < cl; kk += 4)
                    tile_step<SW>(acc, x_lds, m_lds, kk, wid, m, kq);
            }

            // the lane's own centroids of this group, in ascending order
#pragma unroll
            for (int t = 0; t < SW; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = g0 + j * 16 + m;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double v = acc[t][j][r];
                        // (the first one is taken whatever it is: a label is always a cluster)
                        if (c < C && (bc[t][r] == INT_MAX || docindex_before(v, c, bs[t][r], bc[t][r]))) {
                            bs[t][r] = v;
                            bc[t][r] = c;
                        }
                    }
                }
        }

        // the 16 lanes of a document row; lane (l & 15) = 0 writes
#pragma unroll
        for (int t = 0; t < SW; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double v = bs[t][r];
                int c = bc[t][r];
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) {
                    const double ov = __shfl_xor(v, off, kWave);
                    const int oc = __shfl_xor(c, off, kWave);
                    if (docindex_before(ov, oc, v, c)) {
                        v = ov;
                        c = oc;
                    }
                }
                const int ql = q0 + wid * WQ + t * 16 + kq + 4 * r;     // document row in the slab
                if (m == 0 && ql < nrows) {
                    const long long d = slab0 + ql;
                    if (prev && prev[d] != c)
                        ++diff;
                    label[d] = c;
                    sim[d] = v;
                }
            }
    }

    // (integers: the order of these additions does not show)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        diff += __shfl_xor(diff, off, kWave);
    if (lane == 0)
        wave_diff[wid] = diff;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < W; ++w)
            total += wave_diff[w];
        changed[blockIdx.x] = total;
    }
}

// total[0] = the sum of the slabs' counts.  One workgroup.
__global__ __launch_bounds__(kClusterThreads) void cluster_changed_kernel(long long slabs,
                                                                          const int *__restrict__ changed,
                                                                          long long *__restrict__ total)
{
    constexpr int W = kClusterThreads / kWave;
    __shared__ long long wave_sum[W];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    long long a = 0;
    for (long long i = tid; i < slabs; i += kClusterThreads)
        a += changed[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        a += __shfl_xor(a, off, kWave);
    if (lane == 0)
        wave_sum[wid] = a;
    __syncthreads();
    if (tid == 0) {
        long long t = 0;
#pragma unroll
        for (int w = 0; w < W; ++w)
            t += wave_sum[w];
        total[0] = t;
    }
}

// The counting sort, first pass.  Grid (block of kClusterSortRows ids): count[c * nb + b] = the ids of
// block b with label c.  LDS: C ints.
__global__ __launch_bounds__(kClusterThreads) void cluster_hist_kernel(long long N, int C, long long nb,
                                                                       const int *__restrict__ label,
                                                                       int *__restrict__ count)
{
    extern __shared__ int cluster_hist[];
    const int tid = threadIdx.x;
    for (int c = tid; c < C; c += kClusterThreads)
        cluster_hist[c] = 0;
    __syncthreads();
    const long long d0 = (long long)blockIdx.x * kClusterSortRows;
    for (int i = tid; i < kClusterSortRows && d0 + i < N; i += kClusterThreads) {
        const int lab = label[d0 + i];
        if ((unsigned)lab < (unsigned)C)
            atomicAdd(&cluster_hist[lab], 1);
    }
    __syncthreads();
    for (int c = tid; c < C; c += kClusterThreads)
        count[(size_t)c * nb + blockIdx.x] = cluster_hist[c];
}

// The counting sort, second pass.  One workgroup: off = the exclusive prefix sums of count in the order
// (cluster, block), so off[c * nb + b] is where block b's ids of cluster c start in the sorted list;
// start[c] / size[c]: the cluster's run; cstart[c]: the chunks of kClusterChunkRows members that lie
// before cluster c's, cstart[C] their number.  Thread t scans a run of consecutive entries.
__global__ __launch_bounds__(kClusterThreads) void cluster_prefix_kernel(long long N, int C, long long nb,
                                                                         const int *__restrict__ count,
                                                                         long long *__restrict__ off,
                                                                         long long *__restrict__ start,
                                                                         long long *__restrict__ size,
                                                                         long long *__restrict__ cstart)
{
    __shared__ long long part[kClusterThreads];
    const int tid = threadIdx.x;
    const size_t total = (size_t)C * nb, per = (total + kClusterThreads - 1) / kClusterThreads;
    const size_t i0 = tid * per < total ? tid * per : total, i1 = i0 + per < total ? i0 + per : total;
    long long a = 0;
    for (size_t i = i0; i < i1; ++i)
        a += count[i];
    part[tid] = a;
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
    a = part[tid];
    for (size_t i = i0; i < i1; ++i) {
        off[i] = a;
        a += count[i];
    }
    __threadfence_block();
    __syncthreads();
    // the clusters' runs and chunks: thread t takes a run of consecutive clusters
    const int cper = (C + kClusterThreads - 1) / kClusterThreads;
    const int c0 = min(C, tid * cper), c1 = min(C, c0 + cper);
    long long chunks = 0;
    for (int c = c0; c < c1; ++c) {
        const long long s0 = off[(size_t)c * nb], s1 = c + 1 < C ? off[(size_t)(c + 1) * nb] : N;
        start[c] = s0;
        size[c] = s1 - s0;
        chunks += (s1 - s0 + kClusterChunkRows - 1) / kClusterChunkRows;
    }
    part[tid] = chunks;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int t = 0; t < kClusterThreads; ++t) {
            const long long v = part[t];
            part[t] = run;
            run += v;
        }
        cstart[C] = run;
    }
    __syncthreads();
    chunks = part[tid];
    for (int c = c0; c < c1; ++c) {
        const long long s0 = off[(size_t)c * nb], s1 = c + 1 < C ? off[(size_t)(c + 1) * nb] : N;
        cstart[c] = chunks;
        chunks += (s1 - s0 + kClusterChunkRows - 1) / kClusterChunkRows;
    }
}

// The counting sort, third pass.  Grid (block of kClusterSortRows ids), ONE wave, which takes its ids
// 64 at a time in ascending order: the lanes that hold one label get consecutive places in lane
// order, so the sort is stable -- within a cluster the ids ascend.  LDS: C running places.
// All reads of a place come before its write: the fences keep the compiler from moving either across.
__global__ __launch_bounds__(kWave) void cluster_scatter_kernel(long long N, int C, long long nb,
                                                                const int *__restrict__ label,
                                                                const long long *__restrict__ off,
                                                                long long *__restrict__ order)
{
    extern __shared__ __attribute__((aligned(8))) long long cluster_place[];
    const int lane = threadIdx.x;
    for (int c = lane; c < C; c += kWave)
        cluster_place[c] = off[(size_t)c * nb + blockIdx.x];
    __syncthreads();
    const long long d0 = (long long)blockIdx.x * kClusterSortRows;
    const unsigned long long below = (1ull << lane) - 1;
    for (int i0 = 0; i0 < kClusterSortRows && d0 + i0 < N; i0 += kWave) {
        const long long d = d0 + i0 + lane;
        const int lab = d < N ? label[d] : -1;
        const bool valid = (unsigned)lab < (unsigned)C;
        unsigned long long todo = __ballot(valid);
        while (todo) {                                      // (uniform)
            const int L = __builtin_ctzll(todo);
            const int cl = __builtin_amdgcn_readlane(lab, L);
            const unsigned long long same = __ballot(valid && lab == cl);
            if (valid && lab == cl)
                order[cluster_place[cl] + __popcll(same & below)] = d;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (lane == L)
                cluster_place[cl] += __popcll(same);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            todo &= ~same;
        }
    }
}

// Grid (chunk of kClusterChunkRows members of one cluster; cluster_max_chunks of them, those past
// cstart[C] leave).  part[chunk * Kp + k] = the sum of the chunk's rows, one after the other in the
// sorted order.  Thread t takes k = t, t + 256, ...: neighbouring threads read neighbouring values.
__global__ __launch_bounds__(kClusterThreads) void cluster_sum_kernel(int Kp, int C,
                                                                      const double *__restrict__ table,
                                                                      const long long *__restrict__ order,
                                                                      const long long *__restrict__ start,
                                                                      const long long *__restrict__ size,
                                                                      const long long *__restrict__ cstart,
                                                                      double *__restrict__ part)
{
#pragma clang fp contract(off)
    const long long chunk = blockIdx.x;
    if (chunk >= cstart[C])                                 // (the whole workgroup)
        return;
    // the cluster of the chunk: the last c with cstart[c] <= chunk (a cluster without members has no
    // chunk: cstart[c] = cstart[c + 1], and the search passes it)
    int lo = 0, hi = C;                                     // cstart[lo] <= chunk < cstart[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (cstart[mid] <= chunk)
            lo = mid;
        else
            hi = mid;
    }
    const long long m0 = start[lo] + (chunk - cstart[lo]) * kClusterChunkRows;
    const long long m1 = min(start[lo] + size[lo], m0 + kClusterChunkRows);
    for (int k = threadIdx.x; k < Kp; k += kClusterThreads) {
        double s = 0.0;
        for (long long i = m0; i < m1; ++i)
            s += table[(size_t)order[i] * Kp + k];
        part[(size_t)chunk * Kp + k] = s;
    }
}

// One wave per cluster with members: S_k = the cluster's chunk sums in ascending order,
// T = sum_k S_k^2 in the order of docindex_rows_kernel's sums, row_k = S_k / sqrt(T).  The tail of
// the row stays zero.  A cluster without members keeps its row.
__global__ __launch_bounds__(kClusterThreads) void cluster_normalise_kernel(int K, int Kp, int C,
                                                                            const long long *__restrict__ size,
                                                                            const long long *__restrict__ cstart,
                                                                            const double *__restrict__ part,
                                                                            double *__restrict__ crows)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const int c = blockIdx.x * (kClusterThreads / kWave) + wid;
    if (c >= C || size[c] == 0)                             // (the whole wave)
        return;
    const long long ch0 = cstart[c], ch1 = cstart[c + 1];
    double *r = crows + (size_t)c * Kp;
    double b = 0.0;
    for (int k = lane; k < K; k += kWave) {
        double s = 0.0;
        for (long long ch = ch0; ch < ch1; ++ch)
            s += part[(size_t)ch * Kp + k];
        r[k] = s;                                           // (read back below by the lane that wrote it)
        b += s * s;
    }
    const double nrm = sqrt(wave_sum_dpp(b));
    for (int k = lane; k < K; k += kWave)
        r[k] = r[k] / nrm;
}

// theta[k + K c] = theta^ of centroid row c, by topicdocs_theta (scale: the rows' sums, cosine only)
__global__ __launch_bounds__(kClusterThreads) void cluster_theta_kernel(int K, int Kp, int C, int measure,
                                                                        const double *__restrict__ crows,
                                                                        const double *__restrict__ scale,
                                                                        double *__restrict__ theta)
{
    const size_t e = (size_t)blockIdx.x * kClusterThreads + threadIdx.x;
    if (e >= (size_t)K * C)
        return;
    const int k = (int)(e % K);
    const long long c = (long long)(e / K);
    theta[e] = topicdocs_theta(crows[(size_t)c * Kp + k], measure, scale, c);
}

}  // namespace trlda
