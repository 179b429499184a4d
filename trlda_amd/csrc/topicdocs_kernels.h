// trlda_amd/csrc/topicdocs_kernels.h -- topic summaries of an indexed corpus: per topic the documents
// that hold most of it, and the mean and the centred scatter of the documents' topic proportions
// (trlda_docindex_topic_documents, trlda_docindex_topic_moments).  No reference
// counterpart.
//
// theta^.  The index stores a row r per document (docindex_kernels.h); theta is recovered from it as
//   hellinger:  theta^_k = r_k * r_k            (one IEEE multiply, never contracted)
//   cosine:     theta^_k = r_k / sum_j r_j      (IEEE division; the sum as docindex_rows_kernel adds
//               sum gamma: lane l adds elements l, l + 64, ... in that order, then wave_sum_dpp)
// theta^ depends on the row and K alone, and every kernel here forms it by topicdocs_theta.
//
// Selection.  Per topic the total order (theta^ descending, id ascending).  topicdocs_select_kernel
// keeps, per topic and slab of index rows, the best top_n pairs in LDS; docindex_merge_kernel ranks
// the slabs' lists with one workgroup per topic (the lists have the layout of a query's, B = K).  The
// order is total, so the slab partition does not show in the result.
//
// Order of additions.  Nothing here is atomic and nothing depends on launch order.
//   mean     blocks of kTopicDocsMeanRows rows, the rows of a block in ascending order, then the blocks
//            in ascending order, then one division by N: a function of (K, N)
//   scatter  N is cut into chunks of `cr` rows (topicdocs_chunk_rows: a function of K, N); within a
//            chunk every element is one chain of v_mfma_f64_16x16x4_f64 over ascending rows, four at a
//            time; the chunks' partial sums are added in ascending order
// Only the tiles (ti <= tj) of the scatter are formed; element (i, j) with i > j is read from (j, i),
// so the matrix is bitwise symmetric.
#pragma once

#include <climits>

#include "docindex_kernels.h"

namespace trlda {

constexpr int kTopicDocsThreads = 256;     // 4 waves
constexpr int kTopicDocsSelTopics = 32;    // topics per workgroup of the selection: 8 lists per wave
constexpr int kTopicDocsSelRows = 64;      // index rows staged at a time: one per lane
// LDS row stride of the selection's tile in doubles: odd, so the 64 lanes that read one topic of 64
// rows fall into different banks
constexpr int kTopicDocsSelStride = kTopicDocsSelTopics + 1;
constexpr int kTopicDocsMeanRows = 256;    // rows per workgroup of the mean
constexpr int kTopicDocsTile = 64;         // a workgroup's tile of the scatter: 64 x 64 topics
constexpr int kTopicDocsStage = 32;        // index rows staged in LDS at a time
// LDS row (one document's 64 topics) stride in doubles: 16 mod 32.  Half a wave reads 2 rows x 16
// topics of an operand at once, (d + h) * 80 + t0 + m with h = 0, 1 and m = 0 .. 15: the 32 different
// 8-byte banks (80 mod 32 = 16)
constexpr int kTopicDocsStride = kTopicDocsTile + 16;
constexpr int kTopicDocsTargetGroups = 1024;   // workgroups the chunking aims at
constexpr int kTopicDocsMinChunk = 64;         // ... without cutting N finer than this

typedef double topicdocs_f64x4 __attribute__((ext_vector_type(4)));

// LDS of topicdocs_select_kernel: the tile, the lists (fp64 theta^, int32 row in slab)
constexpr size_t topicdocs_select_lds(int top_n)
{
    return (size_t)kTopicDocsSelRows * kTopicDocsSelStride * sizeof(double) +
           (size_t)kTopicDocsSelTopics * top_n * (sizeof(double) + sizeof(int));
}

// Tiles (ti <= tj) of a T x T grid of tiles
inline long long topicdocs_tile_pairs(int K)
{
    const long long T = (K + kTopicDocsTile - 1) / kTopicDocsTile;
    return T * (T + 1) / 2;
}

// Rows per chunk of N: a multiple of the staging size, chosen so that tiles x chunks is about
// kTopicDocsTargetGroups.  K = 500, N = 200 000: 36 tiles, 28 chunks of 7168 rows, 56 MB of partial
// sums; K = 100, N = 1 000 000: 3 tiles, 341 chunks of 2944 rows, 27 MB.  A function of (K, N) alone.
inline long long topicdocs_chunk_rows(int K, long long N)
{
    long long chunks = kTopicDocsTargetGroups / topicdocs_tile_pairs(K);
    if (chunks < 1)
        chunks = 1;
    long long cr = (N + chunks - 1) / chunks;
    if (cr < kTopicDocsMinChunk)
        cr = kTopicDocsMinChunk;
    return (cr + kTopicDocsStage - 1) / kTopicDocsStage * kTopicDocsStage;
}

// theta^ of the stored value r of row d (scale: the rows' sums, cosine only)
__device__ __forceinline__ double topicdocs_theta(double r, int measure, const double *__restrict__ scale,
                                                  long long d)
{
#pragma clang fp contract(off)
    return measure == 0 ? r * r : r / scale[d];
}

// scale[d] = sum_k r_dk in the order of docindex_rows_kernel's sum of gamma.  One wave per row.
__global__ __launch_bounds__(kTopicDocsThreads) void topicdocs_scale_kernel(int K, int Kp, long long N,
                                                                            const double *__restrict__ table,
                                                                            double *__restrict__ scale)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const long long d = (long long)blockIdx.x * (kTopicDocsThreads / kWave) + wid;
    if (d >= N)                                      // (the whole wave)
        return;
    const double *r = table + (size_t)d * Kp;
    double a = 0.0;
    for (int k = lane; k < K; k += kWave)
        a += r[k];
    const double S = wave_sum_dpp(a);
    if (lane == 0)
        scale[d] = S;
}

// Grid (slab of slab_rows index rows, tile of 32 topics), 4 waves.  64 rows x 32 topics of theta^ are
// staged in LDS at a time; wave w owns topics w * 8 ... of the tile -- their lists, so no list is
// shared between waves -- and lane l looks at row l of the staged rows.  A list holds top_n
// (theta^, row in slab) pairs, sorted, filled with (-inf, INT_MAX) at the start: the last entry is
// the threshold a candidate must be before, and most are not.  Rows past N are staged as zeros and
// kept out of the selection; topics past K are neither read, ranked nor written.
// out_v / out_id: (slabs x K x top_n), the pad written as (-inf, int64 max).
__global__ __launch_bounds__(kTopicDocsThreads) void topicdocs_select_kernel(
    int K, int Kp, long long N, int measure, int top_n, int slab_rows, const double *__restrict__ table,
    const double *__restrict__ scale, double *__restrict__ out_v, long long *__restrict__ out_id)
{
#pragma clang fp contract(off)
    constexpr int TT = kTopicDocsSelTopics, R = kTopicDocsSelRows, S = kTopicDocsSelStride;
    constexpr int WT = TT / (kTopicDocsThreads / kWave);    // topics per wave
    extern __shared__ __attribute__((aligned(16))) double topicdocs_lds[];
    double *tile = topicdocs_lds;                           // R x S
    double *ls = tile + R * S;                              // TT x top_n
    int *li = reinterpret_cast<int *>(ls + TT * top_n);     // TT x top_n
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const long long slab0 = (long long)blockIdx.x * slab_rows;
    const int nrows = (int)min((long long)slab_rows, N - slab0);
    const int k0 = blockIdx.y * TT;
    const int st = tid & (TT - 1), sr = tid / TT;           // staging: topic, first row
    const bool k_in = k0 + st < K;
    const double ninf = -__builtin_huge_val();

    for (int i = tid; i < TT * top_n; i += kTopicDocsThreads) {
        ls[i] = ninf;
        li[i] = INT_MAX;
    }
    // (the first barrier of the loop below stands between this and the lists' first use)

    for (int g0 = 0; g0 < nrows; g0 += R) {
        __syncthreads();                                    // the previous rows have been read
#pragma unroll
        for (int e = 0; e < R * TT / kTopicDocsThreads; ++e) {
            const int row = sr + e * (kTopicDocsThreads / TT);
            double x = 0.0;
            if (k_in && g0 + row < nrows) {
                const long long d = slab0 + g0 + row;
                x = topicdocs_theta(table[(size_t)d * Kp + k0 + st], measure, scale, d);
            }
            tile[row * S + st] = x;
        }
        __syncthreads();
#pragma unroll 1
        for (int t = 0; t < WT; ++t) {
            const int tl = wid * WT + t;
            if (k0 + tl >= K)                               // (the whole wave)
                break;
            const double v = tile[lane * S + tl];
            const int rl = g0 + lane;                       // index row in the slab
            const double tv = ls[tl * top_n + top_n - 1];
            const int ti = li[tl * top_n + top_n - 1];
            unsigned long long mask = __ballot(rl < nrows && docindex_before(v, rl, tv, ti));
            while (mask) {                                  // (uniform)
                const int L = __builtin_ctzll(mask);
                mask &= mask - 1;
                const int lo = __builtin_amdgcn_readlane(__double2loint(v), L);
                const int hi = __builtin_amdgcn_readlane(__double2hiint(v), L);
                docindex_insert(ls + tl * top_n, li + tl * top_n, top_n, __hiloint2double(hi, lo), g0 + L, lane);
            }
        }
    }

    // the wave's lists, each as one run of top_n values
    for (int t = 0; t < WT; ++t) {
        const int tl = wid * WT + t;
        if (k0 + tl >= K)
            break;
        const size_t o = ((size_t)blockIdx.x * K + (k0 + tl)) * top_n;
        for (int p = lane; p < top_n; p += kWave) {
            const int id = li[tl * top_n + p];
            out_v[o + p] = ls[tl * top_n + p];
            out_id[o + p] = id == INT_MAX ? LLONG_MAX : slab0 + id;
        }
    }
}

// part[block * K + k] = sum of theta^_dk over the block's rows, ascending.  Thread t takes topics
// t, t + 256, ...: neighbouring threads read neighbouring values.
__global__ __launch_bounds__(kTopicDocsThreads) void topicdocs_mean_kernel(int K, int Kp, long long N, int measure,
                                                                           const double *__restrict__ table,
                                                                           const double *__restrict__ scale,
                                                                           double *__restrict__ part)
{
#pragma clang fp contract(off)
    const long long d0 = (long long)blockIdx.x * kTopicDocsMeanRows, d1 = min(N, d0 + kTopicDocsMeanRows);
    for (int k = threadIdx.x; k < K; k += kTopicDocsThreads) {
        double s = 0.0;
        for (long long d = d0; d < d1; ++d)
            s += topicdocs_theta(table[(size_t)d * Kp + k], measure, scale, d);
        part[(size_t)blockIdx.x * K + k] = s;
    }
}

// mean[k] = (the blocks' partial sums added in ascending block order) / N
__global__ __launch_bounds__(kTopicDocsThreads) void topicdocs_mean_sum_kernel(int K, long long blocks, double n,
                                                                               const double *__restrict__ part,
                                                                               double *__restrict__ mean)
{
#pragma clang fp contract(off)
    const int k = blockIdx.x * kTopicDocsThreads + threadIdx.x;
    if (k >= K)
        return;
    double a = 0.0;
    for (long long b = 0; b < blocks; ++b)
        a += part[(size_t)b * K + k];
    mean[k] = a / n;
}

// Grid (tile pair (ti <= tj) of 64 x 64 topics, chunk of cr rows), 4 waves; wave w owns the 32 x 32
// block (w & 1, w >> 1) of the tile as 2 x 2 MFMA tiles.  32 index rows are staged in LDS at a time
// as [row][topic], transformed while staged: theta^ from r, then - mean.  A row's topics are
// contiguous in memory and in LDS, so the reads are coalesced and nothing is transposed.  Topics past
// K and rows past the chunk's or the table's end are staged as exact zeros (after the centring: not
// as -mean) and are neither read from memory nor written out.  A diagonal tile stages one operand.
//   first operand:  lane l holds B[topic l & 15][row kk + (l >> 4)] (tile tj), second: A likewise
//   (tile ti); D: register r of lane l is (tj topic (l >> 4) + 4 r, ti topic l & 15).
// part[(chunk * K + j) * K + i], i in tile ti, j in tile tj.
__global__ __launch_bounds__(kTopicDocsThreads) void topicdocs_scatter_kernel(
    int K, int Kp, long long N, long long cr, int measure, const double *__restrict__ table,
    const double *__restrict__ scale, const double *__restrict__ mean, double *__restrict__ part)
{
#pragma clang fp contract(off)
    constexpr int S = kTopicDocsStride, T = kTopicDocsTile, W = kTopicDocsStage;
    __shared__ __attribute__((aligned(16))) double a_lds[W * S], b_lds[W * S];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int m = lane & 15, kq = lane >> 4;
    const int wi = (wid & 1) * 32, wj = (wid >> 1) * 32;
    // the pair (ti <= tj) of blockIdx.x: column tj holds the tj + 1 pairs from tj (tj + 1) / 2 on
    int tj = 0, ti = blockIdx.x;
    while (ti > tj) {
        ++tj;
        ti -= tj;
    }
    const bool diag = ti == tj;
    const int i0 = ti * T, j0 = tj * T;
    const long long dbeg = (long long)blockIdx.y * cr, dend = min(N, dbeg + cr);
    const int st = tid & (T - 1), sw = tid / T;                     // staging: topic, first row
    const bool a_in = i0 + st < K, b_in = !diag && j0 + st < K;
    const double ma = a_in ? mean[i0 + st] : 0.0, mb = b_in ? mean[j0 + st] : 0.0;
    const double *ap = table + (a_in ? i0 + st : 0), *bp = table + (b_in ? j0 + st : 0);
    const double *b_src = diag ? a_lds : b_lds;

    topicdocs_f64x4 acc[2][2];
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
            acc[ta][tb] = topicdocs_f64x4{0.0, 0.0, 0.0, 0.0};

    for (long long d0 = dbeg; d0 < dend; d0 += W) {
        __syncthreads();                                            // the previous rows have been read
#pragma unroll
        for (int e = 0; e < W * T / kTopicDocsThreads; ++e) {
            const int w = sw + e * (kTopicDocsThreads / T);
            const long long d = d0 + w;
            double x = 0.0, y = 0.0;
            if (d < dend) {
                if (a_in)
                    x = topicdocs_theta(ap[(size_t)d * Kp], measure, scale, d) - ma;
                if (b_in)
                    y = topicdocs_theta(bp[(size_t)d * Kp], measure, scale, d) - mb;
            }
            a_lds[w * S + st] = x;
            if (!diag)
                b_lds[w * S + st] = y;
        }
        __syncthreads();
        const int steps = ((int)min((long long)W, dend - d0) + 3) / 4;   // (the rows past the end are zeros)
        for (int s = 0; s < steps; ++s) {
            const int row = (s * 4 + kq) * S;
            double a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = a_lds[row + wi + t * 16 + m];
                b[t] = b_src[row + wj + t * 16 + m];
            }
#pragma unroll
            for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                for (int tb = 0; tb < 2; ++tb)
                    acc[ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(b[tb], a[ta], acc[ta][tb], 0, 0, 0);
        }
    }

    double *o = part + (size_t)blockIdx.y * K * K;
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + wi + ta * 16 + m, j = j0 + wj + tb * 16 + kq + 4 * r;
                if (i < K && j < K)
                    o[(size_t)j * K + i] = acc[ta][tb][r];
            }
}

// One thread per element of the scatter: the chunks' partial sums in ascending order.  Element
// (i, j) with i > j lies in a tile that was not formed (or in the lower half of a diagonal one): it is
// read from (j, i).  out[i + K j].
__global__ __launch_bounds__(kTopicDocsThreads) void topicdocs_finish_kernel(int K, int chunks,
                                                                             const double *__restrict__ part,
                                                                             double *__restrict__ out)
{
#pragma clang fp contract(off)
    const size_t n = (size_t)K * K, e = (size_t)blockIdx.x * kTopicDocsThreads + threadIdx.x;
    if (e >= n)
        return;
    const int p = (int)(e % K), q = (int)(e / K);
    const int i = min(p, q), j = max(p, q);
    const size_t src = (size_t)j * K + i;
    double a = 0.0;
    for (int c = 0; c < chunks; ++c)
        a += part[(size_t)c * n + src];
    out[e] = a;
}

}  // namespace trlda
