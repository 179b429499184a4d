// trlda_amd/csrc/effects_kernels.h -- topic prevalence against what the caller knows about the indexed
// documents: the weighted mean and variance of theta^ per group of a labelling, and the least-squares
// regression of theta^ on a design matrix (trlda_docindex_group_moments,
// trlda_docindex_regress_products, trlda_docindex_regress_residuals).  No reference
// counterpart.
//
// theta^ is topicdocs_theta of the stored row everywhere (topicdocs_kernels.h), with
// topicdocs_scale_kernel's row sums for a cosine index.  Nothing here is atomic, nothing depends on
// launch order, and every + - x / is one rounded fp64 operation (fp contract off).
//
// Group passes.  The ids are sorted by label with the counting sort of cluster_kernels.h (stable:
// within a group the ids ascend; the left-out documents take the slot past the last group, whose
// chunks no kernel here visits).  A group's members are taken in chunks of kClusterChunkRows in that
// order; within a chunk the terms are added one after the other from 0.0, the chunk sums of a group in
// ascending order, then one division:
//   first pass    term w_d x theta^_dk (theta^_dk without weights); W_g = sum w_d in the same order
//                 (without weights the chunk's member count as a double); mean = S / W
//   second pass   q = theta^_dk - mean_gk, term (w_d x q) x q (q x q without weights); no division
// A group's column is a function of its members' rows, their weights and K alone.
//
// Products.  G = Z^T W Z (P x P) and C = Z^T W Theta^ (P x K) of the design Z (N x P row-major, row
// stride Pp), the rectangular sibling of topicdocs_scatter_kernel: 64 x 64 tiles on
// v_mfma_f64_16x16x4_f64, 32 rows staged [row][column] at a time, the left operand staged as
// w_d x z_dp (one multiply; z_dp without weights), the right one as z_dq or theta^_dk.  N is cut into
// chunks of `cr` rows (effects_chunk_rows: a function of P, K, N); within a chunk every element is
// one chain of MFMAs over ascending rows, four at a time; the chunks' partial sums are added in
// ascending order.  Only the Gram's tile pairs (pi <= pj) are formed and (q, p) is read from (p, q):
// the Gram is bitwise symmetric.
//
// Residuals.  rss_k = sum_d w_d (theta^_dk - sum_p z_dp b_pk)^2, formed explicitly.  fit is the staged
// tile product of tile_product.h, X the design rows and Y the K coefficient rows of Pp doubles: one
// chain of Pp / 4 MFMAs from +0 per (document, topic).  r = theta^ - fit, term (w x r) x r (r x r
// without weights).  A workgroup owns a fixed block of kEffectsBlockDocs = 64 documents: the 64 terms
// of a topic are added one after the other from 0.0 in ascending document order (a document past N
// adds an exact +0), and the blocks in ascending order.  Nothing of size N x K is written.
#pragma once

#include "cluster_kernels.h"

#define TRLDA_EFFECTS_MAX_COLUMNS 256

namespace trlda {

constexpr int kEffectsThreads = 256;       // 4 waves
constexpr int kEffectsTile = kTopicDocsTile;       // a workgroup's tile of the products: 64 x 64
constexpr int kEffectsStage = kTopicDocsStage;     // rows staged in LDS at a time
constexpr int kEffectsStride = kTopicDocsStride;   // LDS row stride in doubles (topicdocs_kernels.h)
constexpr int kEffectsMaxColumns = TRLDA_EFFECTS_MAX_COLUMNS;   // P': a chosen number
constexpr int kEffectsBlockDocs = 64;      // documents per partial sum of the residuals
// LDS row stride of the residuals' terms in doubles: odd, so the 64 threads that each add one topic
// down the 64 documents, and the lanes that write 16 topics of 4 documents, meet different banks
constexpr int kEffectsTermStride = kEffectsBlockDocs + 1;
constexpr int kEffectsTargetGroups = 1024; // workgroups the chunking of the products aims at
constexpr int kEffectsMinChunk = 64;       // ... without cutting N finer than this

// LDS of effects_residual_kernel: the two staged operands, then -- in the same bytes -- the terms
constexpr size_t effects_residual_lds() { return tile_operands_lds(kEffectsBlockDocs); }
static_assert((size_t)kEffectsBlockDocs * kEffectsTermStride * sizeof(double) <= effects_residual_lds(),
              "the terms lie where the operands lay");

inline int effects_tiles(int n) { return (n + kEffectsTile - 1) / kEffectsTile; }

// Workgroups per chunk of the products: the Gram's tile pairs (pi <= pj), then the cross tiles
inline long long effects_gram_pairs(int P)
{
    const long long T = effects_tiles(P);
    return T * (T + 1) / 2;
}
inline long long effects_product_items(int P, int K)
{
    return effects_gram_pairs(P) + (long long)effects_tiles(P) * effects_tiles(K);
}

// Rows per chunk of N: a multiple of the staging size, chosen so that items x chunks is about
// kEffectsTargetGroups.  P' = 16, K = 100, N = 1 000 000: 3 items, 341 chunks of 2944 rows, 5 MB of
// partial sums; P' = 64, K = 500, N = 200 000: 9 items, 113 chunks of 1792 rows, 33 MB.  A function of
// (P', K, N) alone.
inline long long effects_chunk_rows(int P, int K, long long N)
{
    long long chunks = kEffectsTargetGroups / effects_product_items(P, K);
    if (chunks < 1)
        chunks = 1;
    long long cr = (N + chunks - 1) / chunks;
    if (cr < kEffectsMinChunk)
        cr = kEffectsMinChunk;
    return (cr + kEffectsStage - 1) / kEffectsStage * kEffectsStage;
}

// Grid (chunk of kClusterChunkRows members of one group; cluster_max_chunks(N, G + 1) of them: those
// from cstart[G] on -- the left-out documents' and the surplus -- leave).  SECOND = false:
// part[chunk * K + k] = sum of w_d theta^_dk and wpart[chunk] = sum of w_d over the chunk's members,
// one after the other in the sorted order.  SECOND = true: part = sum of (w_d q) q, q = theta^_dk -
// mean[k + K g].  Thread t takes k = t, t + 256, ...; thread 0 also adds the weights.
template <bool SECOND>
__global__ __launch_bounds__(kEffectsThreads) void effects_group_kernel(
    int K, int Kp, int G, int measure, const double *__restrict__ table, const double *__restrict__ scale,
    const double *__restrict__ w, const long long *__restrict__ order, const long long *__restrict__ start,
    const long long *__restrict__ size, const long long *__restrict__ cstart, const double *__restrict__ mean,
    double *__restrict__ part, double *__restrict__ wpart)
{
#pragma clang fp contract(off)
    const long long chunk = blockIdx.x;
    if (chunk >= cstart[G])                                 // (the whole workgroup)
        return;
    // the group of the chunk: the last g with cstart[g] <= chunk (a group without members has no
    // chunk: cstart[g] = cstart[g + 1], and the search passes it)
    int lo = 0, hi = G;                                     // cstart[lo] <= chunk < cstart[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (cstart[mid] <= chunk)
            lo = mid;
        else
            hi = mid;
    }
    const long long m0 = start[lo] + (chunk - cstart[lo]) * kClusterChunkRows;
    const long long m1 = min(start[lo] + size[lo], m0 + kClusterChunkRows);
    for (int k = threadIdx.x; k < K; k += kEffectsThreads) {
        const double mk = SECOND ? mean[(size_t)lo * K + k] : 0.0;
        double s = 0.0;
        for (long long i = m0; i < m1; ++i) {
            const long long d = order[i];
            const double t = topicdocs_theta(table[(size_t)d * Kp + k], measure, scale, d);
            if (SECOND) {
                const double q = t - mk;
                s += w ? (w[d] * q) * q : q * q;
            } else {
                s += w ? w[d] * t : t;
            }
        }
        part[(size_t)chunk * K + k] = s;
    }
    if (!SECOND && threadIdx.x == 0) {
        double a = (double)(m1 - m0);
        if (w) {
            a = 0.0;
            for (long long i = m0; i < m1; ++i)
                a += w[order[i]];
        }
        wpart[chunk] = a;
    }
}

// One thread per element (k, g): the group's chunk sums in ascending order.  divide != 0:
// out[k + K g] = S / W with W the group's chunk weights in ascending order, and wsum[g] = W (a group
// with W = 0 gets 0 / 0 = NaN); divide == 0: out = the sum, wpart and wsum are not touched.
__global__ __launch_bounds__(kEffectsThreads) void effects_group_finish_kernel(int K, int G, int divide,
                                                                               const long long *__restrict__ cstart,
                                                                               const double *__restrict__ part,
                                                                               const double *__restrict__ wpart,
                                                                               double *__restrict__ out,
                                                                               double *__restrict__ wsum)
{
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * kEffectsThreads + threadIdx.x;
    if (e >= (size_t)K * G)
        return;
    const int k = (int)(e % K), g = (int)(e / K);
    const long long ch0 = cstart[g], ch1 = cstart[g + 1];
    double s = 0.0;
    for (long long ch = ch0; ch < ch1; ++ch)
        s += part[(size_t)ch * K + k];
    if (!divide) {
        out[e] = s;
        return;
    }
    double W = 0.0;
    for (long long ch = ch0; ch < ch1; ++ch)
        W += wpart[ch];
    out[e] = s / W;
    if (k == 0)
        wsum[g] = W;
}

// Grid (item, chunk of cr rows), 4 waves.  Item < effects_gram_pairs(P): the Gram's tile pair
// (ti <= tj), the right operand z; the others are the cross tiles (ti of P, tj of K), the right operand
// theta^.  Wave w owns the 32 x 32 block (w & 1, w >> 1) of the tile as 2 x 2 MFMA tiles; the layout is
// topicdocs_scatter_kernel's.  Columns past P or K and rows past the chunk's or the table's end are
// staged as exact zeros and are neither read from memory nor written out.
//   first operand:  lane l holds B[column l & 15][row kk + (l >> 4)] (tile tj), second: A likewise
//   (tile ti); D: register r of lane l is (tj column (l >> 4) + 4 r, ti column l & 15).
// part_g[(chunk * P + j) * P + i], i in tile ti, j in tile tj; part_c[(chunk * P + i) * K + j].
// A launch takes the items from item0 on and the chunks from chunk0 on (item0 = effects_gram_pairs(P):
// the cross items alone, part_g is not touched), and z holds the design from row z_row0 on: what
// classify_kernels.h works a slab of its rows off with.  The three are 0 for the regression.
__global__ __launch_bounds__(kEffectsThreads) void effects_products_kernel(
    int P, int Pp, int K, int Kp, long long N, long long cr, int measure, const double *__restrict__ z,
    const double *__restrict__ w, const double *__restrict__ table, const double *__restrict__ scale,
    double *__restrict__ part_g, double *__restrict__ part_c, int item0, long long chunk0, long long z_row0)
{
#pragma clang fp contract(off)
    constexpr int S = kEffectsStride, T = kEffectsTile, W = kEffectsStage;
    __shared__ __attribute__((aligned(16))) double a_lds[W * S], b_lds[W * S];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int m = lane & 15, kq = lane >> 4;
    const int wi = (wid & 1) * 32, wj = (wid >> 1) * 32;
    const int PT = (P + T - 1) / T, pairs = PT * (PT + 1) / 2;
    const int item = (int)blockIdx.x + item0;
    const long long chunk = (long long)blockIdx.y + chunk0;
    const bool cross = item >= pairs;
    int tj = 0, ti = item;
    if (cross) {
        ti = (item - pairs) % PT;
        tj = (item - pairs) / PT;
    } else {
        // the pair (ti <= tj): column tj holds the tj + 1 pairs from tj (tj + 1) / 2 on
        while (ti > tj) {
            ++tj;
            ti -= tj;
        }
    }
    const int i0 = ti * T, j0 = tj * T, J = cross ? K : P;
    const long long dbeg = chunk * cr, dend = min(N, dbeg + cr);
    const int st = tid & (T - 1), sw = tid / T;                     // staging: column, first row
    const bool a_in = i0 + st < P, b_in = j0 + st < J;
    const double *ap = z + (a_in ? i0 + st : 0);
    const double *bp = (cross ? table : z) + (b_in ? j0 + st : 0);
    const size_t bstride = cross ? Kp : Pp;

    topicdocs_f64x4 acc[2][2];
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
            acc[ta][tb] = topicdocs_f64x4{0.0, 0.0, 0.0, 0.0};

    for (long long d0 = dbeg; d0 < dend; d0 += W) {
        __syncthreads();                                            // the previous rows have been read
#pragma unroll
        for (int e = 0; e < W * T / kEffectsThreads; ++e) {
            const int r = sw + e * (kEffectsThreads / T);
            const long long d = d0 + r;
            double x = 0.0, y = 0.0;
            if (d < dend) {
                if (a_in) {
                    x = ap[(size_t)(d - z_row0) * Pp];
                    if (w)
                        x = w[d] * x;
                }
                if (b_in) {
                    y = bp[(size_t)(cross ? d : d - z_row0) * bstride];
                    if (cross)
                        y = topicdocs_theta(y, measure, scale, d);
                }
            }
            a_lds[r * S + st] = x;
            b_lds[r * S + st] = y;
        }
        __syncthreads();
        const int steps = ((int)min((long long)W, dend - d0) + 3) / 4;   // (the rows past the end are zeros)
        for (int s = 0; s < steps; ++s) {
            const int row = (s * 4 + kq) * S;
            double a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = a_lds[row + wi + t * 16 + m];
                b[t] = b_lds[row + wj + t * 16 + m];
            }
#pragma unroll
            for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                for (int tb = 0; tb < 2; ++tb)
                    acc[ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(b[tb], a[ta], acc[ta][tb], 0, 0, 0);
        }
    }

    double *og = part_g + (size_t)chunk * P * P, *oc = part_c + (size_t)chunk * P * K;
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + wi + ta * 16 + m, j = j0 + wj + tb * 16 + kq + 4 * r;
                if (i < P && j < J) {
                    if (cross)
                        oc[(size_t)i * K + j] = acc[ta][tb][r];
                    else
                        og[(size_t)j * P + i] = acc[ta][tb][r];
                }
            }
}

// One thread per element of the Gram (P x P) and of the cross products (P x K, row-major): the chunks'
// partial sums in ascending order.  Element (p, q) of the Gram with p > q lies in a tile that was not
// formed (or in the lower half of a diagonal one): it is read from (q, p).  The launch's first thread
// takes element e0 (e0 = P * P: the cross products alone, the Gram is not touched).
__global__ __launch_bounds__(kEffectsThreads) void effects_products_finish_kernel(int P, int K, int chunks,
                                                                                  const double *__restrict__ part_g,
                                                                                  const double *__restrict__ part_c,
                                                                                  double *__restrict__ gram,
                                                                                  double *__restrict__ cross,
                                                                                  size_t e0)
{
#pragma clang fp contract(off)
    const size_t ng = (size_t)P * P, nc = (size_t)P * K;
    const size_t e = e0 + (size_t)blockIdx.x * kEffectsThreads + threadIdx.x;
    if (e >= ng + nc)
        return;
    double a = 0.0;
    if (e < ng) {
        const int p = (int)(e % P), q = (int)(e / P);
        const size_t src = (size_t)max(p, q) * P + min(p, q);
        for (int c = 0; c < chunks; ++c)
            a += part_g[(size_t)c * ng + src];
        gram[e] = a;
    } else {
        const size_t f = e - ng;
        for (int c = 0; c < chunks; ++c)
            a += part_c[(size_t)c * nc + f];
        cross[f] = a;
    }
}

// Grid (block of kEffectsBlockDocs documents), 4 waves.  The topics are taken 64 at a time: the product
// and its layout are those of tile_product.h with SW = 1, X the block's design rows (Pp doubles each,
// the tail zero) and Y the coefficient rows (K rows of Pp).  Rows past N and coefficient rows past K
// are read as row N - 1 / K - 1 and kept out of what follows.  D: register r of acc[0][j] in lane l is
// fit(document w * 16 + (l >> 4) + 4 r of the block, topic 16 j + (l & 15) of the group).  The terms
// go to LDS -- where the operands lay -- as [document][topic]; thread t < 64 adds topic t down the
// documents.  part[block * K + k].
__global__ __launch_bounds__(kEffectsThreads) void effects_residual_kernel(
    int Pp, int K, int Kp, long long N, int measure, const double *__restrict__ z, const double *__restrict__ w,
    const double *__restrict__ coef, const double *__restrict__ table, const double *__restrict__ scale,
    double *__restrict__ part)
{
#pragma clang fp contract(off)
    constexpr int B = kEffectsBlockDocs, S = kDocIndexStride, TS = kEffectsTermStride;
    extern __shared__ __attribute__((aligned(16))) double effects_lds[];
    double *x_lds = effects_lds;                            // B x S
    double *y_lds = x_lds + B * S;                          // 64 x S
    double *terms = effects_lds;                            // B x TS, after the product
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int m = lane & 15, kq = lane >> 4;
    const long long d0 = (long long)blockIdx.x * B;

    for (int g0 = 0; g0 < K; g0 += 64) {
        docindex_f64x4 acc[1][4] = {};
        for (int k0 = 0; k0 < Pp; k0 += kDocIndexChunk) {
            const int cl = min(kDocIndexChunk, Pp - k0);    // a multiple of 4
            __syncthreads();                                // the previous chunk / the terms have been read
            tile_stage<B, kEffectsThreads>(x_lds, z, Pp, k0, cl, tid,
                                           [&](int row) { return min(d0 + row, N - 1); });
            tile_stage<64, kEffectsThreads>(y_lds, coef, Pp, k0, cl, tid,
                                            [&](int row) { return min(g0 + row, K - 1); });
            __syncthreads();
            for (int kk = 0; kk < cl; kk += 4)
                tile_step<1>(acc, x_lds, y_lds, kk, wid, m, kq);
        }
        __syncthreads();                                    // the operands have been read
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int dl = wid * 16 + kq + 4 * r, kl = j * 16 + m;
                const long long d = d0 + dl;
                const int k = g0 + kl;
                double term = 0.0;
                if (d < N && k < K) {
                    const double t = topicdocs_theta(table[(size_t)d * Kp + k], measure, scale, d);
                    const double q = t - acc[0][j][r];
                    term = w ? (w[d] * q) * q : q * q;
                }
                terms[dl * TS + kl] = term;
            }
        __syncthreads();
        if (tid < 64 && g0 + tid < K) {
            double s = 0.0;
            for (int dl = 0; dl < B; ++dl)
                s += terms[dl * TS + tid];
            part[(size_t)blockIdx.x * K + g0 + tid] = s;
        }
    }
}

// rss[k] = the blocks' partial sums added in ascending block order
__global__ __launch_bounds__(kEffectsThreads) void effects_residual_finish_kernel(int K, long long blocks,
                                                                                  const double *__restrict__ part,
                                                                                  double *__restrict__ rss)
{
#pragma clang fp contract(off)
    const int k = blockIdx.x * kEffectsThreads + threadIdx.x;
    if (k >= K)
        return;
    double a = 0.0;
    for (long long b = 0; b < blocks; ++b)
        a += part[(size_t)b * K + k];
    rss[k] = a;
}

}  // namespace trlda
