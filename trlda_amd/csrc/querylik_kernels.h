// trlda_amd/csrc/querylik_kernels.h -- indexed documents ranked by query likelihood: the probability a
// document's topic mixture gives a query's words (trlda_docindex_query_likelihood; the
// LDA term of Wei & Croft's LBDM, SIGIR 2006).  Nothing is inferred for the query.  No reference
// counterpart.
//
// Contract.  Query q with entries (w_i, c_i), i = 0 .. n_q - 1 in the batch's order, indexed document d:
//   b_ik    = lambda_k,w_i / R_k     R_k = sum_v lambda_kv formed from lambda itself (rowsum_partial_kernel,
//                                    rowsum_combine_wave_kernel: the row sums of recommend_kernels.h);
//                                    IEEE division
//   theta^_dk                        from the stored row by topicdocs_theta (topicdocs_kernels.h): r * r
//                                    (hellinger) or r / sum_j r_j (cosine, the sum by topicdocs_scale_kernel)
//   P(d, i) = sum_k theta^_dk b_ik   by v_mfma_f64_16x16x4_f64: one chain of Kp / 4 instructions over
//                                    k = 0, 4, 8, ..., each adding four products to the running value
//                                    (Kp = ceil(K / 4) * 4; topics past K add +0)
//   t_i     = c_i * log(P(d, i))     the fp64 log, one IEEE multiply (never contracted)
// P depends on the index row, the word's b row and K alone -- not on the tile, the slab, the workgroup,
// the batch or the number of rows in the index.  log(0) = -inf, c_i > 0 and P >= 0: no NaN arises.
//
// Word table.  querylik_words_kernel writes the b rows row-major with stride Kp and a zero tail.  A
// query's rows start at a multiple of 16 rows (tile_off[q] * 16) and its last tile of 16 is padded
// with zero rows of count 0, so a tile never mixes two queries.  An entry with c_i <= 0 is a row of
// count 0 too.  A row of count 0 is SKIPPED BY PREDICATE: its term is never formed (not multiplied by
// a zero count, which would turn log(0) = -inf into NaN).
//
// Order of additions.  score(q, d) = sum_i t_i is added in an order that depends on the word's position
// i within its query only.  Position i lies in tile T = i / 16 at j = i % 16, in lane group g = j % 4
// and register r = j / 4 of the MFMA result:
//   p_g   = ((t_g + t_g+4) + t_g+8) + t_g+12       per lane group, ascending r, from 0.0; skipped terms
//                                                  are left out (0.0 + x = x: nothing is rounded)
//   S_T   = (p_0 + p_1) + (p_2 + p_3)              the four lanes that hold one document: two butterfly
//                                                  steps (IEEE addition commutes: all four get the same bits)
//   score = ((S_0 + S_1) + S_2) + ...              tiles in ascending order, from 0.0
// A query without entries has no tiles: its score is 0.0 for every document.
//
// Ranking.  The index's total order (score descending, id ascending).  querylik_score_kernel keeps, per
// query, slab of index rows and WAVE, the best top_n pairs in the wave's own LDS list
// (docindex_before / docindex_insert); the lists leave as (slabs * 4) x B x top_n candidates and
// docindex_merge_kernel ranks them as it ranks slabs' lists.  The order is total, so neither the slab
// partition, the wave a row falls to nor the order of arrival shows in the result.  No atomics.  Nothing
// of size B x N or N x (words) exists in global memory.
#pragma once

#include <climits>

#include "topicdocs_kernels.h"

namespace trlda {

constexpr int kQueryLikThreads = 256;      // 4 waves
constexpr int kQueryLikWaves = kQueryLikThreads / kWave;
constexpr int kQueryLikWordTile = 16;      // words per tile: one MFMA operand
constexpr int kQueryLikWaveTiles = 2;      // tiles of 16 index rows a wave multiplies at a time
constexpr int kQueryLikWaveRows = 16 * kQueryLikWaveTiles;
constexpr int kQueryLikGroup = kQueryLikWaves * kQueryLikWaveRows;   // index rows a workgroup takes at a time
constexpr int kQueryLikChunk = kDocIndexChunk;       // the k chunk staged in LDS
constexpr int kQueryLikStride = kDocIndexStride;     // (its bank argument: tile_product.h)

// LDS of querylik_score_kernel: the index chunk (theta^), the word chunk, the tile's counts, the four
// lists (fp64 score, int32 row in slab)
constexpr size_t querylik_score_lds(int top_n)
{
    return (size_t)(kQueryLikGroup + kQueryLikWordTile) * kQueryLikStride * sizeof(double) +
           (size_t)kQueryLikWordTile * sizeof(double) +
           (size_t)kQueryLikWaves * top_n * (sizeof(double) + sizeof(int));
}

// One workgroup per query: wave w writes rows w, w + 4, ... of the query's tiles.  Row i < n_q with
// c_i > 0 is b_i (lambda's column w_i, K contiguous doubles, each divided by R_k) with count c_i; every
// other row of the tiles is zeros with count 0.  wtab: (tiles * 16) x Kp, wcnt: tiles * 16.
__global__ __launch_bounds__(kQueryLikThreads) void querylik_words_kernel(
    int K, int Kp, int V, const int32_t *__restrict__ indptr, const int32_t *__restrict__ ids,
    const int32_t *__restrict__ cnts, const int *__restrict__ tile_off, const double *__restrict__ lambda,
    const double *__restrict__ rs, double *__restrict__ wtab, double *__restrict__ wcnt)
{
#pragma clang fp contract(off)
    const int q = blockIdx.x, lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const int p0 = indptr[q], n = indptr[q + 1] - p0;
    const long long row0 = (long long)tile_off[q] * kQueryLikWordTile;
    const int rows = (tile_off[q + 1] - tile_off[q]) * kQueryLikWordTile;
    for (int i = wid; i < rows; i += kQueryLikWaves) {     // (the whole wave)
        int w = -1, c = 0;
        if (i < n) {
            w = ids[p0 + i];
            c = cnts[p0 + i];
        }
        const bool live = c > 0 && w >= 0 && w < V;
        double *o = wtab + (size_t)(row0 + i) * Kp;
        const double *col = lambda + (size_t)(live ? w : 0) * K;
        for (int k = lane; k < Kp; k += kWave)
            o[k] = live && k < K ? col[k] / rs[k] : 0.0;
        if (lane == 0)
            wcnt[row0 + i] = live ? (double)c : 0.0;
    }
}

// Grid (query, slab of slab_rows index rows), 4 waves.  The workgroup takes the slab 128 rows at a
// time; wave w owns rows w * 32 ... w * 32 + 31 of them as two MFMA tiles -- their products, their
// running scores and its own list -- and multiplies them with the query's word tiles, one tile of 16
// after the other.  Both operands are staged in LDS in k chunks of 32 taken in ascending k, the index
// rows as theta^ (topicdocs_theta is applied while staging: no second table is kept).  The loop over
// the word tiles lies INSIDE the one over the rows, so the running scores stay in registers; the index
// chunk is staged again for every word tile.  A query of up to 16 words, the common case, has one tile
// and stages every chunk once.  Rows past N are read as row N - 1 (the product is formed) and kept out
// of the selection.
//   A operand: lane l holds b[word l & 15][k + (l >> 4)]; B operand: theta^[row l & 15][k + (l >> 4)];
//   D: register r of lane l is P(row l & 15, word (l >> 4) + 4 r).
// The lanes l, l + 16, l + 32, l + 48 hold the 16 words of one row; after the two butterfly steps each
// of them has the row's tile sum, and lane l < 16 proposes the row to the list.
// A list holds top_n (score, row in slab) pairs: the selection of tile_product.h, one list per wave.
// out_s / out_id: ((slab * 4 + wave) x B x top_n), the pad written as (-inf, int64 max).
__global__ __launch_bounds__(kQueryLikThreads) void querylik_score_kernel(
    int Kp, long long N, int B, int measure, int top_n, int slab_rows, const double *__restrict__ table,
    const double *__restrict__ scale, const int *__restrict__ tile_off, const double *__restrict__ wtab,
    const double *__restrict__ wcnt, double *__restrict__ out_s, long long *__restrict__ out_id)
{
#pragma clang fp contract(off)
    constexpr int S = kQueryLikStride, G = kQueryLikGroup, WT = kQueryLikWaveTiles, WR = kQueryLikWaveRows;
    constexpr int C2 = kQueryLikChunk / 2;                  // double2 per staged row
    extern __shared__ __attribute__((aligned(16))) double querylik_lds[];
    double *r_lds = querylik_lds;                           // G x S
    double *w_lds = r_lds + G * S;                          // 16 x S
    double *c_lds = w_lds + kQueryLikWordTile * S;          // 16
    double *ls = c_lds + kQueryLikWordTile;                 // 4 x top_n
    int *li = reinterpret_cast<int *>(ls + kQueryLikWaves * top_n);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int m = lane & 15, kq = lane >> 4;
    const int q = blockIdx.x;
    const long long slab0 = (long long)blockIdx.y * slab_rows;
    const int nrows = (int)min((long long)slab_rows, N - slab0);
    const int tile0 = tile_off[q], ntiles = tile_off[q + 1] - tile0;

    select_init(ls, li, kQueryLikWaves * top_n, tid, kQueryLikThreads);
    __syncthreads();

    for (int g0 = 0; g0 < nrows; g0 += G) {
        double score[WT];
#pragma unroll
        for (int j = 0; j < WT; ++j)
            score[j] = 0.0;

        for (int t = 0; t < ntiles; ++t) {
            const double *wrow = wtab + (size_t)(tile0 + t) * kQueryLikWordTile * Kp;
            docindex_f64x4 acc[WT];
#pragma unroll
            for (int j = 0; j < WT; ++j)
                acc[j] = docindex_f64x4{0.0, 0.0, 0.0, 0.0};

            for (int k0 = 0; k0 < Kp; k0 += kQueryLikChunk) {
                const int cl = min(kQueryLikChunk, Kp - k0);    // a multiple of 4
                __syncthreads();                                // the previous chunk and counts have been read
                if (k0 == 0 && tid < kQueryLikWordTile)
                    c_lds[tid] = wcnt[(size_t)(tile0 + t) * kQueryLikWordTile + tid];
                {
                    const int row = tid / C2, c = (tid % C2) * 2;   // 16 rows x 16 double2: one each
                    if (c < cl)
                        *reinterpret_cast<double2 *>(w_lds + row * S + c) =
                            *reinterpret_cast<const double2 *>(wrow + (size_t)row * Kp + k0 + c);
                }
                for (int i = tid; i < G * C2; i += kQueryLikThreads) {
                    const int row = i / C2, c = (i % C2) * 2;
                    if (c < cl) {
                        const long long d = min(slab0 + g0 + row, N - 1);
                        const double2 x = *reinterpret_cast<const double2 *>(table + (size_t)d * Kp + k0 + c);
                        double2 y;
                        y.x = topicdocs_theta(x.x, measure, scale, d);
                        y.y = topicdocs_theta(x.y, measure, scale, d);
                        *reinterpret_cast<double2 *>(r_lds + row * S + c) = y;
                    }
                }
                __syncthreads();
                for (int kk = 0; kk < cl; kk += 4) {
                    const double a = w_lds[m * S + kk + kq];
                    double b[WT];
#pragma unroll
                    for (int j = 0; j < WT; ++j)
                        b[j] = r_lds[(wid * WR + j * 16 + m) * S + kk + kq];
#pragma unroll
                    for (int j = 0; j < WT; ++j)
                        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[j], acc[j], 0, 0, 0);
                }
            }

            // the tile's terms: lane group kq holds words kq, kq + 4, kq + 8, kq + 12 of its rows
            double cw[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                cw[r] = c_lds[kq + 4 * r];
#pragma unroll
            for (int j = 0; j < WT; ++j) {
                double p = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (cw[r] > 0.0) {                          // (a pad or dead entry: no term)
                        const double term = cw[r] * log(acc[j][r]);
                        p = p + term;
                    }
                p = p + __shfl_xor(p, 16, kWave);               // (p_0 + p_1), (p_2 + p_3)
                p = p + __shfl_xor(p, 32, kWave);               // their sum, in all four lanes
                score[j] = score[j] + p;
            }
        }

        // the selection: the wave's own rows of this pass, proposed by lanes 0 .. 15
#pragma unroll
        for (int j = 0; j < WT; ++j) {
            const double v = score[j];
            const int rl = g0 + wid * WR + j * 16 + m;              // index row in the slab
            const double tv = ls[wid * top_n + top_n - 1];
            const int ti = li[wid * top_n + top_n - 1];
            const bool pass = kq == 0 && rl < nrows && docindex_before(v, rl, tv, ti);
            select_offer(pass, v, ls, li, top_n, lane, [&](int) { return wid; },
                         [&](int L) { return g0 + wid * WR + j * 16 + L; });
        }
    }

    // the wave's list as one run of top_n values
    const size_t o = (((size_t)blockIdx.y * kQueryLikWaves + wid) * B + q) * top_n;
    select_write<1>(ls + wid * top_n, li + wid * top_n, top_n, 1, out_s + o, out_id + o, slab0, (long long)LLONG_MAX,
                    lane);
}

}  // namespace trlda
