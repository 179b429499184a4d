// trlda_amd/csrc/tile_product.h -- what the search and grouping kernels of an index share: the staged
// fp64 tile product (docindex_query, cluster_assign, silhouette_pairs, neighbors_sweep, recommend_query,
// wordsim_query), the distance of a similarity, and the selection into sorted LDS lists (docindex_query,
// recommend_query, wordsim_query, querylik_score).  DESIGN.md 3.19.  No reference counterpart.
//
// The product.  s(x, y) = sum_k x_k y_k of two rows of Kp = ceil(K / 4) * 4 doubles (the tail zero), by
// v_mfma_f64_16x16x4_f64: every element of every 16 x 16 tile is the same chain of Kp / 4 instructions
// over k = 0, 4, 8, ..., each adding four products to the running value, whatever tile, slab or
// workgroup the pair lies in.  The zero tail adds +0.  s depends on the two rows and K alone.
//
// The layout.  A workgroup of 4 waves holds 64 SW rows of X and 64 rows of Y in LDS, a k chunk of
// kDocIndexChunk at a time, row-major with stride kDocIndexStride; the chunks are taken in ascending k.
// Wave w owns the X rows w * 16 SW ... as SW tiles of 16 and multiplies them with the 4 tiles of Y.
// With m = l & 15 and kq = l >> 4 of lane l:
//   A operand of tile t: lane l holds X[w * 16 SW + 16 t + m][k + kq];
//   B operand of tile j: lane l holds Y[16 j + m][k + kq];
//   D: register r of acc[t][j] in lane l is s(X row w * 16 SW + 16 t + kq + 4 r, Y row 16 j + m).
// A kernel declares `docindex_f64x4 acc[SW][4] = {};` per pass: every chain starts from +0.
// A row past the end of its operand is read as another row (the caller's row_of: a clamp, or an id
// list): the product is formed and the caller keeps it out of what follows.
// No function here holds a barrier: the staging, multiply and selection phases are the kernel's.
#pragma once

#include <climits>

#include "estep_kernels.h"

namespace trlda {

constexpr int kDocIndexChunk = 32;         // the k chunk staged in LDS
// LDS row stride in doubles: 2 mod 4, so the 16 rows x 2 columns that half a wave reads at once fall
// into 32 different 8-byte banks (row * 34 + c mod 32 = 2 row + c, c = 0, 1)
constexpr int kDocIndexStride = kDocIndexChunk + 2;

typedef double docindex_f64x4 __attribute__((ext_vector_type(4)));

// LDS of the two staged operands: `rows` rows of X and the 64 of Y
constexpr size_t tile_operands_lds(int rows) { return (size_t)(rows + 64) * kDocIndexStride * sizeof(double); }

// Columns k0 ... k0 + cl - 1 (cl <= kDocIndexChunk, a multiple of 4) of ROWS rows of the row-major src
// into lds, a double2 per thread and turn; LDS row `row` is row row_of(row) of src.
template <int ROWS, int THREADS, typename RowOf>
__device__ __forceinline__ void tile_stage(double *lds, const double *src, int Kp, int k0, int cl, int tid,
                                           RowOf row_of)
{
    constexpr int C2 = kDocIndexChunk / 2;
    for (int i = tid; i < ROWS * C2; i += THREADS) {
        const int row = i / C2, c = (i % C2) * 2;
        if (c < cl)
            *reinterpret_cast<double2 *>(lds + row * kDocIndexStride + c) =
                *reinterpret_cast<const double2 *>(src + (size_t)row_of(row) * Kp + k0 + c);
    }
}

// One step of every chain: columns kk ... kk + 3 of the staged chunk.
template <int SW>
__device__ __forceinline__ void tile_step(docindex_f64x4 (&acc)[SW][4], const double *x_lds, const double *y_lds,
                                          int kk, int wid, int m, int kq)
{
    constexpr int WQ = 16 * SW, S = kDocIndexStride;
    double a[SW], b[4];
#pragma unroll
    for (int t = 0; t < SW; ++t)
        a[t] = x_lds[(wid * WQ + t * 16 + m) * S + kk + kq];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        b[j] = y_lds[(j * 16 + m) * S + kk + kq];
#pragma unroll
    for (int t = 0; t < SW; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc[t][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b[j], acc[t][j], 0, 0, 0);
}

// the distance of two unit rows of similarity s: sqrt(max(0, 1 - s)) (hellinger) or max(0, 1 - s) (cosine)
__device__ __forceinline__ double docindex_distance(double s, int measure)
{
#pragma clang fp contract(off)
    const double d = fmax(1.0 - s, 0.0);
    return measure == 0 ? sqrt(d) : d;
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

// The selection.  A list holds top_n (value, id) pairs in LDS, sorted by docindex_before and filled with
// (-inf, INT_MAX) at the start: its last entry is the threshold a candidate must be before, and most are
// not.  A list belongs to one wave, so no list is shared between waves.  The kernel reads the threshold
// and forms `pass` and the value itself: what else keeps a candidate out is the kernel's own.

// the `count` entries of a workgroup's lists (a barrier stands between this and their first use)
__device__ __forceinline__ void select_init(double *ls, int *li, int count, int tid, int threads)
{
    for (int i = tid; i < count; i += threads) {
        ls[i] = -__builtin_huge_val();
        li[i] = INT_MAX;
    }
}

// Every lane of the wave offers (v, its id) where `pass`; the offers go in, one after the other in
// lane order: that of lane L as (v of L, id_of(L)) into list list_of(L).
template <typename ListOf, typename IdOf>
__device__ __forceinline__ void select_offer(bool pass, double v, double *ls, int *li, int top_n, int lane,
                                             ListOf list_of, IdOf id_of)
{
    unsigned long long mask = __ballot(pass);
    while (mask) {                                          // (uniform)
        const int L = __builtin_ctzll(mask);
        mask &= mask - 1;
        const int lo = __builtin_amdgcn_readlane(__double2loint(v), L);
        const int hi = __builtin_amdgcn_readlane(__double2hiint(v), L);
        const int cq = list_of(L);
        docindex_insert(ls + cq * top_n, li + cq * top_n, top_n, __hiloint2double(hi, lo), id_of(L), lane);
    }
}

// The first `live` of LISTS consecutive lists of a wave, each as one run of top_n values: the ids
// leave as id0 + id, the pad as (-inf, pad)
template <int LISTS, typename I>
__device__ __forceinline__ void select_write(const double *ls, const int *li, int top_n, int live, double *out_s,
                                             I *out_id, I id0, I pad, int lane)
{
    for (int w = 0; w < LISTS && w < live; ++w) {
        for (int p = lane; p < top_n; p += kWave) {
            const int id = li[w * top_n + p];
            out_s[(size_t)w * top_n + p] = ls[w * top_n + p];
            out_id[(size_t)w * top_n + p] = id == INT_MAX ? pad : id0 + id;
        }
    }
}

}  // namespace trlda
