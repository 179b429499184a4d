// trlda_amd/csrc/coherence_kernels.h -- the device half of topic coherence: the
// top words of every topic, and the document counts of word lists that UMass (Mimno et al. 2011)
// and NPMI (Bouma 2009) are formed from.
//
// Top words.  lambda is column-major (a word's K values are contiguous, a topic's row is strided
// by 8 K bytes), so the selection reads lambda once, by word columns:
//   topn_tile_kernel   a workgroup per (8 topics, 1024 words): the tile's 8 x 1024 values are read
//                      64 contiguous bytes per word into LDS, then each wave selects the best N of
//                      one topic's 1024 and writes them, unordered, as that tile's candidates;
//   topn_merge_kernel  a wave per (topic, 1024 candidates): the best N of them, as the next level's
//                      candidates -- or, at the last level, sorted, as the topic's N word ids.
// "Best" is the order of np.lexsort((arange(V), -lambda[k])): larger value first, equal values by
// smaller word id.  Values are compared as 64-bit keys that order like the doubles (-0 as +0, NaN
// after everything, as NumPy sorts it), so ties are exact whichever tile they fall in.  A wave's
// selection is a threshold search over its 1024 (key, id) pairs: the N-th best key bit by bit, then
// among the pairs with that key the id bit by bit, each step a count over the wave (ballots).
//
// Counts.  For a list of T x N word ids (distinct within a row), U distinct words in all, each word
// gets a slot; per block of documents every slot gets a row of bits, one per document:
//   cooc_bits_kernel   a wave per document sets bit d of the row of each listed word with a count
//                      > 0 (global atomic or: the result does not depend on the order);
//   cooc_pairs_kernel  a workgroup per topic adds popcount(row_i & row_j) to co[t][i][j], i < j,
//                      over the block's rows in LDS chunks of 64 words (4096 documents);
//   cooc_df_kernel     a wave per slot adds the popcount of its row to doc_freq[slot] (int64) and
//                      clears the row (the rows are zeroed once, when the accumulator is made).
// All of it is integer arithmetic: the counts are exact whatever the order of the threads.
#pragma once

#include "estep_kernels.h"

namespace trlda {

constexpr int kTopnMax = 100;            // top_n and list lengths N: 1 .. 100
constexpr int kTopnTileTopics = 8;       // 64 contiguous bytes of each word's column
constexpr int kTopnTileWords = 1024;
constexpr int kTopnThreads = kWave * kTopnTileTopics;   // a wave per topic of the tile
constexpr int kTopnPerLane = 16;         // a wave selects from 64 x 16 = 1024 pairs
constexpr int kTopnGroup = kWave * kTopnPerLane;
constexpr int kTopnTileStride = kTopnTileWords + 1;   // (LDS row stride of the tile, in doubles)
constexpr int32_t kTopnPadId = 0x7fffffff;           // a filler pair (key 0, kTopnPadId) loses to every word
constexpr int kCoocThreads = 256;
constexpr int kCoocChunk = 64;           // 64-bit words of a row per LDS chunk of the pair kernel
constexpr int kCoocChunkStride = kCoocChunk + 1;

// an unsigned key that orders like the double: larger value, larger key; -0 as +0; NaN (either
// sign) is 0, below every number, so it sorts after them as in NumPy
__device__ __forceinline__ uint64_t topn_key(double x)
{
    if (x != x)
        return 0;
    const uint64_t u = x == 0.0 ? 0ull : (uint64_t)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ int wave_count(bool p)
{
    return __popcll(__ballot(p));
}

// The wave's selection of the best n of its kTopnGroup pairs (key[j], id[j]) in the lanes'
// registers: (T, I) such that exactly the pairs with key > T, or key == T and id <= I, are the best
// n -- as long as the pairs are distinct (fillers may repeat: the caller writes at most n).
__device__ __forceinline__ void topn_threshold(const uint64_t (&key)[kTopnPerLane],
                                               const int32_t (&id)[kTopnPerLane], int n, uint64_t &T,
                                               int32_t &I)
{
    // the n-th largest key: the largest T with #(key >= T) >= n.  A step that finds exactly n
    // keys >= c is done: those n are the selection whatever the lower bits say (c > 0, so no
    // filler is among them), and (c, any id) selects them -- without ties at the n-th key that
    // happens once c falls between the n-th and the (n+1)-th key, about 20 steps in, not 64
    uint64_t t = 0;
    for (int bit = 63; bit >= 0; --bit) {
        const uint64_t c = t | (1ull << bit);
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < kTopnPerLane; ++j)
            cnt += wave_count(key[j] >= c);
        if (cnt == n) {
            T = c;
            I = kTopnPadId;
            return;
        }
        if (cnt > n)
            t = c;
    }
    int above = 0;
#pragma unroll
    for (int j = 0; j < kTopnPerLane; ++j)
        above += wave_count(key[j] > t);
    const int r = n - above;                 // the pairs of key t to take: those of the r smallest ids
    // the r-th smallest id among key == t: the largest I with #(key == t, id < I) < r
    int32_t i = 0;
    for (int bit = 30; bit >= 0; --bit) {
        const int32_t c = i | (1 << bit);
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < kTopnPerLane; ++j)
            cnt += wave_count(key[j] == t && id[j] < c);
        if (cnt < r)
            i = c;
    }
    T = t;
    I = i;
}

// writes the selected pairs (at most n, in the order j, then lane) to key_out / id_out[0, n) and
// fillers after them; returns nothing -- exactly n entries are written
__device__ __forceinline__ void topn_emit(const uint64_t (&key)[kTopnPerLane], const int32_t (&id)[kTopnPerLane],
                                          int n, uint64_t T, int32_t I, uint64_t *__restrict__ key_out,
                                          int32_t *__restrict__ id_out)
{
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t below = (1ull << lane) - 1ull;
    int base = 0;
#pragma unroll
    for (int j = 0; j < kTopnPerLane; ++j) {
        const bool sel = key[j] > T || (key[j] == T && id[j] <= I);
        const uint64_t mask = __ballot(sel);
        const int pos = base + __popcll(mask & below);
        if (sel && pos < n) {
            key_out[pos] = key[j];
            id_out[pos] = id[j];
        }
        base += __popcll(mask);
    }
    for (int pos = base + lane; pos < n; pos += kWave) {
        key_out[pos] = 0;
        id_out[pos] = kTopnPadId;
    }
}

// First level: grid (ceil(K / 8), ceil(V / 1024)); candidates of topic k from tile y at
// ckey / cid[k * C + y * n, + n), C = gridDim.y * n.  Dynamic LDS: 8 x kTopnTileStride doubles.
__global__ __launch_bounds__(kTopnThreads) void topn_tile_kernel(int K, int V, int n,
                                                                 const double *__restrict__ lambda,
                                                                 uint64_t *__restrict__ ckey,
                                                                 int32_t *__restrict__ cid)
{
    extern __shared__ uint64_t tile[];       // [8][kTopnTileStride]
    const int k0 = blockIdx.x * kTopnTileTopics, w0 = blockIdx.y * kTopnTileWords;
    const int kt = min(kTopnTileTopics, K - k0);
    const int wt = min(kTopnTileWords, V - w0);
    for (int e = threadIdx.x; e < kTopnTileTopics * kTopnTileWords; e += kTopnThreads) {
        const int kk = e % kTopnTileTopics, ww = e / kTopnTileTopics;
        if (kk < kt && ww < wt)
            tile[kk * kTopnTileStride + ww] = topn_key(lambda[(size_t)(w0 + ww) * K + k0 + kk]);
    }
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const size_t C = (size_t)gridDim.y * n;
    const int kk = wid;
    if (kk < kt) {
        uint64_t key[kTopnPerLane];
        int32_t id[kTopnPerLane];
#pragma unroll
        for (int j = 0; j < kTopnPerLane; ++j) {
            const int ww = lane + kWave * j;
            const bool in = ww < wt;
            key[j] = in ? tile[kk * kTopnTileStride + ww] : 0ull;
            id[j] = in ? w0 + ww : kTopnPadId;
        }
        uint64_t T;
        int32_t I;
        topn_threshold(key, id, n, T, I);
        const size_t at = (size_t)(k0 + kk) * C + (size_t)blockIdx.y * n;
        topn_emit(key, id, n, T, I, ckey + at, cid + at);
    }
}

// Later levels: grid (groups, K), one wave each; group g of topic k takes candidates
// [g * 1024, min(C_in, (g + 1) * 1024)) of the topic's C_in.  words_out == nullptr: its best n go to
// okey / oid[k * gridDim.x * n + g * n, + n); else (gridDim.x == 1) words_out[k * n + r] is the word
// of rank r.
__global__ __launch_bounds__(kWave) void topn_merge_kernel(int n, int C_in, const uint64_t *__restrict__ ikey,
                                                           const int32_t *__restrict__ iid,
                                                           uint64_t *__restrict__ okey,
                                                           int32_t *__restrict__ oid,
                                                           int32_t *__restrict__ words_out)
{
    __shared__ uint64_t skey[kTopnMax];
    __shared__ int32_t sid[kTopnMax];
    const int lane = threadIdx.x;
    const int g = blockIdx.x, k = blockIdx.y;
    const uint64_t *ik = ikey + (size_t)k * C_in;
    const int32_t *ii = iid + (size_t)k * C_in;
    uint64_t key[kTopnPerLane];
    int32_t id[kTopnPerLane];
#pragma unroll
    for (int j = 0; j < kTopnPerLane; ++j) {
        const int p = g * kTopnGroup + lane + kWave * j;
        const bool in = p < C_in;
        key[j] = in ? ik[p] : 0ull;
        id[j] = in ? ii[p] : kTopnPadId;
    }
    uint64_t T;
    int32_t I;
    topn_threshold(key, id, n, T, I);
    if (!words_out) {
        const size_t at = (size_t)k * gridDim.x * n + (size_t)g * n;
        topn_emit(key, id, n, T, I, okey + at, oid + at);
        return;
    }
    topn_emit(key, id, n, T, I, skey, sid);
    __syncthreads();
    // the n selected pairs are distinct words: each one's rank is the number that beat it
    for (int p = lane; p < n; p += kWave) {
        const uint64_t kp = skey[p];
        const int32_t ip = sid[p];
        int r = 0;
        for (int q = 0; q < n; ++q)
            r += (skey[q] > kp || (skey[q] == kp && sid[q] < ip)) ? 1 : 0;
        words_out[(size_t)k * n + r] = ip;
    }
}

// documents [d0, d0 + nb) of a batch: bit (d - d0) of the row of slot[w] (row stride nw 64-bit
// words) for every entry (w, c) with c > 0 whose word is listed.  Grid ceil(nb / 4), a wave each.
__global__ __launch_bounds__(kCoocThreads) void cooc_bits_kernel(int d0, int nb, int V,
                                                                 const int32_t *__restrict__ indptr,
                                                                 const int32_t *__restrict__ ids,
                                                                 const int32_t *__restrict__ cnts,
                                                                 const int32_t *__restrict__ slot,
                                                                 unsigned long long *__restrict__ bits,
                                                                 int nw)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int dl = blockIdx.x * (kCoocThreads / kWave) + threadIdx.x / kWave;
    if (dl >= nb)
        return;
    const int d = d0 + dl;
    const unsigned long long bit = 1ull << (dl & 63);
    const size_t word = (size_t)(dl >> 6);
    for (int p = indptr[d] + lane; p < indptr[d + 1]; p += kWave) {
        const int w = ids[p];
        if (cnts[p] <= 0 || w < 0 || w >= V)
            continue;
        const int s = slot[w];
        if (s >= 0)
            atomicOr(bits + (size_t)s * nw + word, bit);
    }
}

// doc_freq[s] += popcount of row s (nw words), and the row is cleared for the next block (the last
// reader of the rows: launched after cooc_pairs_kernel).  Grid ceil(U / 4), a wave per slot.
__global__ __launch_bounds__(kCoocThreads) void cooc_df_kernel(int U, int nw, unsigned long long *__restrict__ bits,
                                                               long long *__restrict__ doc_freq)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int s = blockIdx.x * (kCoocThreads / kWave) + threadIdx.x / kWave;
    if (s >= U)
        return;
    unsigned long long *row = bits + (size_t)s * nw;
    int c = 0;
    for (int w = lane; w < nw; w += kWave) {
        c += __popcll(row[w]);
        row[w] = 0ull;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        c += __shfl_down(c, off, kWave);
    if (lane == 0)
        doc_freq[s] += c;
}

// co[t][i][j] += sum over the nw words of popcount(row_i & row_j), i < j < n, rows of the slots
// slot_of[t * n + i].  Grid T.  Dynamic LDS: n x kCoocChunkStride words, then n x n int32 counts.
__global__ __launch_bounds__(kCoocThreads) void cooc_pairs_kernel(int n, int nw,
                                                                  const int32_t *__restrict__ slot_of,
                                                                  const unsigned long long *__restrict__ bits,
                                                                  long long *__restrict__ co)
{
    extern __shared__ unsigned long long rows[];          // [n][kCoocChunkStride]
    int *cnt = reinterpret_cast<int *>(rows + (size_t)n * kCoocChunkStride);   // [n][n]
    const int t = blockIdx.x;
    const int nn = n * n;
    for (int p = threadIdx.x; p < nn; p += kCoocThreads)
        cnt[p] = 0;
    for (int c0 = 0; c0 < nw; c0 += kCoocChunk) {
        const int cw = min(kCoocChunk, nw - c0);
        __syncthreads();                                  // (the previous chunk's readers)
        for (int e = threadIdx.x; e < n * kCoocChunk; e += kCoocThreads) {
            const int i = e / kCoocChunk, w = e % kCoocChunk;
            rows[i * kCoocChunkStride + w] =
                w < cw ? bits[(size_t)slot_of[(size_t)t * n + i] * nw + c0 + w] : 0ull;
        }
        __syncthreads();
        for (int p = threadIdx.x; p < nn; p += kCoocThreads) {
            const int i = p / n, j = p % n;
            if (i >= j)
                continue;
            const unsigned long long *ri = rows + i * kCoocChunkStride, *rj = rows + j * kCoocChunkStride;
            int s = 0;
            for (int w = 0; w < cw; ++w)
                s += __popcll(ri[w] & rj[w]);
            cnt[p] += s;
        }
    }
    __syncthreads();
    long long *out = co + (size_t)t * nn;
    for (int p = threadIdx.x; p < nn; p += kCoocThreads)
        if (p / n < p % n)
            out[p] += cnt[p];
}

}  // namespace trlda
