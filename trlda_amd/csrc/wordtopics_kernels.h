// trlda_amd/csrc/wordtopics_kernels.h -- the per-word topic posterior of the variational path, the
// phi that LDA::updateVariablesVI forms inside its fixed point (src/lda.cpp:189-197) and drops:
// for every entry p = (d, w_p, c_p) of the batch's CSR, in the batch's own entry order,
//   s_pk   = exp(psi(gamma_dk) - psi(rs_k)) * exp(psi(lambda_{k, w_p})),   rs_k = sum_v lambda_kv
//   Z_p    = sum_k s_pk
//   phi_pk = s_pk / Z_p
// and the output is the top_n topics of the row in decreasing phi, equal values by smaller topic id
// first (the rule of trlda_model_top_words): topics[p * top_n + r] (int32) and probs[p * top_n + r]
// (fp64), 1 <= top_n <= min(K, 32).  With top_n = K a row of probs is the whole posterior in ranked
// order.  The row depends on w_p and gamma_d only: an entry with c_p = 0 gets a row like any other,
// a document without entries none.  lambda and gamma are taken to be positive and finite; a product
// that is NaN is never picked, and a rank for which nothing is left gets topic -1.
//
// Arithmetic, pinned: the factor f_k = exp_digamma_minus(gamma_dk, digamma(rs_k)) (psi.h), the
// product s_pk = f_k * exp_digamma(lambda_{k, w_p}) rounded once (no contraction with the sum).
// The order of the additions in Z_p depends on K and the wave width (64) alone: lane l adds
// s_{p, l}, s_{p, l + 64}, s_{p, l + 128}, ... in that order, starting from the first, and the 64 lane
// sums go through wave_sum_dpp (row shifts 1, 2, 4, 8, row broadcasts 15 and 31).  phi = s / Z is one
// IEEE division.  The grid, the number of waves and the way a long document is cut into workgroups
// play no part, so a document's rows are bitwise the same alone and inside any batch for the same
// gamma column.  No atomics, nothing depends on the order in which workgroups or waves arrive.
//
// Shape (that of heldout_docs_kernel): a workgroup belongs to one document and forms its K factors
// once in LDS -- K doubles, 54.5 KB at K = 6814, less than the general document kernel holds.  A wave
// takes one entry at a time and reads the word's K contiguous doubles of lambda coalesced.  The grid
// is (document, chunk of kWordTopicsChunk = 128 entries), so a long document is spread over
// ceil(n / 128) workgroups instead of forming the launch's tail; a workgroup whose chunk lies beyond
// its document leaves at once.  Each chunk forms the K factors again: 2 K digammas against the
// (up to) 128 K of its entries, under 2 % of a full chunk's work.
//
// Selection: K <= 512 keeps the row's products in registers (KPL = ceil(K / 64) per lane) and takes
// top_n wave arg-max passes over them.  Beyond (KPL = 0) nothing is kept: each of the top_n passes
// forms the same products again from the same operands -- the same bits -- and picks the first
// product that lies strictly after the previous pick in the order (value descending, id ascending);
// the first pass also adds up Z.  No K doubles per wave anywhere, so every K of the VI path fits.
// DESIGN.md 3.18.
#pragma once

#include "estep_kernels.h"

namespace trlda {

constexpr int kWordTopicsThreads = 256;
constexpr int kWordTopicsChunk = 128;      // entries of a document per workgroup: 32 per wave
constexpr int kWordTopicsMaxTop = 32;      // top_n <= min(K, 32): rank r is kept by lane r until the row is written
constexpr int kWordTopicsRegMaxK = 512;    // the products of a row in registers up to here

__device__ __forceinline__ double wt_product(double f, double lam)
{
    return __dmul_rn(f, exp_digamma(lam));
}

// the first of the wave's 64 (v, k) pairs in the order (v descending, k ascending), in every lane
__device__ __forceinline__ void wt_wave_first(double &v, int &k)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, kWave);
        const int ok = __shfl_xor(k, off, kWave);
        const bool take = ov > v || (ov == v && ok < k);
        v = take ? ov : v;
        k = take ? ok : k;
    }
}

// does (v, k) lie strictly after the pick (pv, pk)?
__device__ __forceinline__ bool wt_after(double v, int k, double pv, int pk)
{
    return v < pv || (v == pv && k > pk);
}

template <int KPL>
__global__ __launch_bounds__(kWordTopicsThreads) void word_topics_kernel(
    int K, int top_n, const int32_t *__restrict__ indptr, const int32_t *__restrict__ ids,
    const double *__restrict__ lambda, const double *__restrict__ rowsum, const double *__restrict__ gamma,
    int32_t *__restrict__ topics, double *__restrict__ probs)
{
    constexpr int W = kWordTopicsThreads / kWave;
    extern __shared__ __attribute__((aligned(16))) double wt_fac[];   // K factors
    const int d = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const int p0 = indptr[d], n = indptr[d + 1] - p0;
    const int chunks = (n + kWordTopicsChunk - 1) / kWordTopicsChunk;
    if ((int)blockIdx.y >= chunks)                   // (the whole workgroup)
        return;
    const double *g = gamma + (size_t)d * K;
    for (int k = threadIdx.x; k < K; k += kWordTopicsThreads)
        wt_fac[k] = exp_digamma_minus(g[k], digamma(rowsum[k]));
    __syncthreads();

    const double inf = __builtin_huge_val();
    for (int c = blockIdx.y; c < chunks; c += gridDim.y) {
        const int q0 = p0 + c * kWordTopicsChunk;
        const int q1 = min(q0 + kWordTopicsChunk, p0 + n);
        for (int p = q0 + wid; p < q1; p += W) {     // (p: the wave's own, uniform)
            const double *col = lambda + (size_t)ids[p] * K;
            double z = 0.0;
            double pv = inf, mine_v = 0.0;           // the previous pick; rank `lane`'s pick
            int pk = -1, mine_k = -1;
            if constexpr (KPL > 0) {
                double s[KPL];
#pragma unroll
                for (int j = 0; j < KPL; ++j) {
                    const int k = lane + j * kWave;
                    s[j] = -1.0;                     // (a product is >= 0 or NaN)
                    if (k < K) {
                        s[j] = wt_product(wt_fac[k], col[k]);
                        z += s[j];
                    }
                }
                z = wave_sum_dpp(z);
                for (int r = 0; r < top_n; ++r) {
                    double bv = -1.0;
                    int bk = K;
#pragma unroll
                    for (int j = 0; j < KPL; ++j) {
                        const int k = lane + j * kWave;
                        if (k < K && s[j] > bv && wt_after(s[j], k, pv, pk)) {   // (k ascends: the first of equals stays)
                            bv = s[j];
                            bk = k;
                        }
                    }
                    wt_wave_first(bv, bk);
                    pv = bv;
                    pk = bk;
                    if (lane == r) {
                        mine_v = bv;
                        mine_k = bk;
                    }
                }
            } else {
                for (int r = 0; r < top_n; ++r) {
                    double bv = -1.0;
                    int bk = K;
                    for (int k = lane; k < K; k += kWave) {
                        const double s = wt_product(wt_fac[k], col[k]);
                        if (r == 0)
                            z += s;
                        if (s > bv && wt_after(s, k, pv, pk)) {
                            bv = s;
                            bk = k;
                        }
                    }
                    if (r == 0)
                        z = wave_sum_dpp(z);
                    wt_wave_first(bv, bk);
                    pv = bv;
                    pk = bk;
                    if (lane == r) {
                        mine_v = bv;
                        mine_k = bk;
                    }
                }
            }
            if (lane < top_n) {
                const size_t o = (size_t)p * top_n + lane;
                topics[o] = mine_k < K ? mine_k : -1;
                probs[o] = mine_k < K ? mine_v / z : __builtin_nan("");
            }
        }
    }
}

}  // namespace trlda
