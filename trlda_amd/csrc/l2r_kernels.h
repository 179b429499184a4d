// trlda_amd/csrc/l2r_kernels.h -- the marginal log-likelihood of a whole unseen document,
// log p(w_d | alpha, beta), by the left-to-right sequential sampler (Wallach, Murray, Salakhutdinov &
// Mimno 2009, Algorithm 3; Buntine 2009) with beta_kw = lambda_kw / rs_k, rs_k = sum_v lambda_kv (the
// point estimate of heldout_kernels.h and marginal_kernels.h).  It samples the tokens' topics, not
// theta, so it has no proposal; its inner step is the collapsed-Gibbs histogram draw of
// gibbs_kernels.h (histogram_draw).  Host side: trlda_hip.hip, trlda_model_left_to_right.
//
// Per document d with tokens w_0 .. w_{N-1} (the entries in order, an entry contributing its count
// c > 0 of consecutive tokens: the token index of the Gibbs contract), per particle r < R and per
// position n = 0 .. N-1, with n_k the counts of the topics the prefix's tokens hold at the moment:
//   1. (resample only) for t = 0 .. n-1 in order: n_{z_t} -= 1; z_t ~ w_k(w_t); n_{z_t} += 1
//   2. z_n ~ w_k(w_n); the histogram's own total T gives p_r(n) = T / (A + n)
//   3. n_{z_n} += 1
//   w_k(w) = (lambda_kw * inv_k) * (alpha_k + (double)n_k),  inv_k = 1 / rs_k
// each operation rounded once, alpha_k + n_k formed anew from the integer count, nothing contracted
// into an FMA; A = sum_k alpha_k, k ascending from 0 (l2r_alpha_sum_kernel), A + n one addition.
// Without `resample` this is the O(N) sequential sampler; with it the work is O(N^2) per particle.
//
// Draws: Philox4x32-10 under the call's key, u = philox_u(x0, x1) of the counter
//   purpose 22  a prefix token's redraw   (token t, position n, d R + r)
//   purpose 23  a new token's draw        (n, n, d R + r)
// (B R < 2^32 and N < 2^32 are the host's checks.)  A histogram whose total is not > 0 or not finite
// sets `flag`; the call then fails with the Gibbs path's error.
//
// l2r_docs_kernel<KPL>: one wave64 per (document, particle), kL2rWaves of them per workgroup, the
// particles of a document next to each other (they read the same columns of lambda).  Lane l holds
// topics l KPL .. l KPL + KPL - 1 as gibbs_docs_kernel does: an integer count, alpha_k and inv_k.
// The prefix's topics live as uint16 per (d, r, token) in a device workspace and pass through the
// lanes 64 tokens at a time (token t is always read and written by lane t mod 64); p_r(n) goes to
// a table of doubles per (d, token, r).  The columns of lambda are plain global reads, an entry's
// column loaded once for its tokens and the next entry's while this one's tokens run (DESIGN.md
// 3.17 has the measurement).
//
// l2r_finish_kernel: one wave per document over its table,
//   'particle'  L_r = sum_n log p_r(n), n ascending from 0 (lane r mod 64);
//               loglik = (M + log sum_r exp(L_r - M)) - log R, M = max_r L_r, r ascending from 0
//   'position'  loglik = sum_n log((sum_r p_r(n)) / R), r ascending from p_0(n), n ascending from 0
// exp(loglik) is unbiased for p(w_d) in the first form for any R; the second (the published one) is
// not for R > 1.  With R = 1 both are the same additions of the same logarithms.  A document without
// tokens gets exactly 0.  Nothing depends on the grid, the batch or the other documents.
#pragma once

#include "gibbs_kernels.h"
#include "philox.h"

namespace trlda {

enum : uint32_t {
    kL2rPrefix = 22,
    kL2rToken = 23,
};

constexpr int kL2rWaves = 4;                       // (document, particle) items per workgroup
// token-particles (N_d R, summed over a group's documents) the workspace holds: 8 B of p and 2 B of z
// each, 80 MiB in all
constexpr long long kL2rBudget = 1LL << 23;

struct L2rArgs {
    int K, R, resample;
    long long items;             // documents of the group x R
    uint32_t key0, key1;
    const int32_t *indptr, *ids, *cnts;
    const int32_t *docs;         // the group's documents
    const int64_t *off;          // B: a document's first token in the group's workspace (x R)
    const int64_t *tokens;       // B: tokens per document
    const double *lambda, *rowsum, *alpha;
    const double *asum;          // A
    uint16_t *z;
    double *p;
    int *flag;
};

__global__ void l2r_alpha_sum_kernel(int K, const double *__restrict__ alpha, double *__restrict__ out)
{
#pragma clang fp contract(off)
    if (blockIdx.x || threadIdx.x)
        return;
    double s = 0.0;
    for (int k = 0; k < K; ++k)
        s = s + alpha[k];
    *out = s;
}

template <int KPL>
__global__ __launch_bounds__(kL2rWaves *kWave) void l2r_docs_kernel(L2rArgs a)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const long long item = (long long)blockIdx.x * kL2rWaves + wv;
    if (item >= a.items)
        return;
    const int K = a.K, R = a.R;
    const int slot = (int)(item / R), r = (int)(item - (long long)slot * R);
    const int doc = a.docs[slot];
    const uint32_t N = (uint32_t)a.tokens[doc];
    if (N == 0)
        return;
    const int e0 = a.indptr[doc], e1 = a.indptr[doc + 1];
    const uint32_t c2 = (uint32_t)doc * (uint32_t)R + (uint32_t)r;
    const uint32_t k0 = a.key0, k1 = a.key1;
    const size_t base = (size_t)a.off[doc] * R;
    uint16_t *z = a.z + base + (size_t)r * N;
    double *pt = a.p + base + r;
    const double A = *a.asum;

    int n_r[KPL];
    double al[KPL], inv[KPL];
#pragma unroll
    for (int q = 0; q < KPL; ++q) {
        const int k = lane * KPL + q;
        n_r[q] = 0;
        al[q] = k < K ? a.alpha[k] : 0.0;
        inv[q] = k < K ? __ddiv_rn(1.0, a.rowsum[k]) : 0.0;
    }

    uint32_t n = 0;
    double un = 0.0;
    bool bad = false;
    for (int jn = e0; jn < e1; ++jn) {
        const int cn = max(a.cnts[jn], 0);
        if (cn == 0)
            continue;
        double w_n[KPL];
        {
            const double *col = a.lambda + (size_t)a.ids[jn] * K;
#pragma unroll
            for (int q = 0; q < KPL; ++q) {
                const int k = lane * KPL + q;
                w_n[q] = __dmul_rn(k < K ? col[k] : 0.0, inv[q]);
            }
        }
        for (int i = 0; i < cn; ++i, ++n) {
            // 1. the prefix, 64 tokens at a time: lane l holds token base + l's topic and uniform
            if (a.resample && n > 0) {
                uint32_t tk = 0;
                int zc = 0;
                double uc = 0.0;
                double w_r[KPL], w_nx[KPL];
#pragma unroll
                for (int q = 0; q < KPL; ++q) {
                    const int k = lane * KPL + q;
                    w_nx[q] = k < K ? a.lambda[(size_t)a.ids[e0] * K + k] : 0.0;
                }
                for (int j = e0; j <= jn; ++j) {
                    const int c = j == jn ? i : max(a.cnts[j], 0);
#pragma unroll
                    for (int q = 0; q < KPL; ++q)
                        w_r[q] = __dmul_rn(w_nx[q], inv[q]);
                    if (j < jn) {
                        const double *nx = a.lambda + (size_t)a.ids[j + 1] * K;
#pragma unroll
                        for (int q = 0; q < KPL; ++q) {
                            const int k = lane * KPL + q;
                            w_nx[q] = k < K ? nx[k] : 0.0;
                        }
                    }
                    for (int t = 0; t < c; ++t, ++tk) {
                        const int ql = (int)(tk & (kWave - 1));
                        if (ql == 0) {
                            if (tk > 0)                         // the chunk behind: its topics back
                                z[tk - kWave + lane] = (uint16_t)zc;
                            const uint32_t idx = tk + lane;
                            uint32_t rw[4];
                            philox_block(rw, idx, n, c2, kL2rPrefix, k0, k1);
                            uc = philox_u(rw[0], rw[1]);
                            zc = idx < n ? (int)z[idx] : 0;
                        }
                        const int zold = __builtin_amdgcn_readlane(zc, ql);
                        double p[KPL];
#pragma unroll
                        for (int q = 0; q < KPL; ++q) {
                            if (lane * KPL + q == zold)
                                n_r[q] -= 1;
                            p[q] = __dmul_rn(w_r[q], __dadd_rn(al[q], (double)n_r[q]));
                        }
                        double total;
                        int znew = histogram_draw<KPL>(p, readlane_d(uc, ql), lane, total);
                        if (znew < 0) {
                            bad = true;
                            znew = zold;
                        }
#pragma unroll
                        for (int q = 0; q < KPL; ++q)
                            if (lane * KPL + q == znew)
                                n_r[q] += 1;
                        if (lane == ql)
                            zc = znew;
                    }
                }
                // the last chunk (tk = n > 0 here)
                const uint32_t idx = ((tk - 1) & ~(uint32_t)(kWave - 1)) + lane;
                if (idx < n)
                    z[idx] = (uint16_t)zc;
            }
            // 2. the new token; the uniforms of 64 positions at a time
            const int qn = (int)(n & (kWave - 1));
            if (qn == 0) {
                uint32_t rw[4];
                philox_block(rw, n + lane, n + lane, c2, kL2rToken, k0, k1);
                un = philox_u(rw[0], rw[1]);
            }
            double p[KPL];
#pragma unroll
            for (int q = 0; q < KPL; ++q)
                p[q] = __dmul_rn(w_n[q], __dadd_rn(al[q], (double)n_r[q]));
            double total;
            int zn = histogram_draw<KPL>(p, readlane_d(un, qn), lane, total);
            if (zn < 0) {
                bad = true;
                zn = 0;
            }
            // 3.
#pragma unroll
            for (int q = 0; q < KPL; ++q)
                if (lane * KPL + q == zn)
                    n_r[q] += 1;
            if (lane == qn) {
                if (a.resample)
                    z[n] = (uint16_t)zn;
                pt[(size_t)n * R] = __ddiv_rn(total, __dadd_rn(A, (double)n));
            }
        }
    }
    if (bad && lane == 0)
        atomicOr(a.flag, 1);
}

// grid: the group's documents; a wave each
__global__ __launch_bounds__(kWave) void l2r_finish_kernel(int R, int position, const int32_t *__restrict__ docs,
                                                           const int64_t *__restrict__ off,
                                                           const int64_t *__restrict__ tokens, double *p,
                                                           double *__restrict__ loglik)
{
#pragma clang fp contract(off)
    const int doc = docs[blockIdx.x];
    const int lane = threadIdx.x;
    const int64_t N = tokens[doc];
    if (N == 0) {
        if (lane == 0)
            loglik[doc] = 0.0;
        return;
    }
    double *tab = p + (size_t)off[doc] * R;
    if (position) {
        double acc = 0.0;
        for (int64_t c0 = 0; c0 < N; c0 += kWave) {
            const int64_t n = c0 + lane;
            double term = 0.0;
            if (n < N) {
                const double *row = tab + (size_t)n * R;
                double s = row[0];
                for (int r = 1; r < R; ++r)
                    s = s + row[r];
                term = log(s / (double)R);
            }
            const int cnt = (int)min((int64_t)kWave, N - c0);
            for (int j = 0; j < cnt; ++j)
                acc = acc + readlane_d(term, j);
        }
        if (lane == 0)
            loglik[doc] = acc;
        return;
    }
    // L_r into row 0 of the table, column r: only lane r mod 64 reads or writes column r before the barrier
    for (int r = lane; r < R; r += kWave) {
        double L = 0.0;
        for (int64_t n = 0; n < N; ++n)
            L = L + log(tab[(size_t)n * R + r]);
        tab[r] = L;
    }
    __syncthreads();
    if (lane == 0) {
        double M = tab[0];
        for (int r = 1; r < R; ++r)
            M = fmax(M, tab[r]);
        double S = 0.0;
        for (int r = 0; r < R; ++r)
            S = S + exp(tab[r] - M);
        loglik[doc] = M == -INFINITY ? -INFINITY : (M + log(S)) - log((double)R);
    }
}

}  // namespace trlda
