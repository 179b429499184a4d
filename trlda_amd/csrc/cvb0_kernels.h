// cvb0_kernels.h -- HIP kernels for gfx950 (MI355X): collapsed variational Bayes, zero order
// (CVB0; Asuncion, Welling, Smyth & Teh, "On smoothing and inference for topic models", UAI 2009,
// with the document-side update of Foulds, Boyles, DuBois, Smyth & Welling, "Stochastic collapsed
// variational Bayesian inference for latent Dirichlet allocation", KDD 2013) of a mini-batch's
// documents on fixed topics, one wave64 per document.  The reference has no counterpart.  It is
// the deterministic form of the conditional gibbs_kernels.h samples from: a token's topic count is
// replaced by its expectation.  Host side: trlda_hip.hip, cvb0_device.
//
// Launch sequence of one call:
//   1. the Gibbs path's preamble on the Gibbs path's buffers (gibbs_preamble):
//      e = exp(psi(lambda) - psi(rowsum(lambda))), NORMALISED, K x V, the batch's active words --
//      trlda_debug_gibbs_table returns what the kernels here read
//   2. per slab of documents (batch order; the slab's phi fits the cap, below):
//      cvb0_docs_kernel<KPL>  per document: init, the sweeps, theta, the iteration count
//      cvb0_stats_kernel      per active word: its column of sstats continued over the slab's entries
//
// ---- the contract (tests/cvb0_host.py restates it step by step) ------------------------------
// A document d has entries p = 0 .. n_d - 1 with word w_p and count c_p; entries with c_p <= 0 are
// skipped (as the Gibbs path skips them).  State: one phi_p (K doubles) per entry and
// n_k = sum_p c_p phi_pk; N_d = sum_p c_p over the kept entries.
// Lane l of the document's wave holds topics l*KPL .. l*KPL + KPL - 1 (KPL as on the Gibbs path:
// the power of two >= K / 64; K <= 1024); topics >= K contribute 0.  "Wave sum": the lane-local
// sequential sum over its KPL topics (from 0, topics ascending), then wave_allsum's butterfly (xor
// 32, 16, .., 1).  Every +, -, x and / below is ONE rounded fp64 operation; nothing is contracted
// into an FMA.  The kernels write them as plain operators under `fp contract(off)`: that is what
// keeps a product and the sum it feeds apart -- hipcc's __dadd_rn(__dmul_rn(a, b), c) is inlined as
// two contractable operations and comes out as one v_fmac_f64 even under the pragma.
//   init    theta0 = column d of the caller's latents, else alpha (unnormalised).  Entries in order:
//             a_k = theta0_k x e[k, w_p];  s = wave sum of a;  inv = 1 / s;  phi_pk = a_k x inv;
//             n_k = n_k + c_p x phi_pk                                        (n starts at 0)
//   sweep   s = 1 .. max_iter, Gauss-Seidel over the entries in their stored order:
//             t_k = n_k - phi_pk                 (ONE token's own contribution, not c_p of them)
//             a_k = (alpha_k + t_k) x e[k, w_p]
//             S = wave sum of a;  inv = 1 / S;  phi'_k = a_k x inv
//             n_k = (n_k - c_p x phi_pk) + c_p x phi'_k;  phi_p = phi'
//   stop    after a sweep delta = (wave sum of |n_k - nprev_k|) / K, nprev = n before the sweep;
//           the sweeps end once delta < threshold (the VI loop's form).  The iteration count is the
//           number of sweeps done: max_iter = 0 returns the init state, threshold = 0 runs exactly
//           max_iter sweeps.
//   theta   theta_k = (alpha_k + n_k) / (wave sum of alpha + N_d).  A document without a kept
//           entry: theta = alpha / wave sum of alpha, 0 iterations.
//   sstats  sstats[k, w] = sum of c_p x phi_pk over the word's entries in the word-major order of
//           the batch index (document order, then entry order): each term one product, added
//           sequentially from 0.  Words outside the batch get 0.  Expected counts, like the Gibbs
//           statistics -- not multiplied by exp E[log beta].  No atomics.
//   failure a normaliser (s, S) that is not > 0 or not finite sets `flag`; the call then fails.
// Nothing of the result depends on the launch geometry, the wave a document lands on, the order
// the documents are worked off, the stream, or the slab partition: a slab's statistics continue
// the sums the earlier slabs stored, which is the same sequence of additions.
//
// phi lives in a global scratch laid out [entry of the slab][K]: a lane reads and writes its KPL
// contiguous doubles, always the same lane the same addresses.  An entry's e column and old phi
// row do not depend on n, so the next entry's loads are issued before this entry's reduction (and
// the word id and count they need were read an entry earlier still).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gibbs_kernels.h"

namespace trlda {

struct Cvb0Args {
    int K, n_docs, max_iter;
    double threshold;
    const int32_t *indptr, *ids, *cnts;
    const int32_t *order;        // the slab's documents, most entries first (n_docs of them)
    int32_t j0;                  // CSR position of the slab's first entry: phi row p is entry j0 + p
    const double *eeb;           // K x V, normalised; the batch's active columns
    const double *alpha;         // K
    const double *theta0;        // K x B, or nullptr: alpha
    double *theta;               // K x B
    int32_t *iters;              // B, or nullptr
    double *phi;                 // [entries of the slab][K]
    int *flag;                   // set to 1 by a normaliser that is not > 0 or not finite
};

// wave_allsum's butterfly -- v + (lane ^ 32's v), then xor 16, 8, 4, 2, 1, the same pairs in the
// same order, so the same bits in every lane -- without the LDS round trip of a shuffle where the
// hardware has a register path: the half- and row-exchanges of gfx950 (v_permlane32_swap,
// v_permlane16_swap; with both operands the same value the two results are the pair's members),
// a rotation by half a row of 16 (xor 8), a swizzle (xor 4) and quad permutations (xor 2, 1).
// An entry update of cvb0_docs_kernel is one such sum and one division long.
__device__ __forceinline__ double cvb0_allsum(double v)
{
#pragma clang fp contract(off)
    typedef unsigned int u32;
    {
        const u32 lo = (u32)__double2loint(v), hi = (u32)__double2hiint(v);
        const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        v = __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
    }
    {
        const u32 lo = (u32)__double2loint(v), hi = (u32)__double2hiint(v);
        const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        v = __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
    }
    {
        const int lo = __double2loint(v), hi = __double2hiint(v);       // row_ror:8
        v = v + __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0x128, 0xF, 0xF, true),
                                 __builtin_amdgcn_update_dpp(0, lo, 0x128, 0xF, 0xF, true));
    }
    {
        const int lo = __double2loint(v), hi = __double2hiint(v);       // and 0x1F, or 0, xor 4
        v = v + __hiloint2double(__builtin_amdgcn_ds_swizzle(hi, 0x101F), __builtin_amdgcn_ds_swizzle(lo, 0x101F));
    }
    {
        const int lo = __double2loint(v), hi = __double2hiint(v);       // quad_perm [2, 3, 0, 1]
        v = v + __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xF, 0xF, true),
                                 __builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xF, 0xF, true));
    }
    {
        const int lo = __double2loint(v), hi = __double2hiint(v);       // quad_perm [1, 0, 3, 2]
        v = v + __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xF, 0xF, true),
                                 __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xF, 0xF, true));
    }
    return v;
}

// lane-local sequential sum (from 0, topics ascending), then the butterfly
template <int KPL>
__device__ __forceinline__ double cvb0_wave_sum(const double (&v)[KPL])
{
#pragma clang fp contract(off)
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < KPL; ++q)
        s = s + v[q];
    return cvb0_allsum(s);
}

// a lane's KPL doubles of a K-long row (0 for topics >= K)
template <int KPL>
__device__ __forceinline__ void cvb0_load(double (&out)[KPL], const double *row, int k0, int K)
{
#pragma unroll
    for (int q = 0; q < KPL; ++q)
        out[q] = k0 + q < K ? row[k0 + q] : 0.0;
}

// rank in word-major order -> CSR position (the inverse of the batch index's wrank)
template <int T>
__global__ __launch_bounds__(T) void cvb0_wpos_kernel(int nnz, const int32_t *__restrict__ wrank,
                                                      int32_t *__restrict__ wpos)
{
    const int j = blockIdx.x * T + threadIdx.x;
    if (j < nnz)
        wpos[wrank[j]] = j;
}

// One wave per document, kGibbsWaves documents per workgroup; the waves never wait for each other.
template <int KPL>
__global__ __launch_bounds__(kGibbsWaves * kWave) void cvb0_docs_kernel(Cvb0Args a)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int slot = blockIdx.x * kGibbsWaves + wv;
    if (slot >= a.n_docs)
        return;
    const int K = a.K, k0 = lane * KPL;
    const int doc = a.order[slot];
    const int e0 = a.indptr[doc], e1 = a.indptr[doc + 1];
    double *phi = a.phi + (size_t)(e0 - a.j0) * K;       // the document's rows; its own lanes' only

    double al[KPL], n[KPL];
    cvb0_load<KPL>(al, a.alpha, k0, K);
#pragma unroll
    for (int q = 0; q < KPL; ++q)
        n[q] = 0.0;
    bool bad = false;
    int64_t Nd = 0;

    // init: the next entry's column is loaded while this one is reduced
    {
        double th[KPL], e_nx[KPL];
        if (a.theta0)
            cvb0_load<KPL>(th, a.theta0 + (size_t)doc * K, k0, K);
        else {
#pragma unroll
            for (int q = 0; q < KPL; ++q)
                th[q] = al[q];
        }
        int c_nx = 0, c_n2 = 0, w_n2 = 0;                // (w_n2, c_n2): the entry after the one in e_nx
        if (e0 < e1) {
            c_nx = a.cnts[e0];
            cvb0_load<KPL>(e_nx, a.eeb + (size_t)a.ids[e0] * K, k0, K);
        }
        if (e0 + 1 < e1) {
            c_n2 = a.cnts[e0 + 1];
            w_n2 = a.ids[e0 + 1];
        }
        for (int j = e0; j < e1; ++j) {
            const int c = c_nx;
            double v[KPL];
#pragma unroll
            for (int q = 0; q < KPL; ++q)
                v[q] = th[q] * e_nx[q];
            if (j + 1 < e1) {
                c_nx = c_n2;
                cvb0_load<KPL>(e_nx, a.eeb + (size_t)w_n2 * K, k0, K);
            }
            if (j + 2 < e1) {
                c_n2 = a.cnts[j + 2];
                w_n2 = a.ids[j + 2];
            }
            if (c <= 0)
                continue;
            const double s = cvb0_wave_sum<KPL>(v);
            bad |= !(s > 0.0 && s <= 1.7976931348623157e308);
            const double inv = 1.0 / s;
            const double cd = (double)c;
            double *row = phi + (size_t)(j - e0) * K;
#pragma unroll
            for (int q = 0; q < KPL; ++q) {
                v[q] = v[q] * inv;
                n[q] = n[q] + cd * v[q];
                if (k0 + q < K)
                    row[k0 + q] = v[q];
            }
            Nd += c;
        }
    }

    // sweeps
    int it = 0;
    if (Nd > 0) {
        const double Kd = (double)K;
        while (it < a.max_iter) {
            double nprev[KPL], e_nx[KPL], p_nx[KPL];
#pragma unroll
            for (int q = 0; q < KPL; ++q) {
                nprev[q] = n[q];
                p_nx[q] = 0.0;
            }
            int c_nx = a.cnts[e0], c_n2 = 0, w_n2 = 0;
            cvb0_load<KPL>(e_nx, a.eeb + (size_t)a.ids[e0] * K, k0, K);
            if (c_nx > 0)
                cvb0_load<KPL>(p_nx, phi, k0, K);
            if (e0 + 1 < e1) {
                c_n2 = a.cnts[e0 + 1];
                w_n2 = a.ids[e0 + 1];
            }
            for (int j = e0; j < e1; ++j) {
                const int c = c_nx;
                double e_r[KPL], p_r[KPL];
#pragma unroll
                for (int q = 0; q < KPL; ++q) {
                    e_r[q] = e_nx[q];
                    p_r[q] = p_nx[q];
                }
                if (j + 1 < e1) {
                    c_nx = c_n2;
                    cvb0_load<KPL>(e_nx, a.eeb + (size_t)w_n2 * K, k0, K);
                    if (c_nx > 0)
                        cvb0_load<KPL>(p_nx, phi + (size_t)(j + 1 - e0) * K, k0, K);
                }
                if (j + 2 < e1) {
                    c_n2 = a.cnts[j + 2];
                    w_n2 = a.ids[j + 2];
                }
                if (c <= 0)
                    continue;
                double v[KPL];
#pragma unroll
                for (int q = 0; q < KPL; ++q) {
                    const double t = n[q] - p_r[q];
                    v[q] = (al[q] + t) * e_r[q];
                }
                const double S = cvb0_wave_sum<KPL>(v);
                bad |= !(S > 0.0 && S <= 1.7976931348623157e308);
                const double inv = 1.0 / S;
                const double cd = (double)c;
                double *row = phi + (size_t)(j - e0) * K;
#pragma unroll
                for (int q = 0; q < KPL; ++q) {
                    v[q] = v[q] * inv;
                    n[q] = (n[q] - cd * p_r[q]) + cd * v[q];
                    if (k0 + q < K)
                        row[k0 + q] = v[q];
                }
            }
            ++it;
            double dv[KPL];
#pragma unroll
            for (int q = 0; q < KPL; ++q)
                dv[q] = fabs(n[q] - nprev[q]);
            const double delta = cvb0_wave_sum<KPL>(dv) / Kd;
            if (delta < a.threshold)
                break;
        }
    }
    if (bad && lane == 0)
        atomicOr(a.flag, 1);

    // theta
    const double denom = cvb0_wave_sum<KPL>(al) + (double)Nd;
#pragma unroll
    for (int q = 0; q < KPL; ++q)
        if (k0 + q < K)
            a.theta[(size_t)doc * K + k0 + q] = (al[q] + n[q]) / denom;
    if (a.iters && lane == 0)
        a.iters[doc] = it;
}

// The statistics of one slab: `gsz` threads (a power of two <= 64) per active word, thread t of a
// group taking topics t, t + gsz, ..  A word's list is walked in word-major order; its entries of
// the slab, CSR positions [j0, j1), continue the column's sums where the earlier slabs left them
// (the caller zeroes sstats before the first slab: 0 + x is x).
template <int T>
__global__ __launch_bounds__(T) void cvb0_stats_kernel(int K, int n_active, int gsz,
                                                       const int32_t *__restrict__ active,
                                                       const int32_t *__restrict__ wptr,
                                                       const int32_t *__restrict__ wpos,
                                                       const int32_t *__restrict__ cnts, int32_t j0, int32_t j1,
                                                       const double *__restrict__ phi, double *__restrict__ sstats)
{
#pragma clang fp contract(off)
    const int per = T / gsz;
    const int kp = threadIdx.x & (gsz - 1);
    for (int i = blockIdx.x * per + threadIdx.x / gsz; i < n_active; i += gridDim.x * per) {
        const int w = active[i];
        const int r0 = wptr[w], r1 = wptr[w + 1];
        for (int k = kp; k < K; k += gsz) {
            double acc = sstats[(size_t)w * K + k];
            for (int r = r0; r < r1; ++r) {
                const int j = wpos[r];
                if (j < j0 || j >= j1)
                    continue;
                const int c = cnts[j];
                if (c > 0)
                    acc = acc + (double)c * phi[(size_t)(j - j0) * K + k];
            }
            sstats[(size_t)w * K + k] = acc;
        }
    }
}

}  // namespace trlda
