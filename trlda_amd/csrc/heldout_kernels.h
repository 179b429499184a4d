// trlda_amd/csrc/heldout_kernels.h -- the held-out predictive log-likelihood (Hoffman et al. 2013,
// SVI section 4): after an E-step on the observed part of each document, the held-out words of the
// document are scored with the means of the variational posteriors,
//   p(w | d) ~= sum_k E[theta_dk] E[beta_kw] = sum_k (gamma_dk / sum_j gamma_dj) (lambda_kw / rs_k),
// rs_k = sum_v lambda_kv (the row sums the E-step's preamble left at psi_sum + K).
//
// One workgroup per document; its K factors gamma_dk / rs_k are formed once, in LDS (K doubles:
// less than the general E-step kernel holds for the same K, so every K the E-step takes fits).
// Each wave takes one held-out entry at a time -- entry p goes to wave (p - first entry) mod W --
// and reads the word's column of lambda (K contiguous doubles) coalesced, lane k mod 64 at a time;
// the dot product is reduced with wave_sum_dpp.  The order of every addition is fixed by K, T and
// the document's own entries, never by the grid, so a document's value does not depend on the
// batch it sits in.  DESIGN.md 3.12.
#pragma once

#include "estep_kernels.h"

namespace trlda {

constexpr int kHeldoutThreads = 256;

// loglik[d] = sum over the held-out entries (w, c) of c (log(sum_k f_k lambda_kw) - log sum_k gamma_dk),
// f_k = gamma_dk / rs_k; tokens[d] = sum of c.  Entries with c = 0 are skipped (no read, no log).
template <int T>
__global__ __launch_bounds__(T) void heldout_docs_kernel(int K, const int32_t *__restrict__ indptr,
                                                         const int32_t *__restrict__ ids,
                                                         const int32_t *__restrict__ cnts,
                                                         const double *__restrict__ lambda,
                                                         const double *__restrict__ rowsum,
                                                         const double *__restrict__ gamma,
                                                         double *__restrict__ loglik,
                                                         double *__restrict__ tokens)
{
    constexpr int W = T / kWave;
    extern __shared__ double fac[];                  // K factors
    __shared__ double red[2 * W];
    const int d = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const int p0 = indptr[d], p1 = indptr[d + 1];
    if (p0 >= p1) {                                  // (the whole workgroup: d is its own)
        if (threadIdx.x == 0) {
            loglik[d] = 0.0;
            tokens[d] = 0.0;
        }
        return;
    }
    const double *g = gamma + (size_t)d * K;
    double gs = 0.0;
    for (int k = threadIdx.x; k < K; k += T) {
        const double gk = g[k];
        gs += gk;
        fac[k] = gk / rowsum[k];
    }
    gs = wave_sum_dpp(gs);
    if (lane == 0)
        red[wid] = gs;
    __syncthreads();
    gs = 0.0;
    for (int w = 0; w < W; ++w)
        gs += red[w];
    const double log_gs = log(gs);
    __syncthreads();                                 // (red is written again below)

    double ll = 0.0, tok = 0.0;
    for (int p = p0 + wid; p < p1; p += W) {
        const int c = cnts[p];
        if (c == 0)                                  // (the wave's own entry: uniform)
            continue;
        const double *col = lambda + (size_t)ids[p] * K;
        double s = 0.0;
#pragma unroll 4
        for (int k = lane; k < K; k += kWave)
            s = fma(fac[k], col[k], s);
        s = wave_sum_dpp(s);
        ll += (double)c * (log(s) - log_gs);
        tok += (double)c;
    }
    if (lane == 0) {
        red[wid] = ll;
        red[W + wid] = tok;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < W; ++w) {
            a += red[w];
            b += red[W + w];
        }
        loglik[d] = a;
        tokens[d] = b;
    }
}

}  // namespace trlda
