// trlda_amd/csrc/marginal_kernels.h -- the marginal log-likelihood of a whole unseen document,
// log p(w_d | alpha, beta), by importance sampling of theta (Wallach, Murray, Salakhutdinov & Mimno
// 2009, section 4.1) with beta_kw = lambda_kw / rs_k, rs_k = sum_v lambda_kv (the point estimate of
// heldout_kernels.h).  The proposal is Dir(a_d): a_d = gamma_d of the fixed-lambda E-step on the
// whole document (proposal 'vi') or a_d = alpha ('prior').  Per document d with entries (w_i, c_i):
//
//   theta^(s) ~ Dir(a_d),  s = 0 .. S-1
//   log w_s = sum_i c_i log(sum_k theta^(s)_k beta_{k, w_i})
//             + C_d + sum_k (alpha_k - a_k) log theta^(s)_k                   ('vi' only)
//   C_d     = [lgamma(sum alpha) - sum lgamma(alpha_k)] - [lgamma(sum a) - sum lgamma(a_k)]
//   loglik_d = logsumexp_s(log w_s) - log S,   ess_d = (sum_s w_s)^2 / sum_s w_s^2
//
// Draws: lg_k = philox_log_gamma(a_k) with purposes 19 / 20 / 21 (normal / accept / boost) and
// counter (s K + k, d, attempt) under the call's key (S K < 2^32 is the caller's check).  log theta_k
// = lg_k - (mx + log sum_j exp(lg_j - mx)), mx = max_j lg_j: theta is never divided and then logged,
// so a tiny alpha gives a very negative log theta_k, never log 0.
//
// One workgroup of W waves per document.  Wave w takes the samples s = w, w + W, ..; lane l owns the
// topics k = q 64 + l, q < ceil(K / 64): it draws lg_k and keeps phi_k = theta_k (1 / rs_k) -- in
// registers for K <= 512 (KPL = ceil(K / 64) is a template argument), in the wave's own K doubles
// of LDS above that (KPL = 0).  That is the layout of a coalesced read of a word's column of
// lambda, so an entry's sum_k phi_k lambda_{k, w} is per-lane FMAs in order of q, then wave_sum_dpp.
// W = marginal_waves(K): 8 while the LDS holds that many rows of K doubles (K <= 2552), else as many
// as fit (2 at the E-step's bound K = 6814).  Eight waves leave each 256 registers: the draws
// (three fp64 logarithms, a cosine and two Philox blocks per attempt) spill at 128.
//
// The order of every addition is a function of K, S, W and the document alone:
//   sums over k       lane l adds its q in ascending order from 0, then wave_sum_dpp
//   the constants     thread t adds k = t, t + 64 W, .. from 0; wave_sum_dpp; the waves in order
//   log w_s           the entries in document order from 0 (c = 0 skipped), then + (C_d + the sum)
//   over the samples  per wave a running (m, s1, s2) = (max, sum exp(log w - m), sum exp(2 (log w
//                     - m))), rescaled when the max rises; thread 0 merges the waves in wave order
//                     against the overall max.  A sample of weight 0 (log w = -inf) adds nothing.
// Nothing depends on the grid, the batch or the other documents.  No product and sum is contracted
// into an FMA except the entries' dot products.  DESIGN.md 3.16.
#pragma once

#include "elbo_kernels.h"            // wave_sum_dpp (estep_kernels.h), wave_max_all
#include "philox.h"

namespace trlda {

enum : uint32_t {
    kMarginalNormal = 19,
    kMarginalAccept = 20,
    kMarginalBoost = 21,
};

constexpr int kMarginalMaxWaves = 8;
constexpr int kMarginalRegMaxK = 512;                              // KPL <= 8
constexpr int kMarginalAhead = 4;                                  // columns in flight per wave (K <= 512)
constexpr int kMarginalRedDoubles = 4 * kMarginalMaxWaves;         // the waves' partial results
constexpr int kMarginalLdsDoubles = (160 * 1024 - 256) / 8;        // what a launch may ask for

// waves per document workgroup
inline int marginal_waves(int K)
{
    if (K <= kMarginalRegMaxK)
        return kMarginalMaxWaves;
    const int fit = (kMarginalLdsDoubles - kMarginalRedDoubles) / K;
    return fit < kMarginalMaxWaves ? fit : kMarginalMaxWaves;
}

// dynamic LDS of a launch, in doubles
inline size_t marginal_lds_doubles(int K)
{
    return (size_t)kMarginalRedDoubles + (K <= kMarginalRegMaxK ? 0 : (size_t)marginal_waves(K) * K);
}

__device__ __forceinline__ double marginal_log_gamma(double a, uint32_t c0, uint32_t d, uint32_t key0,
                                                     uint32_t key1)
{
    return philox_log_gamma(a, c0, d, kMarginalNormal, kMarginalAccept, kMarginalBoost, key0, key1);
}

// gamma: K x B (the proposal's parameters) for 'vi', nullptr for 'prior' (the proposal is alpha and the
// two Dirichlet terms are dropped).  rowsum: K.  loglik, ess: B.
template <int KPL>
__global__ __launch_bounds__(kMarginalMaxWaves *kWave) void marginal_docs_kernel(
    int K, int S, uint32_t key0, uint32_t key1, const int32_t *__restrict__ indptr,
    const int32_t *__restrict__ ids, const int32_t *__restrict__ cnts, const double *__restrict__ lambda,
    const double *__restrict__ rowsum, const double *__restrict__ alpha, const double *__restrict__ gamma,
    double *__restrict__ loglik, double *__restrict__ ess)
{
#pragma clang fp contract(off)
    extern __shared__ double marginal_lds[];
    double *red = marginal_lds;                                    // kMarginalRedDoubles
    const int T = blockDim.x, W = T / kWave;
    const int d = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const int p0 = indptr[d], p1 = indptr[d + 1];
    if (p0 >= p1) {                                                // (the whole workgroup: d is its own)
        if (threadIdx.x == 0) {
            loglik[d] = 0.0;
            ess[d] = (double)S;
        }
        return;
    }
    const bool vi = gamma != nullptr;
    const double *a = vi ? gamma + (size_t)d * K : alpha;

    double C = 0.0;
    if (vi) {
        double sa = 0.0, la = 0.0, sg = 0.0, lg = 0.0;
        for (int k = threadIdx.x; k < K; k += T) {
            const double ak = alpha[k], gk = a[k];
            sa = sa + ak;
            la = la + lgamma(ak);
            sg = sg + gk;
            lg = lg + lgamma(gk);
        }
        sa = wave_sum_dpp(sa);
        la = wave_sum_dpp(la);
        sg = wave_sum_dpp(sg);
        lg = wave_sum_dpp(lg);
        if (lane == 0) {
            red[wid * 4] = sa;
            red[wid * 4 + 1] = la;
            red[wid * 4 + 2] = sg;
            red[wid * 4 + 3] = lg;
        }
        __syncthreads();
        sa = la = sg = lg = 0.0;
        for (int w = 0; w < W; ++w) {
            sa = sa + red[w * 4];
            la = la + red[w * 4 + 1];
            sg = sg + red[w * 4 + 2];
            lg = lg + red[w * 4 + 3];
        }
        C = (lgamma(sa) - la) - (lgamma(sg) - lg);
        __syncthreads();                                           // (red is written again below)
    }

    constexpr int R = KPL > 0 ? KPL : 1;
    [[maybe_unused]] double phi[R], irs[R];
    [[maybe_unused]] double *row = marginal_lds + kMarginalRedDoubles + (size_t)wid * K;   // KPL == 0: the wave's K doubles
    if constexpr (KPL > 0) {
#pragma unroll
        for (int q = 0; q < KPL; ++q) {
            const int k = q * kWave + lane;
            irs[q] = k < K ? 1.0 / rowsum[k] : 0.0;
        }
    }

    double m_run = -INFINITY, s1 = 0.0, s2 = 0.0;
    for (int s = wid; s < S; s += W) {
        const uint32_t c0 = (uint32_t)s * (uint32_t)K;
        double t = 0.0;
        if constexpr (KPL > 0) {
            double lg[KPL];
            double mx = -INFINITY;
#pragma unroll
            for (int q = 0; q < KPL; ++q) {
                const int k = q * kWave + lane;
                lg[q] = -INFINITY;
                if (k < K) {
                    lg[q] = marginal_log_gamma(a[k], c0 + (uint32_t)k, (uint32_t)d, key0, key1);
                    mx = fmax(mx, lg[q]);
                }
            }
            mx = wave_max_all(mx);
            double se = 0.0;
#pragma unroll
            for (int q = 0; q < KPL; ++q)
                if (q * kWave + lane < K)
                    se = se + exp(lg[q] - mx);
            const double lse = mx + log(wave_sum_dpp(se));
#pragma unroll
            for (int q = 0; q < KPL; ++q) {
                const int k = q * kWave + lane;
                phi[q] = 0.0;
                if (k < K) {
                    const double lt = lg[q] - lse;
                    if (vi)
                        t = t + (alpha[k] - a[k]) * lt;
                    phi[q] = exp(lt) * irs[q];
                }
            }
        } else {
            double mx = -INFINITY;
            for (int k = lane; k < K; k += kWave) {
                const double lg = marginal_log_gamma(a[k], c0 + (uint32_t)k, (uint32_t)d, key0, key1);
                row[k] = lg;
                mx = fmax(mx, lg);
            }
            mx = wave_max_all(mx);
            double se = 0.0;
            for (int k = lane; k < K; k += kWave)
                se = se + exp(row[k] - mx);
            const double lse = mx + log(wave_sum_dpp(se));
            for (int k = lane; k < K; k += kWave) {
                const double lt = row[k] - lse;
                if (vi)
                    t = t + (alpha[k] - a[k]) * lt;
                row[k] = exp(lt) * (1.0 / rowsum[k]);
            }
        }
        if (vi)
            t = wave_sum_dpp(t);

        double ll = 0.0;
        if constexpr (KPL > 0) {
            // lane j holds entry pc + j of a chunk of 64; kMarginalAhead entries' columns are loaded
            // before the first of them is reduced, so that the loads' latencies overlap (an entry with
            // c = 0 has its column read with the others, and adds nothing)
            for (int pc = p0; pc < p1; pc += kWave) {
                const int n = min(kWave, p1 - pc);
                const int my_id = lane < n ? ids[pc + lane] : 0, my_c = lane < n ? cnts[pc + lane] : 0;
                for (int j = 0; j < n; j += kMarginalAhead) {
                    double v[kMarginalAhead][KPL];
                    int c[kMarginalAhead];
#pragma unroll
                    for (int u = 0; u < kMarginalAhead; ++u) {
                        const int jj = min(j + u, n - 1);
                        c[u] = j + u < n ? __builtin_amdgcn_readlane(my_c, jj) : 0;
                        const double *col = lambda + (size_t)__builtin_amdgcn_readlane(my_id, jj) * K;
#pragma unroll
                        for (int q = 0; q < KPL; ++q) {
                            const int k = q * kWave + lane;
                            v[u][q] = k < K ? col[k] : 0.0;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < kMarginalAhead; ++u) {
                        if (c[u] == 0)                             // (the wave's own entry: uniform)
                            continue;
                        double acc = 0.0;
#pragma unroll
                        for (int q = 0; q < KPL; ++q)
                            acc = fma(phi[q], v[u][q], acc);       // (phi = 0 beyond K)
                        acc = wave_sum_dpp(acc);
                        ll = ll + (double)c[u] * log(acc);
                    }
                }
            }
        } else {
            for (int p = p0; p < p1; ++p) {
                const int c = cnts[p];
                if (c == 0)                                        // (the wave's own entry: uniform)
                    continue;
                const double *col = lambda + (size_t)ids[p] * K;
                double acc = 0.0;
#pragma unroll 4
                for (int k = lane; k < K; k += kWave)
                    acc = fma(row[k], col[k], acc);
                acc = wave_sum_dpp(acc);
                ll = ll + (double)c * log(acc);
            }
        }
        const double lw = vi ? ll + (C + t) : ll;
        if (lw == -INFINITY)                                       // (a weight of 0)
            continue;
        if (lw > m_run) {
            const double sc = exp(m_run - lw);                     // 0 on the first sample
            s1 = s1 * sc + 1.0;
            s2 = s2 * (sc * sc) + 1.0;
            m_run = lw;
        } else {
            const double e = exp(lw - m_run);
            s1 = s1 + e;
            s2 = s2 + e * e;
        }
    }
    if (lane == 0) {
        red[wid * 4] = m_run;
        red[wid * 4 + 1] = s1;
        red[wid * 4 + 2] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double M = -INFINITY;
        for (int w = 0; w < W; ++w)
            M = fmax(M, red[w * 4]);
        double A = 0.0, Q = 0.0;
        for (int w = 0; w < W; ++w) {
            const double mw = red[w * 4];
            if (mw == -INFINITY)                                   // (a wave without a sample of weight > 0)
                continue;
            const double sc = exp(mw - M);
            A = A + red[w * 4 + 1] * sc;
            Q = Q + red[w * 4 + 2] * (sc * sc);
        }
        const bool none = M == -INFINITY;
        loglik[d] = none ? -INFINITY : (M + log(A)) - log((double)S);
        ess[d] = none ? 0.0 : fmin(fmax((A * A) / Q, 1.0), (double)S);   // (its bounds, whatever the rounding)
    }
}

}  // namespace trlda
