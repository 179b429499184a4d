// trlda_amd/csrc/anchor_kernels.h -- spectral initialisation: the word co-occurrence matrix Q of a
// corpus stream, FastAnchorWords on its row-normalised form and RecoverL2 (Arora et al. 2013, "A practical
// algorithm for topic modeling with provable guarantees").  DESIGN.md 3.36.  No reference counterpart.
//
// Every floating-point result here is a fixed sequence of IEEE operations on its inputs: the kernels
// are compiled with contraction off and spell out the fused operations they want.
//
// The sum of a row (anchor_block_sum): thread t of the 256 adds the elements t, t + 256, t + 512, ...
// in ascending order, starting from +0; the 256 partial sums are folded as p[t] += p[t + s] for
// s = 128, 64, ..., 1.  Row sums, squared norms (of the rounded squares) and dot products (of the
// rounded products) all use it: each is a function of the row (and the pivot) alone.
#pragma once

#include "tile_product.h"

namespace trlda {

constexpr int kAnchorThreads = 256;
constexpr int kAnchorSolveWaves = kAnchorThreads / kWave;
constexpr int kAnchorGramLdsTopics = 128;     // up to here the solver keeps G in LDS (128 x 128 x 8 = 128 KiB)
constexpr int kAnchorMaxTopics = 640;         // 7 vectors x 4 waves x 640 x 8 = 140 KiB of LDS
constexpr int kAnchorSolveVectors = 7;        // x, y, x+, G x, G x+, G y, h

// one rounded operation each, wherever they are inlined (the operations carry no leave to contract)
__device__ __forceinline__ double anchor_add(double a, double b)
{
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ double anchor_sub(double a, double b)
{
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ double anchor_mul(double a, double b)
{
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double anchor_div(double a, double b)
{
#pragma clang fp contract(off)
    return a / b;
}

__device__ __forceinline__ double anchor_block_sum(double part, double *red, int tid)
{
    red[tid] = part;
    __syncthreads();
    for (int s = kAnchorThreads / 2; s > 0; s >>= 1) {
        if (tid < s)
            red[tid] = anchor_add(red[tid], red[tid + s]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();                                        // (red is used again)
    return r;
}

// ---- the accumulator -------------------------------------------------------------------------------

// A thread per document: docn[d] = the sum of its counts (none negative: the host has refused such a
// batch); counters += (1, 0, n) when n >= 2, else (0, 1, 0).
__global__ __launch_bounds__(kAnchorThreads) void anchor_docs_kernel(int B, const int32_t *__restrict__ indptr,
                                                                     const int32_t *__restrict__ cnts,
                                                                     long long *__restrict__ docn,
                                                                     unsigned long long *__restrict__ counters)
{
    const int d = blockIdx.x * kAnchorThreads + threadIdx.x;
    if (d >= B)
        return;
    long long n = 0;
    for (int p = indptr[d]; p < indptr[d + 1]; ++p)
        n += cnts[p];
    docn[d] = n;
    if (n >= 2) {
        atomicAdd(counters + 0, 1ull);
        atomicAdd(counters + 2, (unsigned long long)n);
    } else {
        atomicAdd(counters + 1, 1ull);
    }
}

// A thread per entry p: wpos[rank of p in the word-major order] = p; *flag = 1 when the entry
// before it in its word's list lies in the same document (a word listed twice in a document).
__global__ __launch_bounds__(kAnchorThreads) void anchor_entries_kernel(long long nnz, const int32_t *__restrict__ ids,
                                                                        const int32_t *__restrict__ wrank,
                                                                        const int32_t *__restrict__ wptr,
                                                                        const int32_t *__restrict__ wdoc,
                                                                        int32_t *__restrict__ wpos,
                                                                        int *__restrict__ flag)
{
    const long long p = (long long)blockIdx.x * kAnchorThreads + threadIdx.x;
    if (p >= nnz)
        return;
    const int r = wrank[p];
    wpos[r] = (int32_t)p;
    if (r > wptr[ids[p]] && wdoc[r - 1] == wdoc[r])
        atomicOr(flag, 1);
}

// Row w of Q, a workgroup: the entries of w's list in their order (documents ascending), and for
// each the document's entries spread over the threads -- a document lists a word once, so no two
// threads meet in an element, and the barrier orders one document's additions before the next one's.
// Grid V.
__global__ __launch_bounds__(kAnchorThreads) void anchor_cooc_rows_kernel(
    int Vp, const int32_t *__restrict__ indptr, const int32_t *__restrict__ ids, const int32_t *__restrict__ cnts,
    const int32_t *__restrict__ wptr, const int32_t *__restrict__ wdoc, const int32_t *__restrict__ wpos,
    const long long *__restrict__ docn, double *__restrict__ Q, long long *__restrict__ doc_freq,
    long long *__restrict__ word_count)
{
    const int w = blockIdx.x, tid = threadIdx.x;
    const int e0 = wptr[w], e1 = wptr[w + 1];
    double *row = Q + (size_t)w * Vp;
    long long df = 0, wc = 0;
    for (int e = e0; e < e1; ++e) {                         // (uniform)
        const int d = wdoc[e];
        const long long n = docn[d];
        if (n < 2)
            continue;
        const int p = wpos[e];
        const long long c = cnts[p];
        if (c > 0) {
            ++df;
            wc += c;
        }
        const double denom = (double)(n * (n - 1));
        for (int f = indptr[d] + tid; f < indptr[d + 1]; f += kAnchorThreads) {
            const long long num = c * (long long)cnts[f] - (f == p ? c : 0);
            const int v = ids[f];
            row[v] = anchor_add(row[v], anchor_div((double)num, denom));
        }
        __syncthreads();
    }
    if (tid == 0 && e1 > e0) {
        doc_freq[w] += df;
        word_count[w] += wc;
    }
}

// out[i] = the sum of the n elements of row i of src (row stride `stride`).  Grid rows.
__global__ __launch_bounds__(kAnchorThreads) void anchor_sums_kernel(int n, int stride, const double *__restrict__ src,
                                                                     double *__restrict__ out)
{
    __shared__ double red[kAnchorThreads];
    const double *row = src + (size_t)blockIdx.x * stride;
    double part = 0.0;
    for (int v = threadIdx.x; v < n; v += kAnchorThreads)
        part = anchor_add(part, row[v]);
    const double s = anchor_block_sum(part, red, threadIdx.x);
    if (threadIdx.x == 0)
        out[blockIdx.x] = s;
}

// ---- FastAnchorWords -------------------------------------------------------------------------------

// W_w = Q_w / r_w (a zero row where r_w is not positive), norm2[w] = |W_w|^2.  Grid V.
__global__ __launch_bounds__(kAnchorThreads) void anchor_normalise_kernel(int V, int Vp, const double *__restrict__ Q,
                                                                          const double *__restrict__ r,
                                                                          double *__restrict__ W,
                                                                          double *__restrict__ norm2)
{
    __shared__ double red[kAnchorThreads];
    const int w = blockIdx.x, tid = threadIdx.x;
    const double rw = r[w];
    const double *q = Q + (size_t)w * Vp;
    double *x = W + (size_t)w * Vp;
    double part = 0.0;
    for (int v = tid; v < Vp; v += kAnchorThreads) {
        const double y = (v < V && rw > 0.0) ? anchor_div(q[v], rw) : 0.0;
        x[v] = y;
        if (v < V)
            part = anchor_add(part, anchor_mul(y, y));
    }
    const double s = anchor_block_sum(part, red, tid);
    if (tid == 0)
        norm2[w] = s;
}

// cand[w] = whether word w is a candidate: r_w > 0 and, with min_df >= 0, doc_freq[w] >= min_df
__global__ __launch_bounds__(kAnchorThreads) void anchor_candidates_kernel(int V, long long min_df,
                                                                           const double *__restrict__ r,
                                                                           const long long *__restrict__ doc_freq,
                                                                           int *__restrict__ cand)
{
    const int w = blockIdx.x * kAnchorThreads + threadIdx.x;
    if (w < V)
        cand[w] = (r[w] > 0.0 && (min_df < 0 || doc_freq[w] >= min_df)) ? 1 : 0;
}

// the first of the candidates other than `skip` in the order (norm2 descending, id ascending); -1 if none
__device__ __forceinline__ int anchor_argmax(int V, const double *norm2, const int *cand, int skip, double *bv,
                                             int *bi, int tid, double *value)
{
    double v = -1.0;
    int i = INT_MAX;
    for (int w = tid; w < V; w += kAnchorThreads)
        if (cand[w] && w != skip && docindex_before(norm2[w], w, v, i)) {
            v = norm2[w];
            i = w;
        }
    bv[tid] = v;
    bi[tid] = i;
    __syncthreads();
    for (int s = kAnchorThreads / 2; s > 0; s >>= 1) {
        if (tid < s && docindex_before(bv[tid + s], bi[tid + s], bv[tid], bi[tid])) {
            bv[tid] = bv[tid + s];
            bi[tid] = bi[tid + s];
        }
        __syncthreads();
    }
    const int a = bi[0];
    *value = bv[0];
    __syncthreads();
    return a == INT_MAX ? -1 : a;
}

// Round `round`: the winner a and the runner-up among the candidates, a leaves the candidates, and the
// pivot u = W_a (round 0) or W_a / sqrt(norm2[a]) (later).  One workgroup.
__global__ __launch_bounds__(kAnchorThreads) void anchor_pick_kernel(int V, int Vp, int round,
                                                                     const double *__restrict__ W,
                                                                     const double *__restrict__ norm2,
                                                                     int *__restrict__ cand, double *__restrict__ u,
                                                                     int32_t *__restrict__ out_ids,
                                                                     double *__restrict__ out_score,
                                                                     double *__restrict__ out_runner)
{
    __shared__ double bv[kAnchorThreads];
    __shared__ int bi[kAnchorThreads];
    const int tid = threadIdx.x;
    double score, runner;
    const int a = anchor_argmax(V, norm2, cand, -1, bv, bi, tid, &score);
    if (a < 0)                                              // (the host has counted the candidates)
        return;
    const int b = anchor_argmax(V, norm2, cand, a, bv, bi, tid, &runner);
    if (tid == 0) {
        out_ids[round] = a;
        out_score[round] = score;
        out_runner[round] = b < 0 ? -1.0 : runner;
        cand[a] = 0;
    }
    const double nrm = sqrt(score);
    const double *x = W + (size_t)a * Vp;
    for (int v = tid; v < Vp; v += kAnchorThreads)
        u[v] = round == 0 ? x[v] : (nrm > 0.0 ? anchor_div(x[v], nrm) : 0.0);
}

// Every candidate row: W_w -= u (first) or W_w -= (W_w . u) u, then norm2[w] = |W_w|^2.  Grid V.
__global__ __launch_bounds__(kAnchorThreads) void anchor_update_kernel(int V, int Vp, int first,
                                                                       double *__restrict__ W,
                                                                       const int *__restrict__ cand,
                                                                       const double *__restrict__ u,
                                                                       double *__restrict__ norm2)
{
    __shared__ double red[kAnchorThreads];
    const int w = blockIdx.x, tid = threadIdx.x;
    if (!cand[w])                                           // (uniform)
        return;
    double *x = W + (size_t)w * Vp;
    double dot = 1.0;
    if (!first) {
        double part = 0.0;
        for (int v = tid; v < V; v += kAnchorThreads)
            part = anchor_add(part, anchor_mul(x[v], u[v]));
        dot = anchor_block_sum(part, red, tid);
    }
    double part = 0.0;
    for (int v = tid; v < V; v += kAnchorThreads) {
        const double y = anchor_sub(x[v], first ? u[v] : anchor_mul(dot, u[v]));
        x[v] = y;
        part = anchor_add(part, anchor_mul(y, y));
    }
    const double s = anchor_block_sum(part, red, tid);
    if (tid == 0)
        norm2[w] = s;
}

// ---- RecoverL2 -------------------------------------------------------------------------------------

// H[w * A + k] = W_w . W_{anchors[k]}: the staged tile product over the Vp columns in ascending chunks.
// Grid ceil(V / 64), 4 waves; dynamic LDS tile_operands_lds(64).
__global__ __launch_bounds__(kAnchorThreads) void anchor_product_kernel(int V, int Vp, int A,
                                                                        const double *__restrict__ W,
                                                                        const int32_t *__restrict__ anchors,
                                                                        double *__restrict__ H)
{
    extern __shared__ __attribute__((aligned(16))) double anchor_lds[];
    __shared__ int anc[64];
    double *x_lds = anchor_lds;                             // 64 x S
    double *y_lds = x_lds + 64 * kDocIndexStride;           // 64 x S
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int m = lane & 15, kq = lane >> 4;
    const int w0 = blockIdx.x * 64;
    for (int g0 = 0; g0 < A; g0 += 64) {
        __syncthreads();                                    // the previous group's ids have been read
        if (tid < 64)
            anc[tid] = anchors[min(g0 + tid, A - 1)];
        docindex_f64x4 acc[1][4] = {};
        for (int k0 = 0; k0 < Vp; k0 += kDocIndexChunk) {
            const int cl = min(kDocIndexChunk, Vp - k0);    // a multiple of 4
            __syncthreads();                                // the previous chunk has been read
            tile_stage<64, kAnchorThreads>(x_lds, W, Vp, k0, cl, tid, [&](int row) { return min(w0 + row, V - 1); });
            tile_stage<64, kAnchorThreads>(y_lds, W, Vp, k0, cl, tid, [&](int row) { return anc[row]; });
            __syncthreads();
            for (int kk = 0; kk < cl; kk += 4)
                tile_step<1>(acc, x_lds, y_lds, kk, wid, m, kq);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int w = w0 + wid * 16 + kq + 4 * r, k = g0 + j * 16 + m;
                if (w < V && k < A)
                    H[(size_t)w * A + k] = acc[0][j][r];
            }
    }
}

// G[i * A + j] = H[anchors[i] * A + j] and *L = 2 max_i sum_j |G_ij| (each row's sum over j ascending).
// One workgroup.
__global__ __launch_bounds__(kAnchorThreads) void anchor_gram_kernel(int A, const double *__restrict__ H,
                                                                     const int32_t *__restrict__ anchors,
                                                                     double *__restrict__ G, double *__restrict__ L)
{
    __shared__ double red[kAnchorThreads];
    const int tid = threadIdx.x;
    double mx = 0.0;
    for (int i = tid; i < A; i += kAnchorThreads) {
        const double *h = H + (size_t)anchors[i] * A;
        double s = 0.0;
        for (int j = 0; j < A; ++j) {
            G[(size_t)i * A + j] = h[j];
            s = anchor_add(s, fabs(h[j]));
        }
        mx = fmax(mx, s);
    }
    red[tid] = mx;
    __syncthreads();
    for (int s = kAnchorThreads / 2; s > 0; s >>= 1) {
        if (tid < s)
            red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0)
        *L = 2.0 * red[0];
}

__device__ __forceinline__ void anchor_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the same bits in every lane: each step adds two values that the partner lanes both hold
__device__ __forceinline__ double anchor_wave_sum(double v)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1)
        v = anchor_add(v, __shfl_xor(v, off, kWave));
    return v;
}

__device__ __forceinline__ double anchor_wave_min(double v)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1)
        v = fmin(v, __shfl_xor(v, off, kWave));
    return v;
}

__device__ __forceinline__ int anchor_wave_count(int v)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1)
        v += __shfl_xor(v, off, kWave);
    return v;
}

// out_k = sum_j G[j * A + k] v_j (G is symmetric bit for bit), j ascending, one fma each; lane l
// forms k = l, l + 64, ...
__device__ __forceinline__ void anchor_matvec(int A, const double *G, const double *v, double *out, int lane)
{
    for (int k = lane; k < A; k += kWave) {
        double acc = 0.0;
        for (int j = 0; j < A; ++j)
            acc = fma(G[(size_t)j * A + k], v[j], acc);
        out[k] = acc;
    }
}

// The Euclidean projection of v (A values, in place) onto the simplex by Michelot's iteration: tau =
// (sum of the active - 1) / their number, whoever is not above tau leaves, until nobody does -- at
// most A rounds, no tolerance.  One more step on tau takes the rounding of the sum out:
// tau += (sum of the active (v - tau) - 1) / their number.
__device__ __forceinline__ void anchor_project(int A, double *v, int lane)
{
#pragma clang fp contract(off)
    unsigned act = 0xffffffffu;                             // bit i: element lane + 64 i is active
    int m = A;
    double tau;
    for (;;) {                                              // (uniform)
        double part = 0.0;
        for (int k = lane, i = 0; k < A; k += kWave, ++i)
            if (act >> i & 1)
                part = anchor_add(part, v[k]);
        tau = (anchor_wave_sum(part) - 1.0) / (double)m;
        int gone = 0;
        for (int k = lane, i = 0; k < A; k += kWave, ++i)
            if ((act >> i & 1) && v[k] <= tau) {
                act &= ~(1u << i);
                ++gone;
            }
        gone = anchor_wave_count(gone);
        if (gone == 0 || gone >= m)
            break;
        m -= gone;
    }
    double part = 0.0;
    for (int k = lane, i = 0; k < A; k += kWave, ++i)
        if (act >> i & 1)
            part = anchor_add(part, v[k] - tau);
    tau = tau + (anchor_wave_sum(part) - 1.0) / (double)m;
    for (int k = lane, i = 0; k < A; k += kWave, ++i)
        v[k] = (act >> i & 1) ? fmax(v[k] - tau, 0.0) : 0.0;
}

// A wave per word w: min over the simplex of |W_w - x' W_S|^2 = x' G x - 2 h' x + |W_w|^2, h = row w
// of H, by projected gradient with Nesterov's momentum and the gradient restart ((y - x+) . (x+ - x) > 0
// resets it), step 1 / L, from x = 1 / A.  G x+ is formed once per iteration; G y follows from it
// and G x by the momentum's own combination.  The word stops when its Frank-Wolfe gap
// x . g - min_k g_k, g = 2 (G x - h), is at most tol |W_w|^2, or after max_iter iterations.
// Nothing here depends on another word or on the launch.  GLDS: G is copied to LDS first; the
// arithmetic is the same.  Grid ceil(V / 4); dynamic LDS (GLDS ? A x A : 0) + 4 x 7 x A doubles.
template <bool GLDS>
__global__ __launch_bounds__(kAnchorThreads) void anchor_solve_kernel(
    int V, int A, const double *__restrict__ H, const double *__restrict__ Gm, const double *__restrict__ Lp,
    const double *__restrict__ norm2, double tol, int max_iter, double *__restrict__ X, int32_t *__restrict__ iters,
    double *__restrict__ gaps)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double anchor_lds[];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const double *G = Gm;
    double *vec = anchor_lds;
    if (GLDS) {
        for (int i = tid; i < A * A; i += kAnchorThreads)
            anchor_lds[i] = Gm[i];
        __syncthreads();
        G = anchor_lds;
        vec = anchor_lds + (size_t)A * A;
    }
    const int w = blockIdx.x * kAnchorSolveWaves + wid;
    if (w >= V)
        return;                                             // (no barrier below)
    double *x = vec + (size_t)wid * kAnchorSolveVectors * A;
    double *y = x + A, *xn = y + A, *Gx = xn + A, *Gxn = Gx + A, *Gy = Gxn + A, *h = Gy + A;
    const double L = *Lp, inv_l = L > 0.0 ? 1.0 / L : 0.0;
    const double qq = norm2[w];
    const double x0 = 1.0 / (double)A;
    for (int k = lane; k < A; k += kWave) {
        x[k] = x0;
        y[k] = x0;
        h[k] = H[(size_t)w * A + k];
    }
    anchor_wave_sync();
    int it = 0;
    double gap = 0.0;
    if (qq > 0.0) {
        anchor_matvec(A, G, x, Gx, lane);
        for (int k = lane; k < A; k += kWave)
            Gy[k] = Gx[k];
        double t = 1.0;
        for (it = 1;; ++it) {                               // (uniform)
            for (int k = lane; k < A; k += kWave)
                xn[k] = y[k] - (2.0 * (Gy[k] - h[k])) * inv_l;
            anchor_project(A, xn, lane);
            anchor_wave_sync();
            anchor_matvec(A, G, xn, Gxn, lane);
            double dot = 0.0, mn = __builtin_huge_val(), turn = 0.0;
            for (int k = lane; k < A; k += kWave) {
                const double g = 2.0 * (Gxn[k] - h[k]);
                dot = anchor_add(dot, xn[k] * g);
                mn = fmin(mn, g);
                turn = anchor_add(turn, (y[k] - xn[k]) * (xn[k] - x[k]));
            }
            gap = anchor_wave_sum(dot) - anchor_wave_min(mn);
            turn = anchor_wave_sum(turn);
            const bool stop = gap <= tol * qq || it >= max_iter;
            double beta = 0.0;
            if (!(turn > 0.0)) {
                const double tn = 0.5 * (1.0 + sqrt(1.0 + 4.0 * t * t));
                beta = (t - 1.0) / tn;
                t = tn;
            } else {
                t = 1.0;
            }
            for (int k = lane; k < A; k += kWave) {
                const double xk = xn[k], gk = Gxn[k];
                y[k] = xk + beta * (xk - x[k]);
                Gy[k] = gk + beta * (gk - Gx[k]);
                x[k] = xk;
                Gx[k] = gk;
            }
            anchor_wave_sync();
            if (stop)
                break;
        }
    }
    for (int k = lane; k < A; k += kWave)
        X[(size_t)w * A + k] = x[k];
    if (lane == 0) {
        iters[w] = it;
        gaps[w] = qq > 0.0 ? gap / qq : 0.0;
    }
}

// pi[k] = sum_w X[w * A + k] p_w, p_w = r_w / total: the rounded products in the order of anchor_block_sum.
// Grid A.
__global__ __launch_bounds__(kAnchorThreads) void anchor_mass_kernel(int V, int A, const double *__restrict__ X,
                                                                     const double *__restrict__ r,
                                                                     const double *__restrict__ total,
                                                                     double *__restrict__ pi)
{
    __shared__ double red[kAnchorThreads];
    const int k = blockIdx.x, tid = threadIdx.x;
    const double tot = *total;
    double part = 0.0;
    for (int w = tid; w < V; w += kAnchorThreads)
        part = anchor_add(part, anchor_mul(X[(size_t)w * A + k], anchor_div(r[w], tot)));
    const double s = anchor_block_sum(part, red, tid);
    if (tid == 0)
        pi[k] = s;
}

// beta[w * A + k] = (X[w * A + k] p_w) / pi[k] (0 where pi[k] is not positive)
__global__ __launch_bounds__(kAnchorThreads) void anchor_beta_kernel(int V, int A, const double *__restrict__ X,
                                                                     const double *__restrict__ r,
                                                                     const double *__restrict__ total,
                                                                     const double *__restrict__ pi,
                                                                     double *__restrict__ beta)
{
    const size_t i = (size_t)blockIdx.x * kAnchorThreads + threadIdx.x;
    if (i >= (size_t)V * A)
        return;
    const int w = (int)(i / A), k = (int)(i % A);
    const double pk = pi[k];
    beta[i] = pk > 0.0 ? anchor_div(anchor_mul(X[i], anchor_div(r[w], *total)), pk) : 0.0;
}

}  // namespace trlda
