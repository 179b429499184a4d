// trlda_amd/csrc/tsne_kernels.h -- a 2-D map of an indexed corpus: the k-nearest-neighbour graph of the
// index on itself, the perplexity calibration, the exact t-SNE gradient and its loop
// (trlda_docindex_nearest, trlda_docindex_affinities, trlda_docindex_tsne_*).  No
// reference counterpart.
//
// Neighbours.  docindex_query_kernel and docindex_merge_kernel rank top_n + 1 entries for blocks of the
// table's own rows; tsne_selfdrop_kernel copies a row's list without the entry whose id is the
// row's own (without the last entry where the own id is not among them: more than top_n exact
// duplicates of smaller id).  s is the staged tile product, so a list depends on the table alone.
//
// Calibration.  One wave per document; entry j of its k <= 99 neighbours lives in lane j mod 64.
//   D_j = fmax(1 - s_j, 0),  d_j = D_j - D_0 >= 0 (the list is sorted),  w_j = exp(-(beta d_j)),
//   S = sum w_j,  T = sum w_j d_j,  H(beta) = log S + (beta T) / S,  p_j = w_j / S.
// A lane adds its two entries, the 64 lane values go through wave_sum_dpp.  log k <= log perplexity:
// beta = 0, p = 1 / k.  m = #{d_j = 0} >= perplexity: beta = +inf, p = 1 / m on those m, 0 elsewhere.
// Otherwise hi = 1 / mean(d) is doubled while H(hi) > log perplexity (lo follows), then [lo, hi] is
// halved until hi - lo <= hi 2^-50 or 200 steps; beta = hi.
//
// Gradient.  q_ij = 1 / (1 + |y_i - y_j|^2) by IEEE division, nothing contracted.
//   repulsion   grid (row tile, column stripe); the stripe's y_j staged in LDS kTsneStage points at a
//               time; a thread owns row i and adds q^2 dx, q^2 dy and q over ascending j, j = i left
//               out; the three stripe partials go to part[c][stripe][row]
//   stripe      its width is tsne_stripe_width(N) = max(16, ceil(N / 64) rounded up to 16): at most 64
//               stripes, and N = 1000 already gives 63 stripes x 4 row tiles of 256 = 252 workgroups
//               for 256 CUs.  A function of N alone; the row tile (threads per workgroup) is a knob
//               that moves rows between workgroups and never changes a row's chain.
//   rowsum      row i adds its partials in ascending stripe
//   tree        one workgroup of 1024 threads per sum: thread t adds elements t, t + 1024, ... in that
//               order, wave_sum_dpp, then the 16 wave sums in ascending order.  Z, KL and the column
//               sums of Y all go through it: functions of the values and N alone.
//   attract     one wave per document: lane l takes entries l, l + 64, ... of the row in stored order,
//               adds P q dx, P q dy and P log((P Z)(1 + d^2)) (entries with P = 0 add no KL), then
//               wave_sum_dpp; grad = 4 (exaggeration A - R / Z)
// No atomics.  Every result is a function of (Y, P, N, exaggeration) alone.
#pragma once

#include <climits>

#include "docindex_kernels.h"

namespace trlda {

constexpr int kTsneThreads = 256;          // 4 waves: the wave-per-document kernels, the elementwise ones
constexpr int kTsneMaxNeighbors = 99;      // k = min(N - 1, floor(3 perplexity)), perplexity <= 33
constexpr int kTsneMaxStripes = 64;
constexpr int kTsneStage = 1024;           // points of a stripe in LDS at a time: 16 KB
constexpr int kTsneDefaultTile = 256;      // rows (threads) per workgroup of the repulsion
constexpr int kTsneMaxTile = 1024;
constexpr int kTsneTreeThreads = 1024;

// Columns per stripe of the repulsion: a function of N alone (see the header comment)
inline long long tsne_stripe_width(long long N)
{
    long long w = (N + kTsneMaxStripes - 1) / kTsneMaxStripes;
    w = (w + 15) / 16 * 16;
    return w < 16 ? 16 : w;
}

// in: B lists of top_n + 1 (id, s) of the rows first .. first + B - 1; out: rows first .. of an
// (N x top_n) table.  One thread per row.
__global__ __launch_bounds__(kTsneThreads) void tsne_selfdrop_kernel(
    int B, int top_n, long long first, const long long *__restrict__ in_i, const double *__restrict__ in_s,
    long long *__restrict__ out_i, double *__restrict__ out_s)
{
    const long long q = (long long)blockIdx.x * kTsneThreads + threadIdx.x;
    if (q >= B)
        return;
    const long long own = first + q;
    const long long *ii = in_i + (size_t)q * (top_n + 1);
    const double *is = in_s + (size_t)q * (top_n + 1);
    long long *oi = out_i + (size_t)own * top_n;
    double *os = out_s + (size_t)own * top_n;
    int pos = top_n;                                 // (not found: the last entry goes)
    for (int e = 0; e <= top_n; ++e)
        if (ii[e] == own) {
            pos = e;
            break;
        }
    for (int j = 0; j < top_n; ++j) {
        const int e = j < pos ? j : j + 1;
        oi[j] = ii[e];
        os[j] = is[e];
    }
}

// H(beta) of the header comment for the wave's row; S comes back too
__device__ __forceinline__ double tsne_entropy(double beta, const double (&d)[2], const bool (&in)[2], double &S)
{
#pragma clang fp contract(off)
    const double w0 = in[0] ? exp(-(beta * d[0])) : 0.0;
    const double w1 = in[1] ? exp(-(beta * d[1])) : 0.0;
    S = wave_sum_dpp(w0 + w1);
    const double T = wave_sum_dpp(w0 * d[0] + w1 * d[1]);
    return log(S) + (beta * T) / S;
}

// sim: N x k similarities, each row sorted descending.  p: N x k, beta: N.  One wave per document.
__global__ __launch_bounds__(kTsneThreads) void tsne_calibrate_kernel(long long N, int k, double perplexity,
                                                                      const double *__restrict__ sim,
                                                                      double *__restrict__ p,
                                                                      double *__restrict__ beta_out)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const long long doc = (long long)blockIdx.x * (kTsneThreads / kWave) + wid;
    if (doc >= N)                                    // (the whole wave)
        return;
    const double *s = sim + (size_t)doc * k;
    double *pr = p + (size_t)doc * k;
    const double D0 = fmax(1.0 - s[0], 0.0);
    double d[2];
    bool in[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int j = lane + r * kWave;
        in[r] = j < k;
        d[r] = in[r] ? fmax(1.0 - s[j], 0.0) - D0 : 0.0;
    }
    const double target = log(perplexity);
    double beta, w[2];
    if (log((double)k) <= target) {
        beta = 0.0;
        w[0] = w[1] = 1.0 / (double)k;
    } else {
        const int m = __popcll(__ballot(in[0] && d[0] == 0.0)) + __popcll(__ballot(in[1] && d[1] == 0.0));
        if ((double)m >= perplexity) {
            beta = __builtin_huge_val();
            w[0] = d[0] == 0.0 ? 1.0 / (double)m : 0.0;
            w[1] = d[1] == 0.0 ? 1.0 / (double)m : 0.0;
        } else {
            // (m < k here, so the mean is positive)
            const double mean = wave_sum_dpp(d[0] + d[1]) / (double)k;
            double S, lo = 0.0, hi = 1.0 / mean;
            for (int it = 0; it < 1100 && hi < 1e300 && tsne_entropy(hi, d, in, S) > target; ++it) {
                lo = hi;
                hi = hi * 2.0;
            }
            for (int it = 0; it < 200 && hi - lo > hi * 0x1p-50; ++it) {
                const double mid = 0.5 * (lo + hi);
                if (tsne_entropy(mid, d, in, S) > target)
                    lo = mid;
                else
                    hi = mid;
            }
            beta = hi;
            (void)tsne_entropy(beta, d, in, S);
            w[0] = exp(-(beta * d[0])) / S;
            w[1] = exp(-(beta * d[1])) / S;
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
        if (in[r])
            pr[lane + r * kWave] = w[r];
    if (lane == 0)
        beta_out[doc] = beta;
}

// Grid (row tile of blockDim.x rows, stripe of W columns).  part: 3 x stripes x N (R_x, R_y, Z).
__global__ __launch_bounds__(kTsneMaxTile) void tsne_repulsion_kernel(long long N, long long W,
                                                                      const double *__restrict__ Y,
                                                                      double *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double ys[2 * kTsneStage];
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long j0 = (long long)blockIdx.y * W, j1 = min(N, j0 + W);
    const bool live = i < N;
    const double xi = live ? Y[2 * i] : 0.0, yi = live ? Y[2 * i + 1] : 0.0;
    double rx = 0.0, ry = 0.0, z = 0.0;
    for (long long c0 = j0; c0 < j1; c0 += kTsneStage) {
        const int cn = (int)min((long long)kTsneStage, j1 - c0);
        __syncthreads();                             // the previous points have been read
        for (int t = threadIdx.x; t < 2 * cn; t += blockDim.x)
            ys[t] = Y[2 * c0 + t];
        __syncthreads();
        if (live) {
            const long long self = i - c0;           // (outside [0, cn): no column of this pass is row i)
            for (int jj = 0; jj < cn; ++jj) {
                const double dx = xi - ys[2 * jj], dy = yi - ys[2 * jj + 1];
                const double q = 1.0 / (1.0 + (dx * dx + dy * dy));
                if (jj != self) {
                    const double q2 = q * q;
                    rx = rx + q2 * dx;
                    ry = ry + q2 * dy;
                    z = z + q;
                }
            }
        }
    }
    if (live) {
        const size_t S = gridDim.y, s = blockIdx.y;
        part[(0 * S + s) * (size_t)N + i] = rx;
        part[(1 * S + s) * (size_t)N + i] = ry;
        part[(2 * S + s) * (size_t)N + i] = z;
    }
}

// R (3 x N): row i's stripe partials in ascending stripe
__global__ __launch_bounds__(kTsneThreads) void tsne_rowsum_kernel(long long N, int stripes,
                                                                   const double *__restrict__ part,
                                                                   double *__restrict__ R)
{
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * kTsneThreads + threadIdx.x;
    if (i >= N)
        return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double a = 0.0;
        for (int s = 0; s < stripes; ++s)
            a = a + part[((size_t)c * stripes + s) * (size_t)N + i];
        R[(size_t)c * N + i] = a;
    }
}

struct tsne_tree_job {
    const double *in;                                // element e at in[e * stride]
    long long stride;
    double *out;
};

// Workgroup b adds the n elements of job b in the fixed tree of the header comment.  Up to 3 jobs.
__global__ __launch_bounds__(kTsneTreeThreads) void tsne_tree_kernel(long long n, tsne_tree_job j0, tsne_tree_job j1,
                                                                     tsne_tree_job j2)
{
#pragma clang fp contract(off)
    __shared__ double ws[kTsneTreeThreads / kWave];
    const tsne_tree_job job = blockIdx.x == 0 ? j0 : (blockIdx.x == 1 ? j1 : j2);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    double a = 0.0;
    for (long long e = tid; e < n; e += kTsneTreeThreads)
        a = a + job.in[e * job.stride];
    a = wave_sum_dpp(a);
    if (lane == 0)
        ws[wid] = a;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < kTsneTreeThreads / kWave; ++w)
            t = t + ws[w];
        *job.out = t;
    }
}

// One wave per document.  P: the CSR (indptr N + 1, ids, val); R: 3 x N; Z: one double on the device.
__global__ __launch_bounds__(kTsneThreads) void tsne_attract_kernel(
    long long N, const long long *__restrict__ indptr, const long long *__restrict__ ids,
    const double *__restrict__ P, const double *__restrict__ Y, const double *__restrict__ R,
    const double *__restrict__ Zp, double exaggeration, double *__restrict__ grad, double *__restrict__ klrow)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const long long doc = (long long)blockIdx.x * (kTsneThreads / kWave) + wid;
    if (doc >= N)                                    // (the whole wave)
        return;
    const double Z = *Zp, xi = Y[2 * doc], yi = Y[2 * doc + 1];
    double ax = 0.0, ay = 0.0, kl = 0.0;
    const long long e1 = indptr[doc + 1];
    for (long long e = indptr[doc] + lane; e < e1; e += kWave) {
        const long long j = ids[e];
        const double pij = P[e];
        const double dx = xi - Y[2 * j], dy = yi - Y[2 * j + 1];
        const double one = 1.0 + (dx * dx + dy * dy);
        const double pq = pij * (1.0 / one);
        ax = ax + pq * dx;
        ay = ay + pq * dy;
        if (pij > 0.0)
            kl = kl + pij * log((pij * Z) * one);
    }
    ax = wave_sum_dpp(ax);
    ay = wave_sum_dpp(ay);
    kl = wave_sum_dpp(kl);
    if (lane == 0) {
        grad[2 * doc] = 4.0 * (exaggeration * ax - R[doc] / Z);
        grad[2 * doc + 1] = 4.0 * (exaggeration * ay - R[(size_t)N + doc] / Z);
        klrow[doc] = kl;
    }
}

// The update of one iteration, elementwise over the n = 2 N components
__global__ __launch_bounds__(kTsneThreads) void tsne_update_kernel(long long n, double momentum, double lr,
                                                                   const double *__restrict__ grad,
                                                                   double *__restrict__ vel, double *__restrict__ gain,
                                                                   double *__restrict__ Y)
{
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * kTsneThreads + threadIdx.x;
    if (t >= n)
        return;
    const double g = grad[t];
    double v = vel[t], gn = gain[t];
    const bool same = (g > 0.0) == (v > 0.0);
    gn = same ? gn * 0.8 : gn + 0.2;
    gn = fmax(gn, 0.01);
    v = momentum * v - (lr * gn) * g;
    gain[t] = gn;
    vel[t] = v;
    Y[t] = Y[t] + v;
}

// Y[i][c] -= sums[c] / N
__global__ __launch_bounds__(kTsneThreads) void tsne_centre_kernel(long long n, double N,
                                                                   const double *__restrict__ sums,
                                                                   double *__restrict__ Y)
{
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * kTsneThreads + threadIdx.x;
    if (t >= n)
        return;
    Y[t] = Y[t] - sums[t & 1] / N;
}

// Y[d][c] = sum_k (theta^_dk - mean_k) axes[c K + k], theta^ recovered as in topicdocs_kernels.h (the
// cosine rows' sum in the order of topicdocs_scale_kernel).  Lane l adds k = l, l + 64, ... in that
// order, then wave_sum_dpp.  One wave per document.
__global__ __launch_bounds__(kTsneThreads) void tsne_project_kernel(int K, int Kp, long long N, int measure,
                                                                    const double *__restrict__ table,
                                                                    const double *__restrict__ mean,
                                                                    const double *__restrict__ axes,
                                                                    double *__restrict__ Y)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const long long doc = (long long)blockIdx.x * (kTsneThreads / kWave) + wid;
    if (doc >= N)                                    // (the whole wave)
        return;
    const double *r = table + (size_t)doc * Kp;
    double scale = 1.0;
    if (measure != 0) {
        double a = 0.0;
        for (int k = lane; k < K; k += kWave)
            a += r[k];
        scale = wave_sum_dpp(a);
    }
    double a0 = 0.0, a1 = 0.0;
    for (int k = lane; k < K; k += kWave) {
        const double c = (measure == 0 ? r[k] * r[k] : r[k] / scale) - mean[k];
        a0 = a0 + c * axes[k];
        a1 = a1 + c * axes[K + k];
    }
    a0 = wave_sum_dpp(a0);
    a1 = wave_sum_dpp(a1);
    if (lane == 0) {
        Y[2 * doc] = a0;
        Y[2 * doc + 1] = a1;
    }
}

}  // namespace trlda
