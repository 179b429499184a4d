// trlda_amd/csrc/topicdist_kernels.h -- distances between the topics of two models, a K x K2 matrix
// formed on the device (trlda_model_topic_distances).  No reference counterpart.
//
// Topics.  p_i = lambda_i / S_i, S_i = sum_v lambda_iv (E[beta_i], what top_words ranks by);
// q_j = mu_j / T_j from the second lambda, mu (K2 x V, the same V).  Both are K x V column-major: the
// K values of a word are contiguous.
//   hellinger       sqrt(max(0, 1 - sum_v sqrt(lambda_iv mu_jv) / (sqrt S_i sqrt T_j)))
//   cosine          max(0, 1 - sum_v lambda_iv mu_jv / (sqrt(sum lambda_i^2) sqrt(sum mu_j^2)))
//   kl              (sum_v lambda_iv log lambda_iv - sum_v lambda_iv log mu_jv) / S_i - log S_i + log T_j
//   jensen_shannon  H(m) - (H(p_i) / 2 + H(q_j) / 2),  H(m) = -sum_v m_v log m_v,  m = p_i / 2 + q_j / 2,
//                   H(p_i) = log S_i - sum_v lambda_iv log lambda_iv / S_i
// (kl and jensen_shannon are clamped into their ranges, [0, inf) and [0, ln 2]: the exact values lie
// there, so the clamp only ever removes rounding.)
//
// Order of additions.  Nothing here is atomic and nothing depends on the device or on launch order.
//   row statistics  blocks of kTopicDistStatWords words, the words of a block in ascending order,
//                   then the blocks in ascending order: a function of (K, V)
//   products        V is cut into chunks of `cw` words (topicdist_chunk_words: a function of K, K2, V);
//                   within a chunk every element is one chain of v_mfma_f64_16x16x4_f64 over ascending
//                   words, four at a time; the chunks' partial sums are added in ascending order
//   jensen_shannon  the same chunks, the words of a chunk in ascending order, one at a time
// An element (i, j) is formed from row i of lambda and row j of mu by operations that commute in the
// two (a b, a + b): with mu = lambda the symmetric measures come out bitwise symmetric.
#pragma once

#include "estep_kernels.h"

namespace trlda {

constexpr int kTopicDistThreads = 256;     // 4 waves
constexpr int kTopicDistMeasures = 4;      // 0: hellinger, 1: cosine, 2: kl, 3: jensen_shannon
constexpr int kTopicDistStatWords = 128;   // words per workgroup of the row statistics
constexpr int kTopicDistTile = 64;         // a workgroup's tile: 64 topics of lambda x 64 topics of mu
constexpr int kTopicDistStage = 32;        // words staged in LDS at a time
// LDS row (one word's 64 topics) stride in doubles: 16 mod 32.  Half a wave reads 2 words x 16 topics
// of an operand at once, (w + h) * 80 + t0 + m with h = 0, 1 and m = 0 .. 15: the 32 different 8-byte
// banks (80 mod 32 = 16)
constexpr int kTopicDistStride = kTopicDistTile + 16;
constexpr int kTopicDistTargetGroups = 1024;   // workgroups the chunking aims at
constexpr int kTopicDistMinChunk = 64;         // ... without cutting V finer than this

typedef double topicdist_f64x4 __attribute__((ext_vector_type(4)));

// Words per chunk of V: a multiple of the staging size, chosen so that tiles x chunks is about
// kTopicDistTargetGroups.  K = K2 = 500, V = 100 000: 64 tiles, 16 chunks of 6272 words, 32 MB of
// partial sums.  A function of (K, K2, V) alone.
inline int topicdist_chunk_words(int K, int K2, int V)
{
    const long long tiles = (long long)((K + kTopicDistTile - 1) / kTopicDistTile) *
                            ((K2 + kTopicDistTile - 1) / kTopicDistTile);
    long long chunks = kTopicDistTargetGroups / tiles;
    if (chunks < 1)
        chunks = 1;
    long long cw = (V + chunks - 1) / chunks;
    if (cw < kTopicDistMinChunk)
        cw = kTopicDistMinChunk;
    cw = (cw + kTopicDistStage - 1) / kTopicDistStage * kTopicDistStage;
    return (int)cw;
}

// part[(block * 3 + s) * K + k], s = 0: sum lambda, 1: sum lambda^2, 2: sum lambda log lambda over the
// block's words.  Thread t takes topics t, t + 256, ...: neighbouring threads read neighbouring values.
__global__ __launch_bounds__(kTopicDistThreads) void topicdist_stats_kernel(int K, int V,
                                                                            const double *__restrict__ lam,
                                                                            double *__restrict__ part)
{
#pragma clang fp contract(off)
    const int v0 = blockIdx.x * kTopicDistStatWords, v1 = min(V, v0 + kTopicDistStatWords);
    for (int k = threadIdx.x; k < K; k += kTopicDistThreads) {
        double s = 0.0, q = 0.0, l = 0.0;
        for (int v = v0; v < v1; ++v) {
            const double x = lam[k + (size_t)K * v];
            s += x;
            q += x * x;
            l += x * log(x);
        }
        double *o = part + (size_t)blockIdx.x * 3 * K + k;
        o[0] = s;
        o[K] = q;
        o[2 * (size_t)K] = l;
    }
}

// stats[s * K + k] = the blocks' partial sums added in ascending block order
__global__ __launch_bounds__(kTopicDistThreads) void topicdist_stats_sum_kernel(int K, int blocks,
                                                                                const double *__restrict__ part,
                                                                                double *__restrict__ stats)
{
    const int e = blockIdx.x * kTopicDistThreads + threadIdx.x;     // s * K + k
    if (e >= 3 * K)
        return;
    double a = 0.0;
    for (int b = 0; b < blocks; ++b)
        a += part[(size_t)b * 3 * K + e];
    stats[e] = a;
}

// what is staged of lambda (A) and of mu (B) for the product of measure M
template <int M>
__device__ __forceinline__ double topicdist_a(double x)
{
    return M == 0 ? sqrt(x) : x;
}
template <int M>
__device__ __forceinline__ double topicdist_b(double y)
{
    return M == 0 ? sqrt(y) : M == 1 ? y : log(y);
}

// Grid (tile of 64 topics of lambda, tile of 64 topics of mu, chunk of cw words), 4 waves; wave w owns
// the 32 x 32 block (w & 1, w >> 1) of the tile as 2 x 2 MFMA tiles.  Both operands are staged in LDS
// 32 words at a time, transformed while staged, as [word][topic]: a word's topics are contiguous in
// memory and in LDS, so the reads are coalesced and nothing is transposed.  Topics past K / K2 and
// words past the chunk's end are staged as exact zeros -- in both operands, so for kl the product of
// a pad is 0 * 0, never 0 * log -- and are neither read from memory nor written out.
//   first operand:  lane l holds B[topic l & 15][word kk + (l >> 4)] (mu), second: A likewise (lambda);
//   D: register r of lane l is (mu topic (l >> 4) + 4 r, lambda topic l & 15) -- 16 lanes write 16
//   neighbouring i.
// part[(chunk * K2 + j) * K + i].
template <int M>
__global__ __launch_bounds__(kTopicDistThreads) void topicdist_product_kernel(
    int K, int K2, int V, int cw, const double *__restrict__ lam, const double *__restrict__ mu,
    double *__restrict__ part)
{
    constexpr int S = kTopicDistStride, T = kTopicDistTile, W = kTopicDistStage;
    __shared__ __attribute__((aligned(16))) double a_lds[W * S], b_lds[W * S];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int m = lane & 15, kq = lane >> 4;
    const int wi = (wid & 1) * 32, wj = (wid >> 1) * 32;
    const int i0 = blockIdx.x * T, j0 = blockIdx.y * T;
    const int vbeg = blockIdx.z * cw, vend = min(V, vbeg + cw);     // (chunks * cw < V + cw: no overflow)
    const int st = tid & (T - 1), sw = tid / T;                     // staging: topic, first word
    const bool a_in = i0 + st < K, b_in = j0 + st < K2;
    const double *ap = lam + (a_in ? i0 + st : 0), *bp = mu + (b_in ? j0 + st : 0);

    topicdist_f64x4 acc[2][2];
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
            acc[ta][tb] = topicdist_f64x4{0.0, 0.0, 0.0, 0.0};

    for (int v0 = vbeg; v0 < vend; v0 += W) {
        __syncthreads();                                            // the previous words have been read
#pragma unroll
        for (int e = 0; e < W * T / kTopicDistThreads; ++e) {
            const int w = sw + e * (kTopicDistThreads / T), v = v0 + w;
            double x = 0.0, y = 0.0;
            if (v < vend) {
                if (a_in)
                    x = topicdist_a<M>(ap[(size_t)K * v]);
                if (b_in)
                    y = topicdist_b<M>(bp[(size_t)K2 * v]);
            }
            a_lds[w * S + st] = x;
            b_lds[w * S + st] = y;
        }
        __syncthreads();
        const int steps = (min(W, vend - v0) + 3) / 4;              // (the words past the end are zeros)
        for (int s = 0; s < steps; ++s) {
            const int row = (s * 4 + kq) * S;
            double a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = a_lds[row + wi + t * 16 + m];
                b[t] = b_lds[row + wj + t * 16 + m];
            }
#pragma unroll
            for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                for (int tb = 0; tb < 2; ++tb)
                    acc[ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(b[tb], a[ta], acc[ta][tb], 0, 0, 0);
        }
    }

    double *o = part + (size_t)blockIdx.z * K2 * K;
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + wi + ta * 16 + m, j = j0 + wj + tb * 16 + kq + 4 * r;
                if (i < K && j < K2)
                    o[(size_t)j * K + i] = acc[ta][tb][r];
            }
}

// Jensen-Shannon: the same grid and staging, the staged values being p_iv / 2 = (lambda_iv / S_i) / 2
// and q_jv / 2.  Thread t owns the 16 pairs (i0 + (t & 15) + 16 a, j0 + (t >> 4) + 16 b) and walks the
// staged words: m = p / 2 + q / 2, the sum of -m log m, one log per (i, j, v).  A pad gives m = 0 for the
// words past the end, which adds 0 (not 0 log 0); pads among the topics are not written out.
__global__ __launch_bounds__(kTopicDistThreads) void topicdist_js_kernel(
    int K, int K2, int V, int cw, const double *__restrict__ lam, const double *__restrict__ mu,
    const double *__restrict__ sa, const double *__restrict__ sb, double *__restrict__ part)
{
#pragma clang fp contract(off)
    constexpr int S = kTopicDistStride, T = kTopicDistTile, W = kTopicDistStage;
    __shared__ __attribute__((aligned(16))) double a_lds[W * S], b_lds[W * S];
    const int tid = threadIdx.x;
    const int ti = tid & 15, tj = tid >> 4;
    const int i0 = blockIdx.x * T, j0 = blockIdx.y * T;
    const int vbeg = blockIdx.z * cw, vend = min(V, vbeg + cw);
    const int st = tid & (T - 1), sw = tid / T;
    const bool a_in = i0 + st < K, b_in = j0 + st < K2;
    const double *ap = lam + (a_in ? i0 + st : 0), *bp = mu + (b_in ? j0 + st : 0);
    const double s_a = a_in ? sa[i0 + st] : 1.0, s_b = b_in ? sb[j0 + st] : 1.0;

    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            acc[a][b] = 0.0;

    for (int v0 = vbeg; v0 < vend; v0 += W) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < W * T / kTopicDistThreads; ++e) {
            const int w = sw + e * (kTopicDistThreads / T), v = v0 + w;
            double x = 0.0, y = 0.0;
            if (v < vend) {
                if (a_in)
                    x = 0.5 * (ap[(size_t)K * v] / s_a);
                if (b_in)
                    y = 0.5 * (bp[(size_t)K2 * v] / s_b);
            }
            a_lds[w * S + st] = x;
            b_lds[w * S + st] = y;
        }
        __syncthreads();
        const int words = min(W, vend - v0);
        for (int w = 0; w < words; ++w) {
            double p[4], q[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                p[t] = a_lds[w * S + ti + 16 * t];
                q[t] = b_lds[w * S + tj + 16 * t];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const double mv = p[a] + q[b];
                    const double term = mv * log(mv);
                    acc[a][b] -= mv > 0.0 ? term : 0.0;
                }
        }
    }

    double *o = part + (size_t)blockIdx.z * K2 * K;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + ti + 16 * a, j = j0 + tj + 16 * b;
            if (i < K && j < K2)
                o[(size_t)j * K + i] = acc[a][b];
        }
}

// One thread per element: the chunks' partial sums in ascending order, the measure's closing formula,
// the clamp, and with `self` (mu is lambda itself) an exact 0 on the diagonal.  sa / sb: the row
// statistics (3 x K, 3 x K2) of lambda and mu.  out[i + K j].
__global__ __launch_bounds__(kTopicDistThreads) void topicdist_finish_kernel(
    int K, int K2, int chunks, int measure, int self, const double *__restrict__ part,
    const double *__restrict__ sa, const double *__restrict__ sb, double *__restrict__ out)
{
#pragma clang fp contract(off)
    const size_t n = (size_t)K * K2, e = (size_t)blockIdx.x * kTopicDistThreads + threadIdx.x;
    if (e >= n)
        return;
    const int i = (int)(e % K), j = (int)(e / K);
    double a = 0.0;
    for (int c = 0; c < chunks; ++c)
        a += part[(size_t)c * n + e];
    const double S = sa[i], T = sb[j];
    double d;
    if (measure == 0) {
        // (the two roots apart: S T overflows where sqrt S sqrt T does not)
        d = sqrt(fmax(0.0, 1.0 - a / (sqrt(S) * sqrt(T))));
    } else if (measure == 1) {
        d = fmax(0.0, 1.0 - a / (sqrt(sa[K + i]) * sqrt(sb[K2 + j])));
    } else if (measure == 2) {
        d = fmax(0.0, (sa[2 * (size_t)K + i] - a) / S - log(S) + log(T));
    } else {
        const double hp = log(S) - sa[2 * (size_t)K + i] / S, hq = log(T) - sb[2 * (size_t)K2 + j] / T;
        d = fmin(0.69314718055994530942, fmax(0.0, a - (0.5 * hp + 0.5 * hq)));
    }
    out[e] = self && i == j ? 0.0 : d;
}

}  // namespace trlda
