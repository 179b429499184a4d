// trlda_amd/csrc/classify_kernels.h -- indexed documents classified from their topic proportions:
// multinomial logistic regression of a label on theta^ (trlda_docindex_classify_eval,
// trlda_docindex_classify_predict; Blei, Ng & Jordan 2003, section 7.2).  No reference
// counterpart.
//
// theta^ is topicdocs_theta of the stored row (topicdocs_kernels.h), with topicdocs_scale_kernel's row
// sums for a cosine index.  Nothing here is atomic, nothing depends on launch order, every chain starts
// from +0 and every + - x / is one rounded fp64 operation (fp contract off).
//
// Forward.  z_dc = sum_k theta^_dk W_ck is the staged tile product of tile_product.h with SW = 1: X the
// 64 theta^ rows of the workgroup's block (topicdocs_theta is applied while the row is staged), Y the
// coefficient rows (C rows of Kp doubles, the tail zero), 64 classes at a time: one chain of Kp / 4
// MFMAs from +0 per (document, class), a function of the stored row, the coefficient row and K alone.
// The block's logits lie in LDS as [document][class].  Per document, the classes in ascending order:
//   m = max_c z_c          (the first class that attains it is the label)
//   e_c = exp(z_c - m)     one subtraction, the fp64 exp
//   S = ((0.0 + e_0) + e_1) + ... + e_{C-1}
//   l = (log(S) + m) - z_y
//   p_c = e_c / S          IEEE division
//   r_c = w (p_c - [c = y])    one subtraction, then one multiply (none without weights)
// Thread t looks after document t & 63 and the classes c = t >> 6 (mod 4) of it; S is added by each of
// the document's four threads over all classes in the same ascending order, so the four hold the same
// bits and how the classes are shared does not show.  A document left out (label -1) or past the end
// writes a row of exact zeros and adds an exact +0 to the loss.  The block's 64 terms w_d l_d are added
// one after the other from 0.0 in ascending document order; classify_loss_finish_kernel adds the blocks
// in ascending order.
//
// Gradient.  R^T Theta^ of the rows r (N x Cp, Cp = ceil(C / 4) * 4, the tail zero) is the cross product
// of effects_products_kernel with Z = R on the device and no weights: its cross items alone, chunks of
// classify_chunk_rows(C, K, N) rows, the chunks' partial sums added in ascending order.  R is kept for a
// slab of whole chunks at a time; the partial sums lie outside the slab and are finished once, so
// neither sum depends on the slab.
#pragma once

#include "effects_kernels.h"

#define TRLDA_CLASSIFY_MAX_CLASSES 128

namespace trlda {

constexpr int kClassifyThreads = 256;      // 4 waves
constexpr int kClassifyBlockDocs = 64;     // documents per workgroup, and per partial sum of the loss
constexpr int kClassifyMaxClasses = TRLDA_CLASSIFY_MAX_CLASSES;
constexpr size_t kClassifySlabBytes = (size_t)256 << 20;   // scratch of R per slab: a chosen number

// LDS row stride of the logits in doubles: odd, so the 64 lanes that each read one class of 64
// documents fall into different banks
constexpr int classify_logit_stride(int C) { return C | 1; }

// LDS of classify_forward_kernel: the two staged operands, the logits, the 64 terms of the loss
constexpr size_t classify_forward_lds(int C)
{
    return tile_operands_lds(kClassifyBlockDocs) +
           (size_t)kClassifyBlockDocs * (classify_logit_stride(C) + 1) * sizeof(double);
}
static_assert(classify_forward_lds(kClassifyMaxClasses) <= (size_t)160 << 10,
              "64 x 129 logits beside the 128 x 34 operands within the 160 KiB of a CU");

// Rows per chunk of the gradient: as effects_chunk_rows, over the cross items alone, and a multiple
// of the forward block so that a slab of whole chunks is a slab of whole blocks.  A function of
// (C, K, N) alone.  C = 20, K = 100, N = 1 000 000: 2 items, 512 chunks of 1984 rows, 8 MB of partial
// sums.
inline long long classify_chunk_rows(int C, int K, long long N)
{
    long long chunks = kEffectsTargetGroups / ((long long)effects_tiles(C) * effects_tiles(K));
    if (chunks < 1)
        chunks = 1;
    long long cr = (N + chunks - 1) / chunks;
    if (cr < kEffectsMinChunk)
        cr = kEffectsMinChunk;
    return (cr + kClassifyBlockDocs - 1) / kClassifyBlockDocs * kClassifyBlockDocs;
}

// Rows of R per slab: whole chunks, at least one; `rows` > 0 is the A/B switch, else what
// kClassifySlabBytes holds
inline long long classify_slab_rows(long long rows, long long cr, int Cp)
{
    if (rows <= 0)
        rows = (long long)(kClassifySlabBytes / ((size_t)Cp * sizeof(double)));
    return rows / cr > 0 ? rows / cr * cr : cr;
}

// Grid (block of 64 of the launch's rows, from row0 on), 4 waves.  Row q < n of the launch is row
// ids[q] of the table (q itself without ids); rows past n are read as row n - 1 and kept out.
// FIT: r into R[(q - row0) * Cp + c] (the slab starts at row0) and the block's loss into
// part_loss[q / 64]; labels and w (or NULL) are indexed by q.  Otherwise: label_out[q] and, unless NULL,
// proba_out[q * C + c].
// D of the product: register r of acc[0][j] in lane l is z(document w * 16 + (l >> 4) + 4 r of the
// block, class 16 j + (l & 15) of the group).
template <bool FIT>
__global__ __launch_bounds__(kClassifyThreads) void classify_forward_kernel(
    int C, int Cp, int Kp, long long n, long long row0, int measure, const double *__restrict__ table,
    const double *__restrict__ scale, const long long *__restrict__ ids, const double *__restrict__ coef,
    const int *__restrict__ labels, const double *__restrict__ w, double *__restrict__ R,
    double *__restrict__ part_loss, int *__restrict__ label_out, double *__restrict__ proba_out)
{
#pragma clang fp contract(off)
    constexpr int B = kClassifyBlockDocs, S = kDocIndexStride, C2 = kDocIndexChunk / 2;
    extern __shared__ __attribute__((aligned(16))) double classify_lds[];
    __shared__ long long row_of[B];
    const int ZS = classify_logit_stride(C);
    double *x_lds = classify_lds;                           // B x S
    double *y_lds = x_lds + B * S;                          // 64 x S
    double *z_lds = y_lds + 64 * S;                         // B x ZS: z, then e, then r or p
    double *t_lds = z_lds + B * ZS;                         // B
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int m = lane & 15, kq = lane >> 4;
    const long long q0 = row0 + (long long)blockIdx.x * B;

    if (tid < B) {
        const long long q = min(q0 + tid, n - 1);
        row_of[tid] = ids ? ids[q] : q;
    }
    __syncthreads();

    for (int g0 = 0; g0 < C; g0 += 64) {
        docindex_f64x4 acc[1][4] = {};
        for (int k0 = 0; k0 < Kp; k0 += kDocIndexChunk) {
            const int cl = min(kDocIndexChunk, Kp - k0);    // a multiple of 4
            __syncthreads();                                // the previous chunk has been read
            for (int i = tid; i < B * C2; i += kClassifyThreads) {
                const int row = i / C2, c = (i % C2) * 2;
                if (c < cl) {
                    const long long d = row_of[row];
                    const double2 x = *reinterpret_cast<const double2 *>(table + (size_t)d * Kp + k0 + c);
                    double2 y;
                    y.x = topicdocs_theta(x.x, measure, scale, d);
                    y.y = topicdocs_theta(x.y, measure, scale, d);
                    *reinterpret_cast<double2 *>(x_lds + row * S + c) = y;
                }
            }
            tile_stage<64, kClassifyThreads>(y_lds, coef, Kp, k0, cl, tid,
                                             [&](int row) { return min(g0 + row, C - 1); });
            __syncthreads();
            for (int kk = 0; kk < cl; kk += 4)
                tile_step<1>(acc, x_lds, y_lds, kk, wid, m, kq);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int dl = wid * 16 + kq + 4 * r, c = g0 + j * 16 + m;
                if (c < C)
                    z_lds[dl * ZS + c] = acc[0][j][r];
            }
    }
    __syncthreads();                                        // the logits are complete

    // from here on thread t looks after document dl and the classes c = part (mod 4) of it
    const int dl = tid & (B - 1), part = tid / B;
    const long long q = q0 + dl;
    double *zr = z_lds + dl * ZS;
    int y = -1;
    if (FIT && q < n)
        y = labels[q];
    const bool live = FIT ? y >= 0 : q < n;
    double mx = zr[0], zy = 0.0;
    int arg = 0;
    for (int c = 1; c < C; ++c) {
        const double v = zr[c];
        if (v > mx) {                                       // (strict: equal logits keep the smaller class)
            mx = v;
            arg = c;
        }
    }
    if (FIT && live)
        zy = zr[y];
    __syncthreads();                                        // every z has been read
    for (int c = part; c < C; c += 4)
        zr[c] = exp(zr[c] - mx);
    __syncthreads();
    double sum = 0.0;
    for (int c = 0; c < C; ++c)
        sum += zr[c];
    if (FIT && part == 0) {
        double term = 0.0;
        if (live) {
            term = (log(sum) + mx) - zy;
            if (w)
                term = w[q] * term;
        }
        t_lds[dl] = term;
    }
    __syncthreads();                                        // every e has been read
    if (FIT) {
        const double wd = live && w ? w[q] : 1.0;
        for (int c = part; c < Cp; c += 4) {
            double r = 0.0;
            if (live && c < C) {
                r = zr[c] / sum - (c == y ? 1.0 : 0.0);
                if (w)
                    r = wd * r;
            }
            if (c < ZS)                                     // (Cp <= ZS unless C = Cp: then c < C holds)
                zr[c] = r;
        }
    } else {
        for (int c = part; c < C; c += 4)
            zr[c] = zr[c] / sum;
        if (part == 0 && live)
            label_out[q] = arg;
    }
    __syncthreads();
    const int rows = (int)min((long long)B, n - q0);        // (> 0: the grid covers rows below n only)
    if (FIT) {
        // the block's rows of R are one contiguous run of rows x Cp doubles; the tail beyond the
        // logits' stride is zero by construction
        double *o = R + (size_t)(q0 - row0) * Cp;
        for (int i = tid; i < rows * Cp; i += kClassifyThreads) {
            const int r = i / Cp, c = i % Cp;
            o[i] = c < ZS ? z_lds[r * ZS + c] : 0.0;
        }
        if (tid == 0) {
            double a = 0.0;
            for (int r = 0; r < B; ++r)
                a += t_lds[r];
            part_loss[q0 / B] = a;
        }
    } else if (proba_out) {
        double *o = proba_out + (size_t)q0 * C;
        for (int i = tid; i < rows * C; i += kClassifyThreads)
            o[i] = z_lds[(i / C) * ZS + i % C];
    }
}

// loss[0] = the blocks' partial sums added in ascending block order from 0.0.  One workgroup: thread 0
// adds, one term after the other, out of LDS; all threads fetch the next 256 terms meanwhile (one
// thread reading global memory term by term took 1.1 ms for the 15 625 blocks of N = 10^6).
__global__ __launch_bounds__(kClassifyThreads) void classify_loss_finish_kernel(long long blocks,
                                                                                const double *__restrict__ part,
                                                                                double *__restrict__ loss)
{
#pragma clang fp contract(off)
    constexpr int T = kClassifyThreads;
    __shared__ double tile[2][T];
    const int tid = threadIdx.x;
    if (tid < blocks)
        tile[0][tid] = part[tid];
    __syncthreads();
    double a = 0.0;
    int cur = 0;
    for (long long b0 = 0; b0 < blocks; b0 += T) {
        if (b0 + T + tid < blocks)
            tile[cur ^ 1][tid] = part[b0 + T + tid];
        if (tid == 0) {
            const int n = (int)min((long long)T, blocks - b0);
            for (int i = 0; i < n; ++i)
                a += tile[cur][i];
        }
        __syncthreads();
        cur ^= 1;
    }
    if (tid == 0)
        loss[0] = a;
}

}  // namespace trlda
