// dirichlet_kernels.h -- HIP kernels for gfx950 (MI355X) implementing sampleDirichlet (reference
// src/utils.cpp:251-266): an m x n array, F-order (column j contiguous), each column one draw from
// Dirichlet(alpha 1_m) -- m Gamma(alpha) draws divided by their sum.  Host side: trlda_hip.hip,
// dirichlet_device.
//
// Entry (i, j) is the log of a Gamma(alpha) draw, philox.h's recipe with purposes 16 / 17 / 18
// (normal / accept / boost) and counter (row i, column j, attempt).  A column is normalised in log
// space: mx = the column's max, W_i = exp(lg_i - mx), out_i = W_i / S, S the sum of the W below.
// W_max = 1, so S >= 1 for any alpha > 0: a tiny alpha never gives 0 / 0.  The order of the
// additions is a function of m only -- never of n, the grid or the device -- so under one key
// column j is the same bits whatever n is.
//
// m <= kDirichletWaveRows: one wave per column (dirichlet_wave_kernel), kSampleWaves columns per
// workgroup.  KPL = ceil(m / 64); lane l holds rows q * 64 + l,
// q < KPL (rows >= m absent: nothing is added for them).  Like sample_theta_kernel, the wave keeps
// the column in place: lg, then W, then W / S (a lane only reads back what it wrote).
//   s_l = ((0 + W_l) + W_{64+l}) + W_{128+l}) + ...       (the lane's rows in order of q)
//   S   = the butterfly of the 64 s_l: t_l = s_l, then for h = 32, 16, .., 1: t_l = t_l + t_{l+h}
//         (l < h; each lane adds its partner's value, so every lane holds the same bits), S = t_0
//
// m > kDirichletWaveRows: a column is cut into chunks of kSampleChunk = 4096 rows, a workgroup
// (4 waves) per (column, chunk), b = j * nchunk + c; thread t holds
// rows c * 4096 + q * 256 + t, q < 16.  (A launch covers whole columns j0 .. : grids stay below 2^32
// work-items.)
//   1. dirichlet_chunk_draw_kernel   lg into the column, the chunk's max into part[b]
//   2. dirichlet_reduce_kernel       per column the max over its chunks
//   3. dirichlet_chunk_exp_kernel    W in place and the chunk's sum into part[b]:
//        s_t = (0 + W_{q=0}) + W_{q=1} + ... (in order of q), a wave's 64 by the butterfly above,
//        the chunk ((0 + wave 0) + wave 1) + wave 2) + wave 3
//   4. dirichlet_reduce_kernel       per column S = ((0 + chunk 0) + chunk 1) + ...
//   5. dirichlet_chunk_scale_kernel  W / S
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.h"
#include "sample_kernels.h"           // kSampleThreads, kSampleChunk, sample_wave_max

namespace trlda {

enum : uint32_t {
    kDirichletNormal = 16,
    kDirichletAccept = 17,
    kDirichletBoost = 18,
};

constexpr int kDirichletWaveRows = 1024;
constexpr int kDirichletChunkPerThread = kSampleChunk / kSampleThreads;

// a uniform value moved into a vector register: the key schedule and counter words of the draws
// below then live in VGPRs, and the uniform ones no longer outgrow the scalar register file (left
// to itself the compiler spills SGPRs in both draw kernels)
__device__ __forceinline__ uint32_t dirichlet_vgpr(uint32_t x)
{
    uint32_t v;
    asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
    return v;
}

__device__ __forceinline__ double dirichlet_log_gamma(double alpha, int64_t i, int64_t j, uint32_t key0,
                                                      uint32_t key1)
{
    double lg;
    [[clang::always_inline]] lg = philox_log_gamma(alpha, (uint32_t)i, (uint32_t)j, kDirichletNormal,
                                                   kDirichletAccept, kDirichletBoost, key0, key1);
    return lg;
}

// the butterfly sum of the header: the same bits in every lane
__device__ __forceinline__ double dirichlet_wave_sum(double v)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int h = 32; h > 0; h >>= 1)
        v = v + __shfl_xor(v, h, kWave);
    return v;
}

// m <= kDirichletWaveRows: one wave per column
__global__ __launch_bounds__(kSampleThreads) void dirichlet_wave_kernel(int m, int64_t j0, int64_t n, int kpl,
                                                                       double alpha,
                                                                       uint32_t key0, uint32_t key1,
                                                                       double *__restrict__ out,
                                                                       double *__restrict__ sums)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    key0 = dirichlet_vgpr(key0);
    key1 = dirichlet_vgpr(key1);
    const int64_t j = j0 + (int64_t)blockIdx.x * kSampleWaves + threadIdx.x / kWave;
    if (j < n) {
        double *col = out + j * m;
        double mx = -INFINITY;
        for (int q = 0; q < kpl; ++q) {
            const int i = q * kWave + lane;
            if (i < m) {
                const double lg = dirichlet_log_gamma(alpha, i, j, key0, key1);
                col[i] = lg;
                mx = fmax(mx, lg);
            }
        }
        mx = sample_wave_max(mx);
        double s = 0.0;
        for (int q = 0; q < kpl; ++q) {
            const int i = q * kWave + lane;
            if (i < m) {
                const double W = exp(col[i] - mx);
                col[i] = W;
                s = s + W;
            }
        }
        const double S = dirichlet_wave_sum(s);
        if (sums) {                        // (test hook: W and S, not W / S)
            if (lane == 0)
                sums[j] = S;
            return;
        }
        for (int q = 0; q < kpl; ++q) {
            const int i = q * kWave + lane;
            if (i < m)
                col[i] = col[i] / S;
        }
    }
}

// 1. lg into the column; the chunk's max into part[b]
__global__ __launch_bounds__(kSampleThreads) void dirichlet_chunk_draw_kernel(int m, int64_t j0, int nchunk,
                                                                             double alpha, uint32_t key0,
                                                                             uint32_t key1,
                                                                             double *__restrict__ out,
                                                                             double *__restrict__ part)
{
    __shared__ double red[kSampleWaves];
    key0 = dirichlet_vgpr(key0);
    key1 = dirichlet_vgpr(key1);
    const unsigned jr = blockIdx.x / (unsigned)nchunk;
    const int c = (int)(blockIdx.x - jr * (unsigned)nchunk);
    const int64_t j = j0 + jr;
    const int64_t b = j * nchunk + c;
    double *col = out + j * m;
    const uint32_t jv = dirichlet_vgpr((uint32_t)j);
    double mx = -INFINITY;
#pragma unroll 1
    for (int q = 0; q < kDirichletChunkPerThread; ++q) {
        const int64_t i = (int64_t)c * kSampleChunk + q * kSampleThreads + (int)threadIdx.x;
        if (i < m) {
            const double lg = dirichlet_log_gamma(alpha, i, jv, key0, key1);
            col[i] = lg;
            mx = fmax(mx, lg);
        }
    }
    mx = sample_wave_max(mx);
    if ((threadIdx.x & (kWave - 1)) == 0)
        red[threadIdx.x / kWave] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = red[0];
        for (int k = 1; k < kSampleWaves; ++k)
            v = fmax(v, red[k]);
        part[b] = v;
    }
}

// 2. / 4. one thread per column over its nchunk entries of part, in chunk order: the max (SUM = false)
// or the sum from 0 (SUM = true)
template <bool SUM>
__global__ __launch_bounds__(kSampleThreads) void dirichlet_reduce_kernel(int64_t n, int nchunk,
                                                                         const double *__restrict__ part,
                                                                         double *__restrict__ col_out)
{
#pragma clang fp contract(off)
    const int64_t stride = (int64_t)gridDim.x * kSampleThreads;
    for (int64_t j = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x; j < n; j += stride) {
        const double *p = part + j * nchunk;
        double v = SUM ? 0.0 : -INFINITY;
        for (int c = 0; c < nchunk; ++c)
            v = SUM ? v + p[c] : fmax(v, p[c]);
        col_out[j] = v;
    }
}

// 3. W = exp(lg - mx) in place; the chunk's sum (header) into part[b]
__global__ __launch_bounds__(kSampleThreads) void dirichlet_chunk_exp_kernel(int m, int64_t j0, int nchunk,
                                                                            const double *__restrict__ colmax,
                                                                            double *__restrict__ out,
                                                                            double *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double red[kSampleWaves];
    const unsigned jr = blockIdx.x / (unsigned)nchunk;
    const int c = (int)(blockIdx.x - jr * (unsigned)nchunk);
    const int64_t j = j0 + jr;
    const int64_t b = j * nchunk + c;
    double *col = out + j * m;
    const double mx = colmax[j];
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < kDirichletChunkPerThread; ++q) {
        const int64_t i = (int64_t)c * kSampleChunk + q * kSampleThreads + (int)threadIdx.x;
        if (i < m) {
            const double W = exp(col[i] - mx);
            col[i] = W;
            s = s + W;
        }
    }
    const double wave_total = dirichlet_wave_sum(s);
    if ((threadIdx.x & (kWave - 1)) == 0)
        red[threadIdx.x / kWave] = wave_total;
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = 0.0;
        for (int k = 0; k < kSampleWaves; ++k)
            v = v + red[k];
        part[b] = v;
    }
}

// 5. W / S
__global__ __launch_bounds__(kSampleThreads) void dirichlet_chunk_scale_kernel(int m, int64_t j0, int nchunk,
                                                                              const double *__restrict__ colsum,
                                                                              double *__restrict__ out)
{
    const unsigned jr = blockIdx.x / (unsigned)nchunk;
    const int c = (int)(blockIdx.x - jr * (unsigned)nchunk);
    const int64_t j = j0 + jr;
    double *col = out + j * m;
    const double S = colsum[j];
#pragma unroll
    for (int q = 0; q < kDirichletChunkPerThread; ++q) {
        const int64_t i = (int64_t)c * kSampleChunk + q * kSampleThreads + (int)threadIdx.x;
        if (i < m)
            col[i] = col[i] / S;
    }
}

}  // namespace trlda
