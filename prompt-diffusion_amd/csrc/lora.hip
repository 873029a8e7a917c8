// LoRA merge (pd_lora_set_scales, lora.cpp): rebuilds one matrix parameter's rows of a WMat from its base copy,
//   W[n, k] = round_T( float(W0[n, k]) + sum_{j < R} (s_j * UT[j, n]) * D[j, k] )
// UT: [R][rows] fp32 (the up factors, transposed), D: [R][Kpad] fp32 in the WMat's row layout (k = tap * cin_pad + c, zero pad
// columns), s: one multiplier per column j (0 for an inactive adapter).  Source row n lands on the WMat row that upload_rows
// writes it to: row_off + n, or the 80 + 80 GEGLU interleave.  One thread owns 2 rows x 8 columns and sums over j in
// ascending order in fp32, with no split over R: the result does not depend on the launch and is bit-identical from run
// to run.  W0 is read and W written with 16-byte vector accesses; the D and UT chunks of 32 columns are staged in LDS.
//
// Adapters that are not a stack of rank-1 columns (pd_lora_add_ex: Hadamard, Kronecker, DoRA magnitude) go through two more
// kernels, per active adapter in load order.  lora_form_delta_kernel / lora_kron_delta_kernel write the adapter's scaled delta
// s * D as fp32 [rows][Kpad] in source-row order (pad columns 0); lora_form_apply_kernel, one block per row, adds it (or, under
// a magnitude m, (m / n)(W0 + s D) - W0 with n the row's 2-norm) to a running fp32 sum that starts at W0, and the last adapter's
// apply rounds the sum to T and writes it through the same row mapping as lora_merge_kernel.  The norm is summed per thread in
// ascending k and then over a fixed LDS tree: no atomics, no sum split over blocks.
#include "pd_common.h"

namespace {

constexpr int LM_ROWS = 64;      // rows per block (2 per thread)
constexpr int LM_COLS = 64;      // columns per block (8 per thread)
constexpr int LM_J = 32;         // rank columns staged per LDS round
constexpr int LM_THREADS = 256;

template <int DT> __device__ __forceinline__ void load8(const void* p, float* f) {
    if constexpr (DT == DT_F32) {
        const f32x4 a = reinterpret_cast<const f32x4*>(p)[0], b = reinterpret_cast<const f32x4*>(p)[1];
        f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3];
        f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
    } else {
        unpack8<DT>(*reinterpret_cast<const uint4*>(p), f);
    }
}
template <int DT> __device__ __forceinline__ void store8(void* p, const float* f) {
    if constexpr (DT == DT_F32) {
        reinterpret_cast<f32x4*>(p)[0] = f32x4{f[0], f[1], f[2], f[3]};
        reinterpret_cast<f32x4*>(p)[1] = f32x4{f[4], f[5], f[6], f[7]};
    } else {
        *reinterpret_cast<uint4*>(p) = pack8<DT>(f);
    }
}

template <int DT>
__global__ __launch_bounds__(LM_THREADS) void lora_merge_kernel(void* __restrict__ W, const void* __restrict__ W0, int rows, int row_off,
                                                                int geglu_half, int Kpad, const float* __restrict__ UT,
                                                                const float* __restrict__ D, const float* __restrict__ scale, int R) {
    __shared__ float Us[LM_J][LM_ROWS];
    __shared__ __attribute__((aligned(16))) float Ds[LM_J][LM_COLS];
    const int tid = threadIdx.x, tr = tid >> 3, tc = tid & 7;
    const int r_base = blockIdx.y * LM_ROWS, k_base = blockIdx.x * LM_COLS;
    const int k = k_base + tc * 8;
    float acc[2][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[0][e] = acc[1][e] = 0.f;
    for (int j0 = 0; j0 < R; j0 += LM_J) {
        __syncthreads();   // the previous chunk has been consumed
        for (int i = tid; i < LM_J * LM_COLS / 4; i += LM_THREADS) {
            const int jj = i / (LM_COLS / 4), c4 = (i % (LM_COLS / 4)) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (j0 + jj < R && k_base + c4 < Kpad) v = *reinterpret_cast<const f32x4*>(D + (size_t)(j0 + jj) * Kpad + k_base + c4);
            *reinterpret_cast<f32x4*>(&Ds[jj][c4]) = v;
        }
        for (int i = tid; i < LM_J * LM_ROWS; i += LM_THREADS) {
            const int jj = i / LM_ROWS, rr = i % LM_ROWS;
            float v = 0.f;
            if (j0 + jj < R && r_base + rr < rows) v = scale[j0 + jj] * UT[(size_t)(j0 + jj) * rows + r_base + rr];
            Us[jj][rr] = v;
        }
        __syncthreads();
        const int jn = min(LM_J, R - j0);
        for (int jj = 0; jj < jn; ++jj) {
            const f32x4 d0 = *reinterpret_cast<const f32x4*>(&Ds[jj][tc * 8]);
            const f32x4 d1 = *reinterpret_cast<const f32x4*>(&Ds[jj][tc * 8 + 4]);
            const float u0 = Us[jj][tr], u1 = Us[jj][tr + 32];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[0][e] = fmaf(u0, d0[e], acc[0][e]);
                acc[0][e + 4] = fmaf(u0, d1[e], acc[0][e + 4]);
                acc[1][e] = fmaf(u1, d0[e], acc[1][e]);
                acc[1][e + 4] = fmaf(u1, d1[e], acc[1][e + 4]);
            }
        }
    }
    if (k >= Kpad) return;   // Kpad is a multiple of 32: a thread's 8 columns are all inside or all outside
    constexpr int EB = DT == DT_F32 ? 4 : 2;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = r_base + tr + 32 * h;
        if (r >= rows) continue;
        int dst = row_off + r;
        if (geglu_half) {
            const int j = r < geglu_half ? r : r - geglu_half;
            dst = (j / 80) * 160 + (r < geglu_half ? 0 : 80) + j % 80;
        }
        float w[8];
        load8<DT>(reinterpret_cast<const char*>(W0) + ((size_t)(dst - row_off) * Kpad + k) * EB, w);
#pragma unroll
        for (int e = 0; e < 8; ++e) w[e] = w[e] + acc[h][e];
        store8<DT>(reinterpret_cast<char*>(W) + ((size_t)dst * Kpad + k) * EB, w);
    }
}

// one low-rank product into acc: acc[h][e] += sum_j (mul_j * UT[j, row]) * D[j, k], ascending j; mul_j = scale[j], or s when scale is null
__device__ __forceinline__ void rank_sum(float (&acc)[2][8], float (*Us)[LM_ROWS], float (*Ds)[LM_COLS], const float* __restrict__ UT,
                                         const float* __restrict__ D, const float* __restrict__ scale, float s, int R, int rows, int Kpad,
                                         int r_base, int k_base) {
    const int tid = threadIdx.x, tr = tid >> 3, tc = tid & 7;
    for (int j0 = 0; j0 < R; j0 += LM_J) {
        __syncthreads();   // the previous chunk has been consumed
        for (int i = tid; i < LM_J * LM_COLS / 4; i += LM_THREADS) {
            const int jj = i / (LM_COLS / 4), c4 = (i % (LM_COLS / 4)) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (j0 + jj < R && k_base + c4 < Kpad) v = *reinterpret_cast<const f32x4*>(D + (size_t)(j0 + jj) * Kpad + k_base + c4);
            *reinterpret_cast<f32x4*>(&Ds[jj][c4]) = v;
        }
        for (int i = tid; i < LM_J * LM_ROWS; i += LM_THREADS) {
            const int jj = i / LM_ROWS, rr = i % LM_ROWS;
            float v = 0.f;
            if (j0 + jj < R && r_base + rr < rows) v = (scale ? scale[j0 + jj] : s) * UT[(size_t)(j0 + jj) * rows + r_base + rr];
            Us[jj][rr] = v;
        }
        __syncthreads();
        const int jn = min(LM_J, R - j0);
        for (int jj = 0; jj < jn; ++jj) {
            const f32x4 d0 = *reinterpret_cast<const f32x4*>(&Ds[jj][tc * 8]);
            const f32x4 d1 = *reinterpret_cast<const f32x4*>(&Ds[jj][tc * 8 + 4]);
            const float u0 = Us[jj][tr], u1 = Us[jj][tr + 32];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[0][e] = fmaf(u0, d0[e], acc[0][e]);
                acc[0][e + 4] = fmaf(u0, d1[e], acc[0][e + 4]);
                acc[1][e] = fmaf(u1, d0[e], acc[1][e]);
                acc[1][e + 4] = fmaf(u1, d1[e], acc[1][e + 4]);
            }
        }
    }
}

// out[n, k] = (sum_j mul_j UT1[j, n] D1[j, k]) [HADA: * (sum_j UT2[j, n] D2[j, k])], fp32 [rows][Kpad] in source-row order
template <bool HADA>
__global__ __launch_bounds__(LM_THREADS) void lora_form_delta_kernel(float* __restrict__ out, int rows, int Kpad, const float* __restrict__ UT1,
                                                                     const float* __restrict__ D1, const float* __restrict__ scale, float s,
                                                                     int R1, const float* __restrict__ UT2, const float* __restrict__ D2,
                                                                     int R2) {
    __shared__ float Us[LM_J][LM_ROWS];
    __shared__ __attribute__((aligned(16))) float Ds[LM_J][LM_COLS];
    const int tid = threadIdx.x, tr = tid >> 3, tc = tid & 7;
    const int r_base = blockIdx.y * LM_ROWS, k_base = blockIdx.x * LM_COLS;
    const int k = k_base + tc * 8;
    float acc[2][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[0][e] = acc[1][e] = 0.f;
    rank_sum(acc, Us, Ds, UT1, D1, scale, s, R1, rows, Kpad, r_base, k_base);
    if constexpr (HADA) {
        float acc2[2][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc2[0][e] = acc2[1][e] = 0.f;
        rank_sum(acc2, Us, Ds, UT2, D2, nullptr, 1.f, R2, rows, Kpad, r_base, k_base);
#pragma unroll
        for (int e = 0; e < 8; ++e) { acc[0][e] *= acc2[0][e]; acc[1][e] *= acc2[1][e]; }
    }
    if (k >= Kpad) return;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = r_base + tr + 32 * h;
        if (r >= rows) continue;
        float* o = out + (size_t)r * Kpad + k;
        reinterpret_cast<f32x4*>(o)[0] = f32x4{acc[h][0], acc[h][1], acc[h][2], acc[h][3]};
        reinterpret_cast<f32x4*>(o)[1] = f32x4{acc[h][4], acc[h][5], acc[h][6], acc[h][7]};
    }
}

// out[i * c + p, tap * cin_pad + j * d + q] = (s * w1[i, j]) * w2[p, tap, q]; pad columns 0.  One thread: 4 columns of one row.
__global__ __launch_bounds__(LM_THREADS) void lora_kron_delta_kernel(float* __restrict__ out, int rows, int Kpad, int cin, int cin_pad, int taps,
                                                                     const float* __restrict__ w1, const float* __restrict__ w2, float s,
                                                                     int b, int c, int d) {
    const int n = blockIdx.y, k = (blockIdx.x * LM_THREADS + threadIdx.x) * 4;
    if (n >= rows || k >= Kpad) return;
    const int i = n / c, p = n % c;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const int tp = k / cin_pad, c0 = k % cin_pad;   // cin_pad is a multiple of 8: the 4 columns share a tap
    if (tp < taps) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int cc = c0 + e;
            if (cc < cin) v[e] = (s * w1[(size_t)i * b + cc / d]) * w2[((size_t)p * taps + tp) * d + cc % d];
        }
    }
    *reinterpret_cast<f32x4*>(out + (size_t)n * Kpad + k) = v;
}

// One block per source row n: sum[n, :] = (first ? W0 : sum)[n, :] + E[n, :], E = delta, or (mag[n] / |W0 + delta|_2)(W0 + delta) - W0;
// the last adapter rounds to T and writes W instead of sum.
template <int DT>
__global__ __launch_bounds__(LM_THREADS) void lora_form_apply_kernel(void* __restrict__ W, const void* __restrict__ W0, float* __restrict__ sum,
                                                                     const float* __restrict__ delta, const float* __restrict__ mag, int row_off,
                                                                     int geglu_half, int Kpad, int first, int last) {
    __shared__ float red[LM_THREADS];
    constexpr int EB = DT == DT_F32 ? 4 : 2;
    const int n = blockIdx.x, tid = threadIdx.x;
    int dst = row_off + n;
    if (geglu_half) {
        const int j = n < geglu_half ? n : n - geglu_half;
        dst = (j / 80) * 160 + (n < geglu_half ? 0 : 80) + j % 80;
    }
    const char* w0p = reinterpret_cast<const char*>(W0) + (size_t)(dst - row_off) * Kpad * EB;
    const float* dp = delta + (size_t)n * Kpad;
    float* sp = sum + (size_t)n * Kpad;
    float f = 1.f;
    if (mag) {
        float ss = 0.f;
        for (int k = tid * 8; k < Kpad; k += LM_THREADS * 8) {
            float w[8], t[8];
            load8<DT>(w0p + (size_t)k * EB, w);
            load8<DT_F32>(dp + k, t);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = w[e] + t[e];
                ss = fmaf(v, v, ss);
            }
        }
        red[tid] = ss;
        __syncthreads();
        for (int o = LM_THREADS / 2; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        const float nrm = sqrtf(red[0]);
        f = nrm > 0.f ? mag[n] / nrm : 0.f;
    }
    for (int k = tid * 8; k < Kpad; k += LM_THREADS * 8) {
        float w[8], t[8], a[8];
        load8<DT>(w0p + (size_t)k * EB, w);
        load8<DT_F32>(dp + k, t);
        if (!first) load8<DT_F32>(sp + k, a);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float ev = mag ? f * (w[e] + t[e]) - w[e] : t[e];
            a[e] = (first ? w[e] : a[e]) + ev;
        }
        if (last) store8<DT>(reinterpret_cast<char*>(W) + ((size_t)dst * Kpad + k) * EB, a);
        else store8<DT_F32>(sp + k, a);
    }
}

}  // namespace

int launch_lora_form_delta(float* out, int rows, int Kpad, const float* UT1, const float* D1, const float* scale, float s, int R1,
                           const float* UT2, const float* D2, int R2, hipStream_t st) {
    if (rows <= 0 || Kpad <= 0 || R1 <= 0 || Kpad % 32 != 0 || (UT2 && R2 <= 0)) return 1;
    const dim3 grid((Kpad + LM_COLS - 1) / LM_COLS, (rows + LM_ROWS - 1) / LM_ROWS);
    if (UT2)
        hipLaunchKernelGGL(lora_form_delta_kernel<true>, grid, dim3(LM_THREADS), 0, st, out, rows, Kpad, UT1, D1, scale, s, R1, UT2, D2, R2);
    else
        hipLaunchKernelGGL(lora_form_delta_kernel<false>, grid, dim3(LM_THREADS), 0, st, out, rows, Kpad, UT1, D1, scale, s, R1, UT2, D2, R2);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_lora_kron_delta(float* out, int rows, int Kpad, int cin, int cin_pad, int taps, const float* w1, const float* w2, float s, int a,
                           int b, hipStream_t st) {
    if (rows <= 0 || Kpad % 32 != 0 || cin_pad % 8 != 0 || a <= 0 || b <= 0 || rows % a != 0 || cin % b != 0 || taps * cin_pad > Kpad) return 1;
    const dim3 grid((Kpad / 4 + LM_THREADS - 1) / LM_THREADS, rows);
    hipLaunchKernelGGL(lora_kron_delta_kernel, grid, dim3(LM_THREADS), 0, st, out, rows, Kpad, cin, cin_pad, taps, w1, w2, s, b, rows / a, cin / b);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_lora_form_apply(int dt, void* W, const void* W0, float* sum, const float* delta, const float* mag, int rows, int row_off,
                           int geglu_half, int Kpad, int first, int last, hipStream_t st) {
    if (rows <= 0 || Kpad <= 0 || Kpad % 32 != 0) return 1;
    const dim3 grid(rows), blk(LM_THREADS);
    if (dt == DT_F16)
        hipLaunchKernelGGL(lora_form_apply_kernel<DT_F16>, grid, blk, 0, st, W, W0, sum, delta, mag, row_off, geglu_half, Kpad, first, last);
    else if (dt == DT_BF16)
        hipLaunchKernelGGL(lora_form_apply_kernel<DT_BF16>, grid, blk, 0, st, W, W0, sum, delta, mag, row_off, geglu_half, Kpad, first, last);
    else if (dt == DT_F32)
        hipLaunchKernelGGL(lora_form_apply_kernel<DT_F32>, grid, blk, 0, st, W, W0, sum, delta, mag, row_off, geglu_half, Kpad, first, last);
    else
        return 1;
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_lora_merge(int dt, void* W, const void* W0, int rows, int row_off, int geglu_half, int Kpad, const float* UT,
                      const float* D, const float* scale, int R, hipStream_t s) {
    if (rows <= 0 || Kpad <= 0 || R <= 0 || Kpad % 32 != 0) return 1;
    const dim3 grid((Kpad + LM_COLS - 1) / LM_COLS, (rows + LM_ROWS - 1) / LM_ROWS);
    if (dt == DT_F16)
        hipLaunchKernelGGL(lora_merge_kernel<DT_F16>, grid, dim3(LM_THREADS), 0, s, W, W0, rows, row_off, geglu_half, Kpad, UT, D, scale, R);
    else if (dt == DT_BF16)
        hipLaunchKernelGGL(lora_merge_kernel<DT_BF16>, grid, dim3(LM_THREADS), 0, s, W, W0, rows, row_off, geglu_half, Kpad, UT, D, scale, R);
    else if (dt == DT_F32)
        hipLaunchKernelGGL(lora_merge_kernel<DT_F32>, grid, dim3(LM_THREADS), 0, s, W, W0, rows, row_off, geglu_half, Kpad, UT, D, scale, R);
    else
        return 1;
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
