// LoRA merge (pd_lora_set_scales, lora.cpp): rebuilds one matrix parameter's rows of a WMat from its base copy,
//   W[n, k] = round_T( float(W0[n, k]) + sum_{j < R} (s_j * UT[j, n]) * D[j, k] )
// UT: [R][rows] fp32 (the up factors, transposed), D: [R][Kpad] fp32 in the WMat's row layout (k = tap * cin_pad + c, zero pad
// columns), s: one multiplier per column j (0 for an inactive adapter).  Source row n lands on the WMat row that upload_rows
// writes it to: row_off + n, or the 80 + 80 GEGLU interleave.  One thread owns 2 rows x 8 columns and sums over j in
// ascending order in fp32, with no split over R: the result does not depend on the launch and is bit-identical from run
// to run.  W0 is read and W written with 16-byte vector accesses; the D and UT chunks of 32 columns are staged in LDS.
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

}  // namespace

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
