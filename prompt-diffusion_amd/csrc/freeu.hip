// FreeU (Si et al., arXiv:2309.11497, as diffusers' apply_freeu / fourier_filter restate it): the skip concat of the first
// two decoder stages with the backbone half amplified and the skip half's lowest frequencies attenuated, in one launch.
//   out[r, 0:Ch]     = (h + h_add)[r, c] * (c < Ch / 2 ? b : 1)
//   out[r, Ch:Ch+Cs] = fourier_filter(skip + skip_add, threshold 1, scale s)   per (sample, channel) plane of H x W
// fourier_filter scales X[ky, kx] of the plane's 2-D DFT on the band fftshift puts at [H/2-1, H/2+1) x [W/2-1, W/2+1), which is
// the frequencies {0, -1} per axis ({0} on an axis of length 1).  So no FFT is needed:
//   y[n] = x[n] + (s - 1) / (H W) * sum_{(ky, kx) in Ky x Kx} Re(X[ky, kx] e^{+2 pi i (ky ny / H + kx nx / W)})
// and the four coefficients X[0,0], X[0,-1], X[-1,0], X[-1,-1] are 7 real sums over the plane:
//   S0 = sum x,  (Cx, Sx) = sum x (cos, sin) tx,  (Cy, Sy) = sum x (cos, sin) ty,  (Cxy, Sxy) = sum x (cos, sin) (ty + tx)
// with ty = 2 pi my / H, tx = 2 pi mx / W (the frequency -1 puts e^{+i t} in the forward sum), and
//   y[n] = x[n] + k (S0 + Cx cos tx + Sx sin tx + Cy cos ty + Sy sin ty + Cxy cos(ty+tx) + Sxy sin(ty+tx)),  k = (s - 1) / (H W)
// where the x terms drop when W == 1, the y terms when H == 1, and the xy terms when either is 1.
//
// Layout: NHWC rows (r = sample * H * W + pixel, channels contiguous) in the storage type dt (f32 / f16 / bf16), fp32 arithmetic.
// Blocks [0, B * slices): one block per (sample, 64-channel slice of the skip).  Its 16 channel groups of 4 x 16 pixel lanes
// first reduce the 7 sums per channel over the plane (each pixel row segment is one 128- / 256-byte coalesced access), reduce
// across lanes and waves in a fixed order, then re-read the plane (from L2: the block read it a moment ago) and write the
// filtered skip half.  The twiddles come from the integer phases my / H and mx / W (sincospif of an argument in [0, 2)), kept in
// LDS per block; cos / sin of ty + tx by angle addition.  Blocks [B * slices, grid): the backbone half, grid-stride.
// skip / skip_add may hold only the first skip_rows / skip_add_rows rows (tensors shared by the two halves of a CFG batch),
// like concat_add.
#include "pd_common.h"

namespace {

constexpr int FU_TPB = 256;
constexpr int FU_CG = 16;                // 4-channel groups per block: a 64-channel slice of the skip
constexpr int FU_PL = FU_TPB / FU_CG;    // pixel lanes per block
constexpr int FU_NS = 7;                 // S0, Cx, Sx, Cy, Sy, Cxy, Sxy
constexpr int FU_MAX_HW_SUM = 4096;      // H + W: the twiddle tables (2 (H + W) floats of dynamic LDS)

__global__ __launch_bounds__(FU_TPB) void freeu_concat_kernel(
    const void* __restrict__ h, const void* __restrict__ h_add, const void* __restrict__ skip, const void* __restrict__ skip_add,
    void* __restrict__ out, int dt, int B, int H, int W, int Ch, int Cs, long long skip_rows, long long skip_add_rows, float s,
    float b, int n_skip_blocks) {
    const int HW = H * W;
    const int Ct = Ch + Cs;
    if ((int)blockIdx.x >= n_skip_blocks) {
        // backbone half: h[:, :Ch // 2] *= b after the (mid-block) control residual
        const int Ch4 = Ch / 4, half = Ch / 2;
        const long long total = (long long)B * HW * Ch4;
        const long long stride = (long long)(gridDim.x - n_skip_blocks) * FU_TPB;
        for (long long i = (long long)(blockIdx.x - n_skip_blocks) * FU_TPB + threadIdx.x; i < total; i += stride) {
            const int c = (int)(i % Ch4) * 4;
            const long long r = i / Ch4;
            f32x4 x = load4(h, (size_t)r * Ch + c, dt);
            if (h_add) x += load4(h_add, (size_t)r * Ch + c, dt);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c + j < half) x[j] *= b;
            store4(out, (size_t)r * Ct + c, dt, x);
        }
        return;
    }
    extern __shared__ float tw[];   // [H] cos ty, [H] sin ty, [W] cos tx, [W] sin tx
    __shared__ f32x4 red[FU_TPB / 64][FU_CG][FU_NS];
    __shared__ f32x4 fin[FU_CG][FU_NS];
    float* cyt = tw;
    float* syt = tw + H;
    float* cxt = tw + 2 * H;
    float* sxt = tw + 2 * H + W;
    for (int m = threadIdx.x; m < H; m += FU_TPB) sincospif(2.0f * (float)m / (float)H, &syt[m], &cyt[m]);
    for (int m = threadIdx.x; m < W; m += FU_TPB) sincospif(2.0f * (float)m / (float)W, &sxt[m], &cxt[m]);
    __syncthreads();

    const int slices = (Cs + 4 * FU_CG - 1) / (4 * FU_CG);
    const int n = blockIdx.x / slices;
    const int cg = threadIdx.x % FU_CG;
    const int c = (blockIdx.x % slices) * (4 * FU_CG) + cg * 4;
    const int pl = threadIdx.x / FU_CG;
    const bool active = c < Cs;
    const bool hy = H > 1, wx = W > 1;
    const long long r0 = (long long)n * HW;
    auto src = [&](int p) {
        const long long r = r0 + p;
        f32x4 x = load4(skip, (size_t)(r >= skip_rows ? r - skip_rows : r) * Cs + c, dt);
        if (skip_add) x += load4(skip_add, (size_t)(r >= skip_add_rows ? r - skip_add_rows : r) * Cs + c, dt);
        return x;
    };

    f32x4 acc[FU_NS];
#pragma unroll
    for (int k = 0; k < FU_NS; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (active) {
        for (int p = pl; p < HW; p += FU_PL) {
            const int my = p / W, mx = p - my * W;
            const float cy = cyt[my], sy = syt[my], cx = cxt[mx], sx = sxt[mx];
            const f32x4 x = src(p);
            acc[0] += x;
            acc[1] += x * cx;
            acc[2] += x * sx;
            acc[3] += x * cy;
            acc[4] += x * sy;
            acc[5] += x * (cy * cx - sy * sx);
            acc[6] += x * (sy * cx + cy * sx);
        }
    }
    // the 4 pixel lanes of a wave (lane bits 4 and 5), then the 4 waves in order
#pragma unroll
    for (int k = 0; k < FU_NS; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = acc[k][j];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            acc[k][j] = v;
        }
    const int wave = threadIdx.x / 64;
    if ((threadIdx.x & 63) < FU_CG)
#pragma unroll
        for (int k = 0; k < FU_NS; ++k) red[wave][cg][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < FU_CG * FU_NS) {
        const int g = threadIdx.x / FU_NS, k = threadIdx.x % FU_NS;
        f32x4 v = red[0][g][k];
#pragma unroll
        for (int w = 1; w < FU_TPB / 64; ++w) v += red[w][g][k];
        fin[g][k] = v;
    }
    __syncthreads();
    if (!active) return;
    f32x4 sum[FU_NS];
#pragma unroll
    for (int k = 0; k < FU_NS; ++k) sum[k] = fin[cg][k];
    const float kf = (s - 1.0f) / (float)HW;
    for (int p = pl; p < HW; p += FU_PL) {
        const int my = p / W, mx = p - my * W;
        const float cy = cyt[my], sy = syt[my], cx = cxt[mx], sx = sxt[mx];
        f32x4 corr = sum[0];
        if (wx) corr += sum[1] * cx + sum[2] * sx;
        if (hy) corr += sum[3] * cy + sum[4] * sy;
        if (wx && hy) corr += sum[5] * (cy * cx - sy * sx) + sum[6] * (sy * cx + cy * sx);
        const f32x4 y = src(p) + corr * kf;
        store4(out, (size_t)(r0 + p) * Ct + Ch + c, dt, y);
    }
}

}  // namespace

int launch_freeu_concat(const void* h, const void* h_add, const void* skip, const void* skip_add, void* out, int dt, int B, int H,
                        int W, int Ch, int Cs, float s, float b, hipStream_t st, long long skip_rows, long long skip_add_rows) {
    if (B < 1 || H < 1 || W < 1 || Ch < 4 || Cs < 4 || Ch % 4 || Cs % 4 || H + W > FU_MAX_HW_SUM) return 1;
    if (dt != DT_F32 && dt != DT_F16 && dt != DT_BF16) return 1;
    const long long rows = (long long)B * H * W;
    if (skip_rows <= 0) skip_rows = rows;
    if (skip_add_rows <= 0) skip_add_rows = rows;
    if (rows > 2 * skip_rows || rows > 2 * skip_add_rows) return 1;
    // the broadcast halves must be whole samples
    if (skip_rows % ((long long)H * W) || skip_add_rows % ((long long)H * W)) return 1;
    const long long n_skip = (long long)B * ((Cs + 4 * FU_CG - 1) / (4 * FU_CG));
    long long n_h = (rows * (Ch / 4) + FU_TPB - 1) / FU_TPB;
    if (n_h > 4096) n_h = 4096;
    if (n_skip + n_h > 0x7fffffffLL) return 1;
    const size_t lds = (size_t)2 * (H + W) * sizeof(float);
    hipLaunchKernelGGL(freeu_concat_kernel, dim3((unsigned)(n_skip + n_h)), dim3(FU_TPB), lds, st, h, h_add, skip, skip_add, out,
                       dt, B, H, W, Ch, Cs, skip_rows, skip_add_rows, s, b, (int)n_skip);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
