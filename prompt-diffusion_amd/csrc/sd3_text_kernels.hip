// Small kernels of the SD3 text encoders (sd3_text.cpp, and text.cpp for the two CLIP ones): T5's token embedding, row RMSNorm, the Toeplitz rows of its relative-position
// bias, the EOS-row gather of the CLIP pooling and the strided write into the joint prompt_embeds layout.  All HBM-trivial next to the
// encoders' GEMMs; the contractions and the attention are the shared kernels (gemm.hip, attention.hip).
#include "pd_common.h"

namespace {

constexpr int TPB = 256;
inline int nblocks(long long n, int per = TPB, int cap = 65535 * 16) {
    long long b = (n + per - 1) / per;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

// embed_tokens_kernel (elementwise.hip) minus the positions, into the fp32 residual stream
__global__ void embed_rows_kernel(const int* __restrict__ ids, const void* __restrict__ tok, int tok_ld, int dt, float* __restrict__ out,
                                  long long rows, int C, int vocab) {
    const long long total = rows * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        int id = ids[i / C];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        out[i] = dt == DT_F32 ? reinterpret_cast<const float*>(tok)[(size_t)id * tok_ld + c]
                              : cvt32_rt(reinterpret_cast<const uint16_t*>(tok)[(size_t)id * tok_ld + c], dt);
    }
}

// one wave per row, like layernorm_kernel, but looping over the row (d_model 4096 does not fit its register tile): the second
// read of the row comes from L2.  No mean, no bias (T5LayerNorm).  C % 4 == 0.
__global__ __launch_bounds__(256) void rmsnorm_rows_kernel(const float* __restrict__ x, void* __restrict__ y, int y_dt, const float* __restrict__ w,
                                                            long long rows, int C, float eps, int rows_per_sample, int y_sample_rows, int y_row_off,
                                                            int y_ld) {
    const int lane = threadIdx.x & 63;
    const long long row = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + (size_t)row * C;
    float q = 0.f;
    for (int v = lane; v < C / 4; v += 64) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(xr + v * 4);
        q += (t[0] * t[0] + t[1] * t[1]) + (t[2] * t[2] + t[3] * t[3]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = 1.0f / sqrtf(q / (float)C + eps);
    size_t orow = (size_t)row;
    if (y_sample_rows) {
        const long long b = row / rows_per_sample;
        orow = (size_t)(b * y_sample_rows + y_row_off + (row - b * rows_per_sample));
    }
    for (int v = lane; v < C / 4; v += 64) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(xr + v * 4);
        const f32x4 g = *reinterpret_cast<const f32x4*>(w + v * 4);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = g[j] * (t[j] * rstd);
        store4(y, orow * y_ld + (size_t)v * 4, y_dt, o);
    }
}

__global__ void t5_relbias_kernel(const int* __restrict__ bucket, const void* __restrict__ table, int ld, int dt, float* __restrict__ relbias,
                                  int heads, int n) {
    const int total = heads * n;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int h = i / n, d = i - h * n;
        const size_t at = (size_t)bucket[d] * ld + h;
        const float v = dt == DT_F32 ? reinterpret_cast<const float*>(table)[at] : cvt32_rt(reinterpret_cast<const uint16_t*>(table)[at], dt);
        relbias[i] = v * 1.4426950408889634f;
    }
}

__global__ void joint_write_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int rows_per_sample, int C, int width,
                                   int dst_sample_rows, int dst_ld, int c_off) {
    const long long total = (long long)B * rows_per_sample * width;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % width);
        const long long br = i / width;
        const int r = (int)(br % rows_per_sample);
        const long long b = br / rows_per_sample;
        dst[((size_t)b * dst_sample_rows + r) * dst_ld + c_off + c] = c < C ? src[(size_t)br * C + c] : 0.f;
    }
}

// one block per sample: thread 0 finds the position (L <= 512 ids: a serial scan of at most 2 KB), the block copies the row
__global__ __launch_bounds__(256) void eos_gather_kernel(const int* __restrict__ ids, const float* __restrict__ x, float* __restrict__ out, int L, int C,
                                                          int eos_id) {
    __shared__ int s_pos;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        const int* r = ids + (size_t)b * L;
        int pos = 0;
        if (eos_id == 2) {   // argmax, first maximum (torch.argmax's tie rule for the padded EOS run)
            int best = r[0];
            for (int l = 1; l < L; ++l)
                if (r[l] > best) { best = r[l]; pos = l; }
        } else {             // first match; none: (ids == eos).argmax() = 0
            for (int l = 0; l < L; ++l)
                if (r[l] == eos_id) { pos = l; break; }
        }
        s_pos = pos;
    }
    __syncthreads();
    const float* src = x + ((size_t)b * L + s_pos) * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) out[(size_t)b * C + c] = src[c];
}

}  // namespace

int launch_embed_rows(const int* ids, const void* tok, int tok_ld, int dt, float* out, long long rows, int C, int vocab, hipStream_t s) {
    hipLaunchKernelGGL(embed_rows_kernel, dim3(nblocks(rows * C)), dim3(TPB), 0, s, ids, tok, tok_ld, dt, out, rows, C, vocab);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_rmsnorm_rows(const float* x, void* y, int y_dt, const float* w, long long rows, int C, float eps, int rows_per_sample, int y_sample_rows,
                        int y_row_off, int y_ld, hipStream_t s) {
    if (rows < 1 || C % 4 || y_ld % 4 || rows_per_sample < 1) return 1;
    hipLaunchKernelGGL(rmsnorm_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, y, y_dt, w, rows, C, eps, rows_per_sample,
                       y_sample_rows, y_row_off, y_ld);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_t5_relbias(const int* bucket, const void* table, int ld, int dt, float* relbias, int heads, int n, hipStream_t s) {
    hipLaunchKernelGGL(t5_relbias_kernel, dim3(nblocks((long long)heads * n)), dim3(TPB), 0, s, bucket, table, ld, dt, relbias, heads, n);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_joint_write(const float* src, float* dst, int B, int rows_per_sample, int C, int width, int dst_sample_rows, int dst_ld, int c_off,
                       hipStream_t s) {
    if (width < C || c_off + width > dst_ld || rows_per_sample > dst_sample_rows) return 1;
    hipLaunchKernelGGL(joint_write_kernel, dim3(nblocks((long long)B * rows_per_sample * width)), dim3(TPB), 0, s, src, dst, B, rows_per_sample, C,
                       width, dst_sample_rows, dst_ld, c_off);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_eos_gather(const int* ids, const float* x, float* out, int B, int L, int C, int eos_id, hipStream_t s) {
    hipLaunchKernelGGL(eos_gather_kernel, dim3(B), dim3(256), 0, s, ids, x, out, L, C, eos_id);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
