// Perturbed-attention guidance (Ahn et al., arXiv:2403.17377, as diffusers' PAGCFGIdentitySelfAttnProcessor2_0 restates it): in a
// perturbed block the self-attention map of the perturbed samples is the identity, so their attn1 is to_out(V) and no softmax runs.
// The QKV GEMM has already written V transposed for the attention kernel, VT [B][C][npad]; attn1.to_out reads token rows.  This
// kernel is that change of layout and nothing else (gfx950):
//   att[b, n, c] = VT[src + b, c, n]      b < count, n < N, c < C
// A bit copy of the storage type (2-byte modes; the 4-byte storage of f32 and f16x2), so it is instantiated over the element width
// only.  One block moves a 64 x 64 tile through LDS: it reads 64 rows of VT, a wave per row segment of 64 consecutive tokens (128 /
// 256 contiguous bytes), and writes 64 token rows of 64 consecutive channels the same way.  The LDS row stride is an odd number of
// dwords (33 for 2-byte elements, 65 for 4-byte ones), so the 32 lanes of a half wave that walk down a tile column in the second
// phase sit on 32 different banks; the first phase writes along a row.  Edge tiles mask both phases by n < N and c < C: N and C need
// not be multiples of 64, and the pad columns of VT (n >= N) are never read.
#include "pd_common.h"

namespace {

constexpr int PAG_TILE = 64;
constexpr int PAG_TPB = 256;

template <typename U>
__global__ __launch_bounds__(PAG_TPB) void pag_identity_kernel(const U* __restrict__ VT, U* __restrict__ att, int N, int C, int npad) {
    constexpr int LD = PAG_TILE + (sizeof(U) == 2 ? 2 : 1);
    __shared__ U tile[PAG_TILE][LD];
    const int n0 = blockIdx.x * PAG_TILE, c0 = blockIdx.y * PAG_TILE;
    const int tx = threadIdx.x % PAG_TILE, ty = threadIdx.x / PAG_TILE;
    const U* __restrict__ src = VT + (size_t)blockIdx.z * C * npad;
    U* __restrict__ dst = att + (size_t)blockIdx.z * N * C;
    for (int j = ty; j < PAG_TILE; j += PAG_TPB / PAG_TILE) {
        const int c = c0 + j, n = n0 + tx;
        if (c < C && n < N) tile[j][tx] = src[(size_t)c * npad + n];
    }
    __syncthreads();
    for (int j = ty; j < PAG_TILE; j += PAG_TPB / PAG_TILE) {
        const int n = n0 + j, c = c0 + tx;
        if (n < N && c < C) dst[(size_t)n * C + c] = tile[tx][j];
    }
}

}  // namespace

// VT [.][C][npad] and att [count][N][C] in a storage type of elem_bytes (2 or 4); samples [src, src + count) of VT.  0 launched,
// 1 refused or launch failure
int launch_pag_identity(const void* VT, void* att, int elem_bytes, int src, int count, int N, int C, int npad, hipStream_t s) {
    if (!VT || !att || src < 0 || count < 1 || count > 65535 || N < 1 || C < 1 || npad < N || (elem_bytes != 2 && elem_bytes != 4)) return 1;
    const dim3 grid((N + PAG_TILE - 1) / PAG_TILE, (C + PAG_TILE - 1) / PAG_TILE, count);
    if (grid.y > 65535) return 1;
    const size_t off = (size_t)src * C * npad;
    if (elem_bytes == 2)
        hipLaunchKernelGGL(pag_identity_kernel<uint16_t>, grid, dim3(PAG_TPB), 0, s, reinterpret_cast<const uint16_t*>(VT) + off,
                           reinterpret_cast<uint16_t*>(att), N, C, npad);
    else
        hipLaunchKernelGGL(pag_identity_kernel<uint32_t>, grid, dim3(PAG_TPB), 0, s, reinterpret_cast<const uint32_t*>(VT) + off,
                           reinterpret_cast<uint32_t*>(att), N, C, npad);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
