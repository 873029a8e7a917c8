// pdengine: the Canny edge detector (host side in canny.cpp; contract in include/pdengine.h, "Canny edge detector").  The arithmetic is
// a restatement of OpenCV's portable C++ path (canny.cpp, aperture 3, L2gradient = false); all of it is integer, so the edge map is the
// same bytes as the NumPy restatement in tests/canny_ref.py:
//   thresholds  lo = floor(low), hi = floor(high), swapped if lo > hi (done by the host side)
//   gradients   3x3 Sobel per channel in int32 over replicated borders:
//                 dx = (p[-1,+1] + 2 p[0,+1] + p[+1,+1]) - (p[-1,-1] + 2 p[0,-1] + p[+1,-1])   ([row, col] offsets), dy the transpose
//   magnitude   n = |dx| + |dy|; with three channels a pixel takes dx, dy, m = n of the channel with the largest n, the lowest index on a
//               tie (a strict > scan); m counts as 0 outside the picture on all four sides
//   candidates  m > lo and, with x = |dx|, y = |dy| << 15, t22 = x * 13573, t67 = t22 + (x << 16):
//                 y < t22 (horizontal gradient)  m > m[0,-1] and m >= m[0,+1]
//                 else y > t67 (vertical)        m > m[-1,0] and m >= m[+1,0]
//                 else (diagonal)                s = (dx ^ dy) < 0 ? -1 : +1;  m > m[-1,-s] and m > m[+1,+s]
//   strong      a candidate with m > hi; the others are weak
//   hysteresis  a weak pixel that is 8-connected, through candidates, to a strong one becomes strong; 255 at strong pixels, 0 elsewhere
// Three kernels over a state map [B][H][W] of one byte per pixel (PD_CANNY_NONE / WEAK / STRONG):
//   canny_nms_kernel         u8 NHWC source -> states.  One block per 16 x 64 tile: the source tile with a 2-pixel halo (coordinates
//                            clamped: the replicated border) in LDS, dx / dy / m of the tile plus a 1-pixel ring, then the tests above
//   canny_hysteresis_kernel  one sweep.  One block per 64 x 64 tile: the tile's states plus a 1-pixel halo in LDS, "a weak pixel with a
//                            strong 8-neighbour becomes strong" -- 16 pixels of a row per thread, as bit masks squeezed out of
//                            aligned words -- repeated until a block-wide vote says nothing changed (at most one round per pixel
//                            of the tile); a tile that changed is written back and raises *flag
//   canny_emit_kernel        states -> u8 0 / 255 and / or three equal fp32 channels (v / 255) * mul + add
// The host relaunches the sweep until one raises no flag.  The update is monotone (weak -> strong only, and only next to a strong
// pixel), so the states climb to the one least fixed point -- every weak pixel connected to a strong one -- whatever the order in which
// threads, tiles and launches see each other's writes: a halo read during a launch returns the old or the new byte of a neighbouring
// tile, and either is a state on the way to that fixed point.  A launch that raises no flag read only final values, so it proves the
// fixed point.  The number of sweeps may differ from run to run; the bytes may not.  No floating point before the emit kernel.
#include "pd_common.h"

namespace {

constexpr int TPB = 256;
constexpr int NONE = CANNY_NONE, WEAK = CANNY_WEAK, STRONG = CANNY_STRONG;
// canny_nms_kernel's tile
constexpr int NTX = 64, NTY = 16;
constexpr int SRC_W = NTX + 4, SRC_H = NTY + 4;     // source patch: 2-pixel halo
constexpr int RING_W = NTX + 2, RING_H = NTY + 2;   // gradients: 1-pixel ring
constexpr int TG22 = 13573;                         // tan(22.5 deg) * 2^15
// canny_hysteresis_kernel's tile: a thread owns HRUN neighbouring pixels of a row
constexpr int HT = 64, HRUN = HT * HT / TPB, HPITCH = 96, HX0 = 16;   // row pitch and first tile column, in bytes
constexpr int PX = 4;                               // canny_emit_kernel: pixels per thread

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <int C>
__global__ __launch_bounds__(TPB) void canny_nms_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ states, int H, int W,
                                                         int tiles_x, int tiles_y, int lo, int hi) {
    __shared__ uint8_t s_src[C][SRC_H][SRC_W];
    __shared__ short s_dx[RING_H][RING_W], s_dy[RING_H][RING_W], s_m[RING_H][RING_W];   // |dx|, |dy| <= 1020, m <= 2040
    const int tid = threadIdx.x;
    const int tx0 = (int)(blockIdx.x % tiles_x) * NTX;
    const int ty0 = (int)((blockIdx.x / tiles_x) % tiles_y) * NTY;
    const long long b = blockIdx.x / ((long long)tiles_x * tiles_y);
    const uint8_t* img = src + b * H * W * C;
    for (int i = tid; i < SRC_H * SRC_W; i += TPB) {
        const int ry = i / SRC_W, rx = i % SRC_W;
        const int gy = clampi(ty0 - 2 + ry, H - 1), gx = clampi(tx0 - 2 + rx, W - 1);
        const uint8_t* p = img + ((long long)gy * W + gx) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) s_src[c][ry][rx] = p[c];
    }
    __syncthreads();
    for (int i = tid; i < RING_H * RING_W; i += TPB) {
        const int ry = i / RING_W, rx = i % RING_W;
        const int gy = ty0 - 1 + ry, gx = tx0 - 1 + rx;
        int dx = 0, dy = 0, m = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const uint8_t(*q)[SRC_W] = s_src[c];
                const int y = ry + 1, x = rx + 1;   // the pixel in patch coordinates
                const int a00 = q[y - 1][x - 1], a01 = q[y - 1][x], a02 = q[y - 1][x + 1];
                const int a10 = q[y][x - 1], a12 = q[y][x + 1];
                const int a20 = q[y + 1][x - 1], a21 = q[y + 1][x], a22 = q[y + 1][x + 1];
                const int cdx = (a02 + 2 * a12 + a22) - (a00 + 2 * a10 + a20);
                const int cdy = (a20 + 2 * a21 + a22) - (a00 + 2 * a01 + a02);
                const int n = abs(cdx) + abs(cdy);
                if (c == 0 || n > m) { dx = cdx; dy = cdy; m = n; }
            }
        }
        s_dx[ry][rx] = (short)dx;
        s_dy[ry][rx] = (short)dy;
        s_m[ry][rx] = (short)m;
    }
    __syncthreads();
    uint8_t* out = states + b * H * W;
    for (int i = tid; i < NTY * NTX; i += TPB) {
        const int py = i / NTX, px = i % NTX;
        const int gy = ty0 + py, gx = tx0 + px;
        if (gy >= H || gx >= W) continue;
        const int y = py + 1, x = px + 1;           // the pixel in ring coordinates
        const int m = s_m[y][x];
        int st = NONE;
        if (m > lo) {
            const int dx = s_dx[y][x], dy = s_dy[y][x];
            // |dx|, |dy| <= 1020, so t67 <= 1020 * 79109 < 2^27 would fit 32 bits; 64 bits keep the line free of that argument
            const long long ax = abs(dx), ay = (long long)abs(dy) << 15;
            const long long t22 = ax * TG22, t67 = t22 + (ax << 16);
            bool keep;
            if (ay < t22) {
                keep = m > s_m[y][x - 1] && m >= s_m[y][x + 1];
            } else if (ay > t67) {
                keep = m > s_m[y - 1][x] && m >= s_m[y + 1][x];
            } else {
                const int s = (dx ^ dy) < 0 ? -1 : 1;
                keep = m > s_m[y - 1][x - s] && m > s_m[y + 1][x + s];
            }
            if (keep) st = m > hi ? STRONG : WEAK;
        }
        out[(long long)gy * W + gx] = (uint8_t)st;
    }
}

// bit j of the result = bit `bit` of byte j of d (the four products land on bits 24 .. 27 and nothing carries into them)
__device__ __forceinline__ uint32_t byte_bits(uint32_t d, int bit) { return (((d >> bit) & 0x01010101u) * 0x01020408u) >> 24; }
// ... and back: byte j of the result = 3 where bit j of the low four bits of m is set, else 0
__device__ __forceinline__ uint32_t bits_to_bytes3(uint32_t m) { return (((m & 0xfu) * 0x00204081u) & 0x01010101u) * 3u; }

__global__ __launch_bounds__(TPB) void canny_hysteresis_kernel(uint8_t* states, int H, int W, int tiles_x, int tiles_y, int* flag) {
    // Row r of the tile is row r + 1 here and column c is byte HX0 + c of it, so a thread's HRUN = 16 pixels are four aligned dwords;
    // the halo columns are bytes HX0 - 1 and HX0 + HT, the bytes beyond them zero.  Anything but WEAK / STRONG is held as NONE.
    __shared__ uint32_t s_words[(HT + 2) * HPITCH / 4];
    uint8_t* s_bytes = reinterpret_cast<uint8_t*>(s_words);
    // threads read the words their neighbours promote pixels in while a round is under way; any mix of old and new is a valid state
    volatile uint32_t* sv = s_words;
    const int tid = threadIdx.x;
    const int tx0 = (int)(blockIdx.x % tiles_x) * HT;
    const int ty0 = (int)((blockIdx.x / tiles_x) % tiles_y) * HT;
    const long long b = blockIdx.x / ((long long)tiles_x * tiles_y);
    uint8_t* map = states + b * H * W;
    for (int i = tid; i < (HT + 2) * HPITCH / 4; i += TPB) s_words[i] = 0;
    __syncthreads();
    for (int i = tid; i < (HT + 2) * (HT + 2); i += TPB) {
        const int ry = i / (HT + 2), rx = i % (HT + 2);
        const int gy = ty0 - 1 + ry, gx = tx0 - 1 + rx;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const uint8_t v = map[(long long)gy * W + gx];
            s_bytes[ry * HPITCH + HX0 - 1 + rx] = (v == WEAK || v == STRONG) ? v : (uint8_t)NONE;
        }
    }
    __syncthreads();
    const int y = tid / (HT / HRUN) + 1, seg = tid % (HT / HRUN);     // this thread's run: row y, columns 16 seg .. 16 seg + 15
    const int w0 = (y * HPITCH + HX0 + seg * HRUN) / 4;               // its first word
    // strong pixels of the 24 bytes from 4 left of the run to 4 right of it, in the row `up` rows above: bit k = byte k
    auto strong24 = [&](int up) -> uint32_t {
        const int w = w0 - up * (HPITCH / 4) - 1;
        uint32_t m = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) m |= byte_bits(sv[w + k], 1) << (4 * k);
        return m;
    };
    // A round promotes at least one pixel or is the last, and the tile has HT * HT pixels: the bound is never what ends the loop on a
    // converging tile, and a tile it did cut short has raised the flag, so the host sweeps again.
    int tile_changed = 0;
    for (int round = 0; round < HT * HT; ++round) {
        uint32_t own[4], weak = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            own[k] = sv[w0 + k];
            weak |= byte_bits(own[k], 0) << (4 * k);
        }
        uint32_t grown = 0;
        if (weak) {
            weak <<= 4;                                               // bit 4 + j: pixel j of the run, as in strong24
            const uint32_t nb = strong24(1) | strong24(0) | strong24(-1);
            grown = weak & (nb | (nb << 1) | (nb >> 1));          // weak pixels with a strong 8-neighbour
            // ... and the weak pixels of the run that those reach along it: a round carries a promotion from either end of the run to
            // the other.  (Runs down the columns as well, in the byte-wise first version of this kernel, made the rounds cost more than
            // they saved.)
            for (int j = 1; j < HRUN && grown; ++j) {
                const uint32_t next = grown | (weak & ((grown << 1) | (grown >> 1)));
                if (next == grown) break;
                grown = next;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t flip = bits_to_bytes3(grown >> (4 + 4 * k));   // WEAK ^ 3 = STRONG
                if (flip) sv[w0 + k] = own[k] ^ flip;
            }
        }
        if (!__syncthreads_or(grown != 0)) break;
        tile_changed = 1;
    }
    if (!tile_changed) return;   // uniform over the block
    const int gy = ty0 + y - 1;
    for (int j = 0; j < HRUN; ++j) {
        const int gx = tx0 + seg * HRUN + j;
        if (gy < H && gx < W && s_bytes[y * HPITCH + HX0 + seg * HRUN + j] == STRONG) map[(long long)gy * W + gx] = (uint8_t)STRONG;
    }
    if (tid == 0) *flag = 1;
}

// One thread: PX neighbouring pixels of the flattened H * W of one sample.  vec_s / vec_u8: HW % 4 == 0 and the pointer 4-byte aligned;
// vec_f: HW % 4 == 0 and dst_f 16-byte aligned.
__global__ __launch_bounds__(TPB) void canny_emit_kernel(const uint8_t* __restrict__ states, uint8_t* __restrict__ dst_u8,
                                                          float* __restrict__ dst_f, int B, long long HW, int Cf, int c_off, float mul, float add,
                                                          int vec_s, int vec_u8, int vec_f) {
    const long long gp = (HW + PX - 1) / PX;
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long long)B * gp) return;
    const long long p0 = (i % gp) * PX, b = i / gp;
    const int n = (int)(HW - p0 < PX ? HW - p0 : PX);
    const uint8_t* sp = states + b * HW + p0;
    int v[PX];
    if (vec_s && n == PX) {
        const uint32_t u = *reinterpret_cast<const uint32_t*>(sp);
#pragma unroll
        for (int p = 0; p < PX; ++p) v[p] = ((u >> (8 * p)) & 0xffu) == STRONG ? 255 : 0;
    } else {
#pragma unroll
        for (int p = 0; p < PX; ++p) v[p] = (p < n && sp[p] == STRONG) ? 255 : 0;
    }
    if (dst_u8) {
        uint8_t* o = dst_u8 + b * HW + p0;
        if (vec_u8 && n == PX) {
            *reinterpret_cast<uint32_t*>(o) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
        } else {
#pragma unroll
            for (int p = 0; p < PX; ++p)
                if (p < n) o[p] = (uint8_t)v[p];
        }
    }
    if (dst_f) {
        float f[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) f[p] = mul_add_rn(__fdiv_rn((float)v[p], 255.0f), mul, add);
        float* o = dst_f + (b * Cf + c_off) * HW + p0;
#pragma unroll
        for (int c = 0; c < 3; ++c, o += HW) {
            if (vec_f && n == PX) {
                *reinterpret_cast<f32x4*>(o) = f32x4{f[0], f[1], f[2], f[3]};
            } else {
#pragma unroll
                for (int p = 0; p < PX; ++p)
                    if (p < n) o[p] = f[p];
            }
        }
    }
}

// blocks = B * tiles of tile_h x tile_w over H x W, as a 1-D grid
inline bool tile_grid(int B, int H, int W, int tile_h, int tile_w, int& tiles_x, int& tiles_y, dim3& grid) {
    if (B < 1 || H < 1 || W < 1) return false;
    tiles_x = (W + tile_w - 1) / tile_w;
    tiles_y = (H + tile_h - 1) / tile_h;
    const long long blocks = (long long)B * tiles_x * tiles_y;
    if (blocks > 0x7fffffffll) return false;
    grid = dim3((unsigned)blocks);
    return true;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

static_assert(HRUN == 16 && HT % HRUN == 0 && HX0 % 16 == 0 && HX0 + HT + 4 <= HPITCH && HPITCH % 16 == 0,
              "a thread's run is four aligned words of one row, with a word to spare on either side");

int launch_canny_nms(const uint8_t* src, uint8_t* states, int B, int H, int W, int C, int lo, int hi, hipStream_t s) {
    dim3 grid;
    int tiles_x, tiles_y;
    if ((C != 1 && C != 3) || lo > hi || !tile_grid(B, H, W, NTY, NTX, tiles_x, tiles_y, grid)) return 1;
    if (C == 3) hipLaunchKernelGGL(canny_nms_kernel<3>, grid, dim3(TPB), 0, s, src, states, H, W, tiles_x, tiles_y, lo, hi);
    else hipLaunchKernelGGL(canny_nms_kernel<1>, grid, dim3(TPB), 0, s, src, states, H, W, tiles_x, tiles_y, lo, hi);
    return hipGetLastError() != hipSuccess;
}

int launch_canny_hysteresis(uint8_t* states, int B, int H, int W, int* flag, hipStream_t s) {
    dim3 grid;
    int tiles_x, tiles_y;
    if (!flag || !tile_grid(B, H, W, HT, HT, tiles_x, tiles_y, grid)) return 1;
    hipLaunchKernelGGL(canny_hysteresis_kernel, grid, dim3(TPB), 0, s, states, H, W, tiles_x, tiles_y, flag);
    return hipGetLastError() != hipSuccess;
}

int launch_canny_emit(const uint8_t* states, uint8_t* dst_u8, float* dst_f, int B, int H, int W, int Cf, int c_off, float mul, float add,
                      hipStream_t s) {
    if (B < 1 || H < 1 || W < 1 || (!dst_u8 && !dst_f)) return 1;
    if (dst_f && (c_off < 0 || c_off + 3 > Cf)) return 1;
    const long long HW = (long long)H * W;
    const long long blocks = ((long long)B * ((HW + PX - 1) / PX) + TPB - 1) / TPB;
    if (blocks > 0x7fffffffll) return 1;
    const bool v4 = HW % PX == 0;
    hipLaunchKernelGGL(canny_emit_kernel, dim3((unsigned)blocks), dim3(TPB), 0, s, states, dst_u8, dst_f, B, HW, Cf, c_off, mul, add,
                       (int)(v4 && aligned(states, 4)), (int)(v4 && aligned(dst_u8, 4)), (int)(v4 && aligned(dst_f, 16)));
    return hipGetLastError() != hipSuccess;
}
