// pdengine: the kernels of the M-LSD line detector that are no contraction (annotator/mlsd; host side in mlsd.cpp).
//   mlsd_upload_kernel    u8 RGB [B][H][W][3] -> NHWC in the compute type: x / 127.5 - 1 and the constant-one fourth plane (pred_lines :54-59)
//   mlsd_dwconv_kernel    MobileNetV2's depthwise conv3x3 + folded BatchNorm bias + ReLU6, stride 1 / 2, through an LDS patch
//   mlsd_upcat_kernel     BlockTypeA's bilinear x2 upsample (align_corners = True), written into its half of the concat buffer
//   mlsd_tpmap_kernel     channels 7..15 of block23's fp32 output as the [B][9][h][w] map the decode reads
//   mlsd_peaks_kernel     3x3 non-maximum suppression of the centre logits -> one sortable key per peak
//   mlsd_select_kernel    per image: the 200 largest keys (radix select + bitonic sort), thresholds, endpoints
//   mlsd_draw_kernel      cv2.line of every kept segment: clip to the image, then the 8-connected Bresenham walk
#include "pd_common.h"

namespace {

constexpr int TPB = 256;

// 16 bytes of an NHWC row as floats: VEC = 4 (fp32) or 8 (2-byte types)
template <int DT> struct MVec;
template <> struct MVec<DT_F32> {
    static constexpr int VEC = 4;
    typedef f32x4 raw;
    static __device__ __forceinline__ void unpack(const raw& r, float* f) { f[0] = r[0]; f[1] = r[1]; f[2] = r[2]; f[3] = r[3]; }
    static __device__ __forceinline__ raw pack(const float* f) { return f32x4{f[0], f[1], f[2], f[3]}; }
    static __device__ __forceinline__ raw zero() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
};
template <> struct MVec<DT_F16> {
    static constexpr int VEC = 8;
    typedef uint4 raw;
    static __device__ __forceinline__ void unpack(const raw& r, float* f) { unpack8<DT_F16>(r, f); }
    static __device__ __forceinline__ raw pack(const float* f) { return pack8<DT_F16>(f); }
    static __device__ __forceinline__ raw zero() { return make_uint4(0, 0, 0, 0); }
};
template <> struct MVec<DT_BF16> {
    static constexpr int VEC = 8;
    typedef uint4 raw;
    static __device__ __forceinline__ void unpack(const raw& r, float* f) { unpack8<DT_BF16>(r, f); }
    static __device__ __forceinline__ raw pack(const float* f) { return pack8<DT_BF16>(f); }
    static __device__ __forceinline__ raw zero() { return make_uint4(0, 0, 0, 0); }
};

// (float32 array / 127.5) - 1.0 as NumPy evaluates it: one correctly rounded division, one subtraction
__device__ __forceinline__ float mlsd_norm(float v) {
#pragma clang fp contract(off)
    const float q = __fdiv_rn(v, 127.5f);
    return q - 1.0f;
}

__global__ __launch_bounds__(TPB) void mlsd_upload_kernel(const uint8_t* __restrict__ in, void* __restrict__ out, int out_dt, long long npix) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= npix) return;
    const uint8_t* s = in + i * 3;
    const float v0 = mlsd_norm((float)s[0]), v1 = mlsd_norm((float)s[1]), v2 = mlsd_norm((float)s[2]), v3 = mlsd_norm(1.0f);
    if (out_dt == DT_F32) {
        float* o = reinterpret_cast<float*>(out) + i * 8;
        *reinterpret_cast<f32x4*>(o) = f32x4{v0, v1, v2, v3};
        *reinterpret_cast<f32x4*>(o + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
        uint4 u;
        u.x = out_dt == DT_F16 ? pack2h(v0, v1) : pack2bf(v0, v1);
        u.y = out_dt == DT_F16 ? pack2h(v2, v3) : pack2bf(v2, v3);
        u.z = 0u; u.w = 0u;
        reinterpret_cast<uint4*>(out)[i] = u;
    }
}

// Depthwise conv3x3.  A block owns TY x TX output pixels of one sample and one chunk of LANES 16-byte channel vectors (128 bytes of every
// pixel's row).  It stages the input patch those outputs read -- ((TY - 1) S + 3) x ((TX - 1) S + 3) pixels, zero outside the image --
// into LDS with one global read per element, the ReLU6 of the producing layer applied on the way (the producer stored max(x, 0); min
// with 6 of a stored value is exact).  Thread (pixel slot, lane) then keeps its lane's 9 x VEC weights and VEC biases in registers and
// walks its outputs: nine LDS vectors, 9 x VEC fp32 FMAs in tap order, + bias, clamp to [0, 6], one rounding, one 16-byte store.
constexpr int DW_LANES = 8, DW_TX = 16;
template <int DT, int S>
__global__ __launch_bounds__(TPB) void mlsd_dwconv_kernel(const void* __restrict__ x, void* __restrict__ y, const float* __restrict__ w,
                                                          const float* __restrict__ bias, int H, int W, int C, int Ho, int Wo, int tiles_x,
                                                          int tiles_y, int nchunk, int in_relu6) {
    typedef MVec<DT> V;
    typedef typename V::raw raw;
    constexpr int VEC = V::VEC, CC = DW_LANES * VEC;
    constexpr int TX = DW_TX, TY = S == 1 ? 8 : 4;
    constexpr int PW = (TX - 1) * S + 3, PH = (TY - 1) * S + 3, PAD = S == 1 ? 1 : 0;
    __shared__ raw s_x[PH * PW][DW_LANES];
    __shared__ float s_w[9][CC];
    __shared__ float s_b[CC];
    const int tid = threadIdx.x;
    int bid = blockIdx.x;
    const int chunk = bid % nchunk; bid /= nchunk;
    const int tx0 = (bid % tiles_x) * TX; bid /= tiles_x;
    const int ty0 = (bid % tiles_y) * TY;
    const long long b = bid / tiles_y;
    const int nv = C / VEC;                                   // 16-byte vectors per pixel
    const int lanes = min(DW_LANES, nv - chunk * DW_LANES);   // of this chunk
    const raw* xin = reinterpret_cast<const raw*>(x) + b * H * W * nv + chunk * DW_LANES;
    for (int i = tid; i < PH * PW * DW_LANES; i += TPB) {
        const int lane = i % DW_LANES, pix = i / DW_LANES;
        const int py = pix / PW, px = pix - py * PW;
        const int iy = ty0 * S - PAD + py, ix = tx0 * S - PAD + px;
        raw r = V::zero();
        if (lane < lanes && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
            r = xin[((long long)iy * W + ix) * nv + lane];
            if (in_relu6) {
                float f[VEC];
                V::unpack(r, f);
#pragma unroll
                for (int k = 0; k < VEC; ++k) f[k] = fminf(fmaxf(f[k], 0.f), 6.f);
                r = V::pack(f);
            }
        }
        s_x[pix][lane] = r;
    }
    for (int i = tid; i < 10 * CC; i += TPB) {
        const int t = i / CC, c = i - t * CC;
        const int gc = chunk * CC + c;
        if (t < 9) s_w[t][c] = gc < C ? w[(long long)gc * 9 + t] : 0.f;
        else s_b[c] = gc < C ? bias[gc] : 0.f;
    }
    __syncthreads();
    const int lane = tid % DW_LANES, slot = tid / DW_LANES;
    if (lane >= lanes) return;
    float wr[9][VEC], br[VEC];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int k = 0; k < VEC; ++k) wr[t][k] = s_w[t][lane * VEC + k];
#pragma unroll
    for (int k = 0; k < VEC; ++k) br[k] = s_b[lane * VEC + k];
    raw* yout = reinterpret_cast<raw*>(y) + b * Ho * Wo * nv + chunk * DW_LANES + lane;
    for (int o = slot; o < TX * TY; o += TPB / DW_LANES) {
        const int oy = o / TX, ox = o - oy * TX;
        const int gy = ty0 + oy, gx = tx0 + ox;
        if (gy >= Ho || gx >= Wo) continue;
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            float f[VEC];
            V::unpack(s_x[(oy * S + t / 3) * PW + ox * S + t % 3][lane], f);
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = fmaf(f[k], wr[t][k], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = fminf(fmaxf(acc[k] + br[k], 0.f), 6.f);
        yout[((long long)gy * Wo + gx) * nv] = V::pack(acc);
    }
}

// upsample_bilinear2d with align_corners = True along one axis: output d reads source position d (n - 1) / (2n - 1).  PyTorch forms
// that product in float (area_pixel_compute_scale, then scale * d), which leaves the weight lambda with an absolute error that grows
// with d -- 4.4 x 2^-24 max|x| in the result at n = 8 and 84 x at n = 128, measured against fp64.  Here the
// position is the exact rational: integer quotient and remainder, one correctly rounded division for lambda.  Index and weight agree
// with PyTorch's to its own rounding error; the result is within 3 roundings of the exact interpolation at every size.
__device__ __forceinline__ void upcat_axis(int d, int n, int& i0, int& i1, float& l0, float& l1) {
    const int den = 2 * n - 1, num = d * (n - 1);
    i0 = num / den;
    i1 = min(i0 + 1, n - 1);
    l1 = __fdiv_rn((float)(num - i0 * den), (float)den);
    l0 = 1.0f - l1;
}

// one thread per (output pixel, 16-byte channel vector); the four source vectors come from L2 (the source is a quarter of the output)
template <int DT>
__global__ __launch_bounds__(TPB) void mlsd_upcat_kernel(const void* __restrict__ x, int ldx, void* __restrict__ y, int ldy, int B, int h, int w,
                                                         int C) {
#pragma clang fp contract(off)
    typedef MVec<DT> V;
    typedef typename V::raw raw;
    constexpr int VEC = V::VEC;
    const int nv = C / VEC;
    const long long total = (long long)B * 2 * h * 2 * w * nv;
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const int v = (int)(i % nv);
    long long pix = i / nv;
    const int ox = (int)(pix % (2 * w)); pix /= 2 * w;
    const int oy = (int)(pix % (2 * h));
    const long long b = pix / (2 * h);
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    upcat_axis(oy, h, y0, y1, ly0, ly1);
    upcat_axis(ox, w, x0, x1, lx0, lx1);
    const raw* src = reinterpret_cast<const raw*>(x);
    const int lv = ldx / VEC;
    const long long base = b * h * w;
    float a[VEC], bq[VEC], c[VEC], d[VEC], o[VEC];
    V::unpack(src[(base + (long long)y0 * w + x0) * lv + v], a);
    V::unpack(src[(base + (long long)y0 * w + x1) * lv + v], bq);
    V::unpack(src[(base + (long long)y1 * w + x0) * lv + v], c);
    V::unpack(src[(base + (long long)y1 * w + x1) * lv + v], d);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float t0 = lx0 * a[k] + lx1 * bq[k];
        const float t1 = lx0 * c[k] + lx1 * d[k];
        o[k] = ly0 * t0 + ly1 * t1;
    }
    reinterpret_cast<raw*>(y)[(((b * 2 * h + oy) * 2 * w) + ox) * (ldy / VEC) + v] = V::pack(o);
}

__global__ __launch_bounds__(TPB) void mlsd_tpmap_kernel(const float* __restrict__ x, float* __restrict__ tp, int B, long long hw) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long long)B * hw) return;
    const long long b = i / hw, p = i - b * hw;
    const float* s = x + i * 16 + 7;
#pragma unroll
    for (int c = 0; c < 9; ++c) tp[(b * 9 + c) * hw + p] = s[c];
}

// a float as an unsigned integer of the same order
__device__ __forceinline__ uint32_t ord_f32(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Non-maximum suppression on the logits (the sigmoid is monotone): a pixel is a peak when no pixel of its 3x3 window (pixels outside the
// map count as -inf) exceeds it.  Every peak appends the key (order of the logit << 32) | ~index to its image's list: keys are unique,
// larger logits first, equal logits by ascending index, whatever order the appends land in.
__global__ __launch_bounds__(TPB) void mlsd_peaks_kernel(const float* __restrict__ tp, unsigned long long* __restrict__ cand,
                                                         int* __restrict__ ncand, int B, int h, int w) {
    const long long hw = (long long)h * w;
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long long)B * hw) return;
    const long long b = i / hw;
    const int p = (int)(i - b * hw);
    const int yy = p / w, xx = p - yy * w;
    const float* c = tp + b * 9 * hw;
    const float v = c[p];
    bool peak = v == v;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int ny = yy + dy, nx = xx + dx;
            if ((unsigned)ny < (unsigned)h && (unsigned)nx < (unsigned)w && c[(long long)ny * w + nx] > v) peak = false;
        }
    if (!peak) return;
    const int slot = atomicAdd(ncand + b, 1);   // at most h * w peaks per image: the list holds them all
    cand[b * hw + slot] = ((unsigned long long)ord_f32(v) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)p);
}

// One block per image.  The MLSD_TOPK-th largest key is found by a radix select over the 8 key bytes (one histogram pass each); the keys
// at or above it are gathered into LDS and sorted in descending order (bitonic, 256 slots).  Entry i then evaluates pred_lines' filter
// and endpoints:  score = sigmoid(logit) > thr_v,  dist = sqrt((dx0 - dx1)^2 + (dy0 - dy1)^2) > thr_d in fp32, every operation rounded on
// its own;  endpoint = int(2 * (x + disp)) with x + disp in fp64 (int64 + float32 in NumPy), truncated towards zero.
constexpr int SEL_TPB = 1024, SEL_N = 256;
static_assert(MLSD_TOPK <= SEL_N, "the sort holds the selection");
__global__ __launch_bounds__(SEL_TPB) void mlsd_select_kernel(const float* __restrict__ tp, const unsigned long long* __restrict__ cand,
                                                              const int* __restrict__ ncand, int* __restrict__ segs, int* __restrict__ count,
                                                              int h, int w, float thr_v, float thr_d) {
#pragma clang fp contract(off)
    __shared__ unsigned long long s_key[SEL_N];
    __shared__ int s_hist[256];
    __shared__ unsigned long long s_prefix;
    __shared__ int s_k, s_n;
    __shared__ int s_flag[SEL_N];
    const int tid = threadIdx.x;
    const long long b = blockIdx.x;
    const long long hw = (long long)h * w;
    const unsigned long long* keys = cand + b * hw;
    const int n = ncand[b];
    if (tid < SEL_N) s_key[tid] = 0ull;
    if (tid == 0) { s_prefix = 0ull; s_k = MLSD_TOPK; s_n = 0; }
    __syncthreads();
    if (n <= MLSD_TOPK) {
        if (tid < n) s_key[tid] = keys[tid];
    } else {
        for (int pass = 7; pass >= 0; --pass) {
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            const unsigned long long prefix = s_prefix;
            const unsigned long long himask = pass == 7 ? 0ull : (~0ull << (8 * (pass + 1)));
            for (int i = tid; i < n; i += SEL_TPB) {
                const unsigned long long k = keys[i];
                if ((k & himask) == prefix) atomicAdd(&s_hist[(int)((k >> (8 * pass)) & 0xffull)], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int k = s_k, d = 255;
                for (; d > 0; --d) {
                    if (s_hist[d] >= k) break;
                    k -= s_hist[d];
                }
                s_k = k;
                s_prefix = prefix | ((unsigned long long)d << (8 * pass));
            }
            __syncthreads();
        }
        const unsigned long long kth = s_prefix;   // keys are unique: exactly MLSD_TOPK of them are >= the MLSD_TOPK-th largest
        for (int i = tid; i < n; i += SEL_TPB) {
            const unsigned long long k = keys[i];
            if (k >= kth) {
                const int slot = atomicAdd(&s_n, 1);
                if (slot < SEL_N) s_key[slot] = k;
            }
        }
    }
    __syncthreads();
    // bitonic sort, descending (the zero pads sink to the end: every real key is non-zero)
    for (int k = 2; k <= SEL_N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (tid < SEL_N) {
                const int ixj = tid ^ j;
                if (ixj > tid) {
                    const unsigned long long a = s_key[tid], c = s_key[ixj];
                    const bool desc = (tid & k) == 0;
                    if (desc ? a < c : a > c) { s_key[tid] = c; s_key[ixj] = a; }
                }
            }
            __syncthreads();
        }
    const int nsel = min(n, MLSD_TOPK);
    int sx = 0, sy = 0, ex = 0, ey = 0, keep = 0;
    if (tid < nsel) {
        const int p = (int)(0xffffffffu - (uint32_t)(s_key[tid] & 0xffffffffull));
        const int yy = p / w, xx = p - yy * w;
        const float* c = tp + b * 9 * hw;
        const float logit = c[p];
        const float d0 = c[hw + p], d1 = c[2 * hw + p], d2 = c[3 * hw + p], d3 = c[4 * hw + p];
        const float score = __fdiv_rn(1.0f, 1.0f + expf(-logit));
        const float dx = d0 - d2, dy = d1 - d3;
        const float dist = __fsqrt_rn(dx * dx + dy * dy);
        keep = (score > thr_v && dist > thr_d) ? 1 : 0;
        auto end = [](int base, float disp) {
            double v = 2.0 * ((double)base + (double)disp);
            v = v < -1.0e9 ? -1.0e9 : (v > 1.0e9 ? 1.0e9 : v);   // (keeps the cast defined; no image is that large)
            return (int)v;
        };
        sx = end(xx, d0); sy = end(yy, d1); ex = end(xx, d2); ey = end(yy, d3);
    }
    if (tid < SEL_N) s_flag[tid] = keep;
    __syncthreads();
    if (tid < SEL_N) {
        int pos = 0, total = 0;
        for (int j = 0; j < SEL_N; ++j) {
            pos += j < tid ? s_flag[j] : 0;
            total += s_flag[j];
        }
        if (keep) {
            int* o = segs + (b * MLSD_TOPK + pos) * 4;
            o[0] = sx; o[1] = sy; o[2] = ex; o[3] = ey;
        }
        if (tid == 0) count[b] = total;
    }
}

// cv2.clipLine on 64-bit coordinates: false when nothing of the segment lies inside [0, W) x [0, H)
__device__ __forceinline__ bool clip_line(long long W, long long H, long long& x1, long long& y1, long long& x2, long long& y2) {
    const long long right = W - 1, bottom = H - 1;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        long long a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (long long)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (long long)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (long long)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (long long)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

// one thread per segment: the walk of cv2's LineIterator (connectivity 8, left to right) over the clipped end points.  Segments
// overlap, but every store writes the same byte, so the order of the stores does not matter
__global__ __launch_bounds__(TPB) void mlsd_draw_kernel(const int* __restrict__ segs, const int* __restrict__ count, int max_segs,
                                                        uint8_t* __restrict__ map, int H, int W) {
    const int s = blockIdx.x * TPB + threadIdx.x;
    const long long b = blockIdx.y;
    if (s >= max_segs || s >= count[b]) return;
    const int* q = segs + (b * max_segs + s) * 4;
    long long x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3];
    if (x1 < 0 || x1 >= W || x2 < 0 || x2 >= W || y1 < 0 || y1 >= H || y2 < 0 || y2 >= H) {
        if (!clip_line(W, H, x1, y1, x2, y2)) return;
        // (clipLine leaves both ends inside the image when it accepts; the walk below never leaves the box they span)
        if (x1 < 0 || x1 >= W || x2 < 0 || x2 >= W || y1 < 0 || y1 >= H || y2 < 0 || y2 >= H) return;
    }
    int dx = (int)(x2 - x1), dy = (int)(y2 - y1);
    int px = (int)x1, py = (int)y1, step_x = 1, step_y = 1;
    if (dx < 0) { dx = -dx; dy = -dy; px = (int)x2; py = (int)y2; }   // left to right
    if (dy < 0) { dy = -dy; step_y = -1; }
    const bool vert = dy > dx;
    if (vert) { const int t = dx; dx = dy; dy = t; }
    int err = dx - (dy + dy);
    const int plus = dx + dx, minus = -(dy + dy);
    uint8_t* img = map + b * H * W;
    for (int i = 0; i <= dx; ++i) {
        if ((unsigned)px < (unsigned)W && (unsigned)py < (unsigned)H) img[(long long)py * W + px] = (uint8_t)CANNY_STRONG;
        const bool m = err < 0;
        err += minus + (m ? plus : 0);
        if (vert) { py += step_y; px += m ? step_x : 0; }
        else { px += step_x; py += m ? step_y : 0; }
    }
}

}  // namespace

int launch_mlsd_upload(const uint8_t* in, void* out, int out_dt, int B, int H, int W, hipStream_t s) {
    if (B < 1 || H < 1 || W < 1) return 1;
    const long long npix = (long long)B * H * W, blocks = (npix + TPB - 1) / TPB;
    if (blocks > 0x7fffffffll) return 1;
    hipLaunchKernelGGL(mlsd_upload_kernel, dim3((unsigned)blocks), dim3(TPB), 0, s, in, out, out_dt, npix);
    return hipGetLastError() != hipSuccess;
}

namespace {
template <int DT>
int launch_dw(const void* x, void* y, const float* w, const float* bias, int B, int H, int W, int C, int stride, int in_relu6, hipStream_t s) {
    constexpr int VEC = MVec<DT>::VEC;
    const int Ho = stride == 1 ? H : H / 2, Wo = stride == 1 ? W : W / 2;
    const int TY = stride == 1 ? 8 : 4;
    const int tiles_x = (Wo + DW_TX - 1) / DW_TX, tiles_y = (Ho + TY - 1) / TY, nchunk = (C / VEC + DW_LANES - 1) / DW_LANES;
    const long long blocks = (long long)B * tiles_x * tiles_y * nchunk;
    if (blocks > 0x7fffffffll) return 1;
    if (stride == 1)
        hipLaunchKernelGGL((mlsd_dwconv_kernel<DT, 1>), dim3((unsigned)blocks), dim3(TPB), 0, s, x, y, w, bias, H, W, C, Ho, Wo, tiles_x, tiles_y,
                           nchunk, in_relu6);
    else
        hipLaunchKernelGGL((mlsd_dwconv_kernel<DT, 2>), dim3((unsigned)blocks), dim3(TPB), 0, s, x, y, w, bias, H, W, C, Ho, Wo, tiles_x, tiles_y,
                           nchunk, in_relu6);
    return hipGetLastError() != hipSuccess;
}
}  // namespace

int launch_mlsd_dwconv(const void* x, void* y, int dt, const float* w, const float* bias, int B, int H, int W, int C, int stride, int in_relu6,
                       hipStream_t s) {
    const int vec = dt == DT_F32 ? 4 : 8;
    if (B < 1 || H < 1 || W < 1 || C < vec || C % vec || (stride != 1 && stride != 2)) return 1;
    if (stride == 2 && ((H | W) & 1)) return 1;
    if (dt == DT_F32) return launch_dw<DT_F32>(x, y, w, bias, B, H, W, C, stride, in_relu6, s);
    if (dt == DT_F16) return launch_dw<DT_F16>(x, y, w, bias, B, H, W, C, stride, in_relu6, s);
    if (dt == DT_BF16) return launch_dw<DT_BF16>(x, y, w, bias, B, H, W, C, stride, in_relu6, s);
    return 1;
}

int launch_mlsd_upcat(const void* x, int ldx, void* y, int ldy, int dt, int B, int h, int w, int C, hipStream_t s) {
    const int vec = dt == DT_F32 ? 4 : 8;
    if (B < 1 || h < 1 || w < 1 || C < vec || C % vec || ldx % vec || ldy % vec || ldx < C || ldy < C) return 1;
    const long long blocks = ((long long)B * 4 * h * w * (C / vec) + TPB - 1) / TPB;
    if (blocks > 0x7fffffffll) return 1;
    const dim3 grid((unsigned)blocks), blk(TPB);
    if (dt == DT_F32) hipLaunchKernelGGL(mlsd_upcat_kernel<DT_F32>, grid, blk, 0, s, x, ldx, y, ldy, B, h, w, C);
    else if (dt == DT_F16) hipLaunchKernelGGL(mlsd_upcat_kernel<DT_F16>, grid, blk, 0, s, x, ldx, y, ldy, B, h, w, C);
    else if (dt == DT_BF16) hipLaunchKernelGGL(mlsd_upcat_kernel<DT_BF16>, grid, blk, 0, s, x, ldx, y, ldy, B, h, w, C);
    else return 1;
    return hipGetLastError() != hipSuccess;
}

int launch_mlsd_tpmap(const float* x, float* tp, int B, int h, int w, hipStream_t s) {
    if (B < 1 || h < 1 || w < 1) return 1;
    const long long hw = (long long)h * w, blocks = (B * hw + TPB - 1) / TPB;
    if (blocks > 0x7fffffffll) return 1;
    hipLaunchKernelGGL(mlsd_tpmap_kernel, dim3((unsigned)blocks), dim3(TPB), 0, s, x, tp, B, hw);
    return hipGetLastError() != hipSuccess;
}

int launch_mlsd_decode(const float* tp, unsigned long long* cand, int* ncand, int* segs, int* count, int B, int h, int w, float thr_v,
                       float thr_d, hipStream_t s) {
    if (B < 1 || h < 1 || w < 1 || (long long)h * w >= 0x7fffffffll) return 1;
    const long long blocks = ((long long)B * h * w + TPB - 1) / TPB;
    if (blocks > 0x7fffffffll) return 1;
    if (hipMemsetAsync(ncand, 0, (size_t)B * sizeof(int), s) != hipSuccess) return 1;
    hipLaunchKernelGGL(mlsd_peaks_kernel, dim3((unsigned)blocks), dim3(TPB), 0, s, tp, cand, ncand, B, h, w);
    if (hipGetLastError() != hipSuccess) return 1;
    hipLaunchKernelGGL(mlsd_select_kernel, dim3((unsigned)B), dim3(SEL_TPB), 0, s, tp, cand, ncand, segs, count, h, w, thr_v, thr_d);
    return hipGetLastError() != hipSuccess;
}

int launch_mlsd_draw(const int* segs, const int* count, int max_segs, uint8_t* map, int B, int H, int W, hipStream_t s) {
    if (B < 1 || H < 1 || W < 1 || max_segs < 1 || B > 65535) return 1;
    if (hipMemsetAsync(map, 0, (size_t)B * H * W, s) != hipSuccess) return 1;
    hipLaunchKernelGGL(mlsd_draw_kernel, dim3((unsigned)((max_segs + TPB - 1) / TPB), (unsigned)B), dim3(TPB), 0, s, segs, count, max_segs, map, H, W);
    return hipGetLastError() != hipSuccess;
}
