// IP-Adapter's decoupled cross-attention term (gfx950): att[b, i, :] = round_T(att[b, i, :] + s * o_ip[b, i, :]) in place, with
//   o_ip = softmax(q K_ip^T scale) V_ip per head over the T <= 64 image keys of the sample.
// One pass and memory-bound: every q and att element is read once, att is written once, 16 bytes per access; the sample's K_ip / V_ip
// sit in LDS; logits, softmax and o_ip never leave registers.
//
// Work split.  A head's dh channels of one query row belong to a group of G = dh / 8 neighbouring lanes, 8 channels (one 16-byte
// access in the 2-byte types, two in fp32) per lane; a wave holds GPW = 64 / G whole groups (dh 40 / 80 / 160: 60 of 64 lanes work).
// Each lane forms the partial dot product of its 8 channels against a key, the group sums the G partials with shuffles -- an XOR
// butterfly over the power-of-two factor of G, then the five partials of the odd factor gathered in one fixed order, so every lane
// of the group holds the same bits -- and from then on every lane runs the row's softmax redundantly and accumulates its own 8
// channels of o_ip.  Plain VALU: with T = 4 keys an MFMA tile would be three quarters padding on the key side and the kernel has
// under 3 FLOP per byte, far below where the matrix pipe matters; the operands are used as stored (fp32 in the fp32-storage modes).
//
// Arithmetic, all fp32: logit = dot * (scale * log2 e); keys go in tiles of 32 whose logits stay in registers, so the running
// maximum is raised (and o, l rescaled) at most once per 32 keys; p = exp2(logit - m); o += p v; at the end o / l, * s, + att, and one
// rounding to the storage type at the store.
//
// A block of 256 threads takes `rb` query rows x `hb` heads of one sample (grid: row chunks, head chunks, samples).  hb is the largest
// divisor of the head count whose keys and values fit 48 KiB of LDS; where a single head's do not (dh 160 in fp32 beyond 38 keys)
// the keys pass through LDS in chunks of 32.
#include "pd_common.h"

namespace {
constexpr int kThreads = 256, kWaves = kThreads / 64, kTile = 32, kLdsBudget = 48 * 1024;

template <int DT> struct Elem { typedef uint16_t type; };
template <> struct Elem<DT_F32> { typedef float type; };

template <int DT> __device__ __forceinline__ void load8(const void* p, float* f) {
    if constexpr (DT == DT_F32) {
        const f32x4 a = reinterpret_cast<const f32x4*>(p)[0], b = reinterpret_cast<const f32x4*>(p)[1];
        f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
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

// the sum of v over the G lanes of the group that starts at lane `base`; the same bits in every lane of the group
template <int G> __device__ __forceinline__ float group_sum(float v, int base, int lig) {
    constexpr int P2 = G & -G, ODD = G / P2;
#pragma unroll
    for (int m = 1; m < P2; m <<= 1) v += __shfl_xor(v, m, 64);
    if constexpr (ODD > 1) {
        const int first = base + (lig & (P2 - 1));
        float s = __shfl(v, first, 64);
#pragma unroll
        for (int j = 1; j < ODD; ++j) s += __shfl(v, first + j * P2, 64);
        v = s;
    }
    return v;
}

struct IpAttnArgs {
    const void* q;
    void* att;
    const void* K;
    const void* V;
    long long kv_bs;   // elements between two samples' keys (0: one set for every sample)
    int N, C, T, hb, rb, tc;
    float sl2, s;      // scale * log2(e); the adapter scale
};

template <int DT, int G>
__global__ __launch_bounds__(kThreads) void ip_attn_add_kernel(const IpAttnArgs a) {
    typedef typename Elem<DT>::type E;
    constexpr int DH = 8 * G, GPW = 64 / G, EPC = 16 / (int)sizeof(E);   // EPC: elements per 16-byte piece
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = lane / G, lig = lane - grp * G, base = grp * G;
    const int b = blockIdx.z, hc = blockIdx.y, row0 = blockIdx.x * a.rb;
    const int Wd = a.hb * DH;                        // channels this block serves
    E* ldsK = reinterpret_cast<E*>(lds_raw);
    E* ldsV = ldsK + (size_t)a.tc * Wd;
    const E* Kg = reinterpret_cast<const E*>(a.K) + (size_t)b * a.kv_bs + (size_t)hc * Wd;
    const E* Vg = reinterpret_cast<const E*>(a.V) + (size_t)b * a.kv_bs + (size_t)hc * Wd;
    const int nchunk = (a.T + a.tc - 1) / a.tc;
    const int ppr = Wd / EPC;                        // 16-byte pieces per key row
    auto stage = [&](int t0, int nt) {
        for (int i = tid; i < nt * ppr; i += kThreads) {
            const int t = i / ppr, c = (i - t * ppr) * EPC;
            *reinterpret_cast<uint4*>(ldsK + (size_t)t * Wd + c) = *reinterpret_cast<const uint4*>(Kg + (size_t)(t0 + t) * a.C + c);
            *reinterpret_cast<uint4*>(ldsV + (size_t)t * Wd + c) = *reinterpret_cast<const uint4*>(Vg + (size_t)(t0 + t) * a.C + c);
        }
    };
    if (nchunk == 1) {
        stage(0, a.T);
        __syncthreads();
    }
    const int items = a.rb * a.hb;                   // (row, head) pairs of this block, heads fastest
    const int passes = (items + kWaves * GPW - 1) / (kWaves * GPW);   // the same in every wave: the barriers below are block-uniform
    for (int ps = 0; ps < passes; ++ps) {
        const int it = (ps * kWaves + wave) * GPW + grp;
        const int rl = it / a.hb, hl = it - rl * a.hb, row = row0 + rl;
        const bool valid = grp < GPW && it < items && row < a.N;
        const size_t off = ((size_t)b * a.N + row) * a.C + (size_t)(hc * a.hb + hl) * DH + lig * 8;
        float q[8], x[8], o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { q[j] = 0.f; x[j] = 0.f; o[j] = 0.f; }
        if (valid) {
            load8<DT>(reinterpret_cast<const E*>(a.q) + off, q);
            load8<DT>(reinterpret_cast<const E*>(a.att) + off, x);
        }
        const int col = (valid ? hl : 0) * DH + lig * 8;
        float m = -INFINITY, l = 0.f;
        for (int ch = 0; ch < nchunk; ++ch) {
            const int t0 = ch * a.tc, nt = min(a.tc, a.T - t0);
            if (nchunk > 1) {
                __syncthreads();
                stage(t0, nt);
                __syncthreads();
            }
            for (int t1 = 0; t1 < nt; t1 += kTile) {
                float sl[kTile];
                float tmax = -INFINITY;
#pragma unroll
                for (int t = 0; t < kTile; ++t) {
                    sl[t] = -INFINITY;
                    if (t1 + t < nt) {
                        float k[8];
                        load8<DT>(ldsK + (size_t)(t1 + t) * Wd + col, k);
                        float d = q[0] * k[0];
#pragma unroll
                        for (int j = 1; j < 8; ++j) d = fmaf(q[j], k[j], d);
                        sl[t] = group_sum<G>(d, base, lig) * a.sl2;
                        tmax = fmaxf(tmax, sl[t]);
                    }
                }
                const float mn = fmaxf(m, tmax);
                const float alpha = __builtin_amdgcn_exp2f(m - mn);   // 0 on the first tile (m = -inf), 1 where the maximum stays
                l *= alpha;
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] *= alpha;
                m = mn;
#pragma unroll
                for (int t = 0; t < kTile; ++t) {
                    if (t1 + t < nt) {
                        const float p = __builtin_amdgcn_exp2f(sl[t] - m);
                        float v[8];
                        load8<DT>(ldsV + (size_t)(t1 + t) * Wd + col, v);
                        l += p;
#pragma unroll
                        for (int j = 0; j < 8; ++j) o[j] = fmaf(p, v[j], o[j]);
                    }
                }
            }
        }
        if (valid) {
            const float rl_ = 1.0f / l;
            float y[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) y[j] = x[j] + a.s * (o[j] * rl_);
            store8<DT>(reinterpret_cast<E*>(a.att) + off, y);
        }
    }
}

template <int DT>
int launch_dt(const IpAttnArgs& a, int G, dim3 grid, size_t lds, hipStream_t s) {
    switch (G) {
        case 1: hipLaunchKernelGGL((ip_attn_add_kernel<DT, 1>), grid, dim3(kThreads), lds, s, a); break;
        case 2: hipLaunchKernelGGL((ip_attn_add_kernel<DT, 2>), grid, dim3(kThreads), lds, s, a); break;
        case 4: hipLaunchKernelGGL((ip_attn_add_kernel<DT, 4>), grid, dim3(kThreads), lds, s, a); break;
        case 5: hipLaunchKernelGGL((ip_attn_add_kernel<DT, 5>), grid, dim3(kThreads), lds, s, a); break;
        case 10: hipLaunchKernelGGL((ip_attn_add_kernel<DT, 10>), grid, dim3(kThreads), lds, s, a); break;
        case 20: hipLaunchKernelGGL((ip_attn_add_kernel<DT, 20>), grid, dim3(kThreads), lds, s, a); break;
        default: return 2;
    }
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
}  // namespace

// 0 launched, 1 launch failure, 2 a shape the kernel does not take (head dim, T, C)
int launch_ip_attention_add(const void* q2, void* att, const void* K_ip, const void* V_ip, long long kv_sample_stride, int B, int N, int C, int heads,
                            int T, float scale, float s, int dt, hipStream_t stream) {
    if (B < 1 || N < 1 || heads < 1 || C < 8 || C % 8 || C % heads || T < 1 || T > 64 || B > 65535) return 2;
    const int dh = C / heads;
    if (dh != 8 && dh != 16 && dh != 32 && dh != 40 && dh != 80 && dh != 160) return 2;
    const int G = dh / 8, gpw = 64 / G;
    const size_t eb = dt_size(dt);
    int hb = heads, tc = T;
    while (hb > 1 && (heads % hb || (size_t)T * hb * dh * 2 * eb > (size_t)kLdsBudget)) --hb;
    if ((size_t)T * hb * dh * 2 * eb > (size_t)kLdsBudget) tc = kTile;   // hb is 1 here: the keys pass through LDS 32 at a time
    if (heads / hb > 65535) return 2;
    // rows per block: four passes of the block's groups, fewer while the grid would stay below ~4 blocks per compute unit
    const int per_pass = kWaves * gpw;
    int rb = (4 * per_pass + hb - 1) / hb;
    const int rb_min = (per_pass + hb - 1) / hb;
    while (rb > rb_min && (long long)((N + rb - 1) / rb) * (heads / hb) * B < 1024) rb = (rb + 1) / 2;
    if (rb < rb_min) rb = rb_min;
    IpAttnArgs a;
    a.q = q2; a.att = att; a.K = K_ip; a.V = V_ip; a.kv_bs = kv_sample_stride;
    a.N = N; a.C = C; a.T = T; a.hb = hb; a.rb = rb; a.tc = tc;
    a.sl2 = scale * 1.4426950408889634f; a.s = s;
    const dim3 grid((unsigned)((N + rb - 1) / rb), (unsigned)(heads / hb), (unsigned)B);
    const size_t lds = (size_t)tc * hb * dh * 2 * eb;
    if (dt == DT_F32) return launch_dt<DT_F32>(a, G, grid, lds, stream);
    if (dt == DT_F16) return launch_dt<DT_F16>(a, G, grid, lds, stream);
    if (dt == DT_BF16) return launch_dt<DT_BF16>(a, G, grid, lds, stream);
    return 2;
}
