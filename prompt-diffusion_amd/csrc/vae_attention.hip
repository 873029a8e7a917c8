// Single-head flash attention for the first stage's mid block (AttnBlock, ldm/modules/diffusionmodules/model.py:144-202):
// softmax(Q K^T * C^-0.5) V with ONE head over all C channels (C = 128 or 512), without the [N, N] score matrix.  2-byte
// modes only; fp32 logits and fp32 online softmax like attention.hip.
//
// attn_kernel cannot take a head of 512: it keeps a wave's whole Q row and O^T accumulator in registers.  Here the head
// dimension is split over the block's four waves instead.  A block owns QB queries of one sample (64 at C = 128, 48 at C = 512: what
// the register file takes without spilling); wave w owns the d-slice
// [w C/4, (w+1) C/4) of BOTH products:
//   S^T partial [32 keys][QB queries] = K[:, slice] . Q[:, slice]^T   (A = K rows from LDS, B = the wave's Q slice in registers)
//   the four fp32 partials meet in LDS; after one barrier every wave sums them in the same order (w = 0..3), so all four hold
//   bit-identical logits and run the same online-softmax update: the same max, sum and P^T in every wave
//   O^T[slice][QB queries] += V^T[slice rows] . P^T                    (A = the wave's V^T rows from LDS, B = P^T from S^T's registers)
// Fragment mapping, key order of the V^T tile (vt_slot) and the K row stride rule are attention.hip's.
// Per 32-key tile: the next tile's K and V^T chunks are requested into registers first; K lands in LDS behind the first barrier
// (everybody is done with QK^T), V^T behind the second (everybody is done with PV), so a tile costs two barriers and no wait on HBM.
#include "pd_common.h"
#include "pd_mma.h"
#include "attn_vt.h"

namespace {

constexpr int VA_TK = 32;          // keys per tile (one K = 32 PV step)

template <int C>
struct VaCfg {
    static constexpr int QT = C > 128 ? 3 : 4;     // 16-query MFMA tiles per block: what the register file takes without spilling
    static constexpr int QB = QT * 16;             // queries per block
    static constexpr int DS = C / 4;               // channels per wave
    static constexpr int KS = DS / 32;             // 32-channel k-steps of the wave's QK^T slice
    static constexpr int NTD = DS / 16;            // 16-row d tiles of the wave's O^T slice
    static constexpr int NCH = C / 8;              // 16-byte chunks per K row
    static constexpr int KROW = C * 2 + 16;        // K tile row stride: an odd multiple of 16 bytes (conflict-free b128 fragment reads)
    static constexpr int VROW = VA_TK * 2;         // V^T tile rows: 32 permuted keys = 4 chunks; a fragment read covers 16 whole rows
    static constexpr int K_BYTES = VA_TK * KROW;
    static constexpr int V_BYTES = C * VROW;
    static constexpr int P_BYTES = 4 * (VA_TK / 16) * QT * 64 * 16;   // [wave][key tile][query tile][lane] f32x4
    static constexpr int SMEM = K_BYTES + V_BYTES + P_BYTES;
    static constexpr int K_IT = VA_TK * NCH / 256, V_IT = C * 4 / 256;   // staged chunks per thread
    static_assert(DS % 32 == 0 && (VA_TK * NCH) % 256 == 0 && (C * 4) % 256 == 0, "C must be a multiple of 128");
};

template <int P, int C>
__global__ __launch_bounds__(256) void vae_attn_kernel(VaeAttnParams p) {
    using Cfg = VaCfg<C>;
    constexpr int DS = Cfg::DS, KS = Cfg::KS, NTD = Cfg::NTD, NCH = Cfg::NCH, KROW = Cfg::KROW, VROW = Cfg::VROW;
    constexpr int K_IT = Cfg::K_IT, V_IT = Cfg::V_IT, QT = Cfg::QT, TK = VA_TK;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sK = smem;
    char* sV = smem + Cfg::K_BYTES;
    char* sP = sV + Cfg::V_BYTES;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int b = blockIdx.y;
    const int q0 = blockIdx.x * Cfg::QB;
    const int N = p.N;

    const char* Qb = reinterpret_cast<const char*>(p.Q) + (size_t)b * p.q_bs * 2;
    const char* Kb = reinterpret_cast<const char*>(p.K) + (size_t)b * p.k_bs * 2;
    const char* Vb = reinterpret_cast<const char*>(p.VT) + (size_t)b * p.vt_bs * 2;

    // the wave's slice of Q^T (B operand): lane holds query fr of each 16-query tile, channels wave*DS + 32 ks + 8 fq ..
    uint4 qf[KS][QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        int q = q0 + qt * 16 + fr;
        q = q < N ? q : N - 1;   // rows past N are clamped copies: computed, never stored
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            qf[ks][qt] = *reinterpret_cast<const uint4*>(Qb + (size_t)q * p.ldq * 2 + (wave * (DS / 8) + ks * 4 + fq) * 16);
    }

    // staging registers of the next tile
    u32x4 kr[K_IT], vr[V_IT];   // (native vectors: hipcc leaves conditionally written uint4 arrays in scratch memory)
    // per-thread offsets of its chunks in tile 0 (bytes; a sample's K / V^T stay below 2 GiB: checked by the launcher)
    unsigned k_off[K_IT], v_off[V_IT];
#pragma unroll
    for (int i = 0; i < K_IT; ++i) {
        const int s = tid + 256 * i;
        k_off[i] = (unsigned)(s / NCH) * (unsigned)p.ldk * 2u + (unsigned)(s % NCH) * 16u;
    }
#pragma unroll
    for (int i = 0; i < V_IT; ++i) {
        const int s = tid + 256 * i;
        v_off[i] = (unsigned)(s >> 2) * (unsigned)p.vt_ld * 2u + (unsigned)(s & 3) * 16u;
    }
    f32x4 o[NTD][QT];
#pragma unroll
    for (int n = 0; n < NTD; ++n)
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) o[n][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float mrow[QT], lrow[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) { mrow[qt] = -INFINITY; lrow[qt] = 0.f; }
    const float sl2 = p.scale * 1.4426950408889634f;

    // Iteration -1 only stages tile 0.
    const int ntiles = (N + TK - 1) / TK;
    for (int t = -1; t < ntiles; ++t) {
        const int t0 = t * TK;
        const bool more = t + 1 < ntiles;      // block-uniform
        const bool ragged = t0 + 2 * TK > N;   // ... of the tile being staged
        if (more) {
            // no lane branches: a key row past N reads row N - 1 instead (its logits are masked), a V^T chunk past N the row's last
            // chunk (its keys are zeroed on the way into LDS)
#pragma unroll
            for (int i = 0; i < K_IT; ++i) {
                unsigned off = k_off[i] + (unsigned)(t0 + TK) * (unsigned)p.ldk * 2u;
                if (ragged) {
                    const int s = tid + 256 * i;
                    off = (unsigned)min(t0 + TK + s / NCH, N - 1) * (unsigned)p.ldk * 2u + (unsigned)(s % NCH) * 16u;
                }
                kr[i] = *reinterpret_cast<const u32x4*>(Kb + off);
            }
        }
        if (t >= 0) {
        // ---- partial S^T over the wave's channels: 2 key tiles x QT query tiles
        f32x4 s[TK / 16][QT];
#pragma unroll
        for (int kt = 0; kt < TK / 16; ++kt)
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) s[kt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int kt = 0; kt < TK / 16; ++kt) {
                const uint4 kf = *reinterpret_cast<const uint4*>(sK + (kt * 16 + fr) * KROW + (wave * (DS / 8) + ks * 4 + fq) * 16);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) mma_raw<P>(kf, qf[ks][qt], s[kt][qt]);
            }
#pragma unroll
        for (int kt = 0; kt < TK / 16; ++kt)
#pragma unroll
            for (int qt = 0; qt < QT; ++qt)
                *reinterpret_cast<f32x4*>(sP + (((wave * (TK / 16) + kt) * QT + qt) * 64 + lane) * 16) = s[kt][qt];
        }
        __syncthreads();   // partials visible; nobody reads this K tile again
        if (more) {
#pragma unroll
            for (int i = 0; i < K_IT; ++i) {
                const int s = tid + 256 * i;
                *reinterpret_cast<u32x4*>(sK + (s / NCH) * KROW + (s % NCH) * 16) = kr[i];
            }
            // ... and its V^T chunks are requested now: they land behind the second barrier
#pragma unroll
            for (int i = 0; i < V_IT; ++i) {
                unsigned off = v_off[i] + (unsigned)(t0 + TK) * 2u;
                if (ragged) {   // vt_ld >= round_up(N, 8): the chunk that holds key N - 1 is inside the row
                    const int s = tid + 256 * i;
                    off = (unsigned)(s >> 2) * (unsigned)p.vt_ld * 2u + (unsigned)min(t0 + TK + (s & 3) * 8, (N - 1) & ~7) * 2u;
                }
                vr[i] = *reinterpret_cast<const u32x4*>(Vb + off);
            }
        }
        if (t >= 0) {

        // ---- per query tile: full logits (the four partials in wave order, the same sum in every wave), then the online softmax
        // (base 2) of query fr; keys 16 kt + 4 fq + j.  P^T leaves in the k order of the PV step (vt_slot)
        uint4 pf[QT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            f32x4 sf[TK / 16];
            float mx = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < TK / 16; ++kt) {
                f32x4 acc = *reinterpret_cast<const f32x4*>(sP + (((0 * (TK / 16) + kt) * QT + qt) * 64 + lane) * 16);
#pragma unroll
                for (int w = 1; w < 4; ++w) acc += *reinterpret_cast<const f32x4*>(sP + (((w * (TK / 16) + kt) * QT + qt) * 64 + lane) * 16);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int key = t0 + kt * 16 + fq * 4 + j;
                    acc[j] = key < N ? acc[j] * sl2 : -INFINITY;
                    mx = fmaxf(mx, acc[j]);
                }
                sf[kt] = acc;
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mnew = fmaxf(mrow[qt], mx);   // finite: every tile holds at least one key < N
            const float alpha = __builtin_amdgcn_exp2f(mrow[qt] - mnew);
            mrow[qt] = mnew;
            float ps = 0.f;
#pragma unroll
            for (int kt = 0; kt < TK / 16; ++kt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float e = __builtin_amdgcn_exp2f(sf[kt][j] - mnew);
                    sf[kt][j] = e;
                    ps += e;
                }
            lrow[qt] = lrow[qt] * alpha + ps;
#pragma unroll
            for (int n = 0; n < NTD; ++n) o[n][qt] *= alpha;
            pf[qt].x = pack2<P>(sf[0][0], sf[0][1]);
            pf[qt].y = pack2<P>(sf[0][2], sf[0][3]);
            pf[qt].z = pack2<P>(sf[1][0], sf[1][1]);
            pf[qt].w = pack2<P>(sf[1][2], sf[1][3]);
            __builtin_amdgcn_sched_barrier(0);   // one query tile's partials in flight at a time: hoisting all 32 loads costs 128 registers
        }
        // ---- O^T slice += V^T rows . P^T: one K = 32 step over the tile's keys
#pragma unroll
        for (int n = 0; n < NTD; ++n) {
            const uint4 vf = *reinterpret_cast<const uint4*>(sV + (wave * DS + n * 16 + fr) * VROW + fq * 16);
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) mma_raw<P>(vf, pf[qt], o[n][qt]);
        }
        }
        __syncthreads();   // nobody reads this V^T tile or these partials again; the next K tile is visible
        if (more) {        // read behind the next tile's first barrier
#pragma unroll
            for (int i = 0; i < V_IT; ++i) {
                const int s = tid + 256 * i;
                const int d = s >> 2, c = s & 3;
                u32x4 v = vr[i];
                if (ragged) {   // zero the keys past N (0 * garbage must stay 0)
                    const int key = t0 + TK + c * 8;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        v[j] &= (key + 2 * j < N ? 0x0000ffffu : 0u) | (key + 2 * j + 1 < N ? 0xffff0000u : 0u);
                }
                const int s0 = vt_slot(c * 8), s1 = vt_slot(c * 8 + 4);
                *reinterpret_cast<uint2*>(sV + d * VROW + s0 * 2) = make_uint2(v[0], v[1]);
                *reinterpret_cast<uint2*>(sV + d * VROW + s1 * 2) = make_uint2(v[2], v[3]);
            }
        }
    }

    // ---- normalise and store: lane holds channels wave*DS + 16 n + 4 fq + j of query fr
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        float l = lrow[qt];
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        const float inv = 1.0f / l;
        const int q = q0 + qt * 16 + fr;
        if (q >= N) continue;
#pragma unroll
        for (int n = 0; n < NTD; ++n)
            store4(p.O, (size_t)b * p.o_bs + (size_t)q * p.ldo + wave * DS + n * 16 + fq * 4, P, o[n][qt] * inv);
    }
}

template <int P, int C>
int launch_c(const VaeAttnParams& p, hipStream_t s) {
    using Cfg = VaCfg<C>;
    auto kfn = vae_attn_kernel<P, C>;
    static unsigned long long attr_done = 0;
    if (ensure_dyn_smem(reinterpret_cast<const void*>(kfn), Cfg::SMEM, &attr_done)) return 1;
    hipLaunchKernelGGL(kfn, dim3((p.N + Cfg::QB - 1) / Cfg::QB, p.B), dim3(256), Cfg::SMEM, s, p);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

template <int P>
int launch_p(const VaeAttnParams& p, hipStream_t s) {
    switch (p.C) {
        case 128: return launch_c<P, 128>(p, s);
        case 512: return launch_c<P, 512>(p, s);
        default: return 2;
    }
}

}  // namespace

bool vae_attention_eligible(int prec, int C) { return (prec == DT_BF16 || prec == DT_F16) && (C == 128 || C == 512); }

// 0 launched, 1 launch failure, 2 not an instantiated (mode, C) or a layout the 16-byte loads cannot take
int launch_vae_attention(const VaeAttnParams& p, int prec, hipStream_t s) {
    if (p.B <= 0 || p.N <= 0) return 0;
    if (!vae_attention_eligible(prec, p.C)) return 2;
    if (!p.Q || !p.K || !p.VT || !p.O || p.B > 65535) return 2;
    if (p.ldq % 8 || p.ldk % 8 || p.vt_ld % 8 || p.ldo % 4 || p.q_bs % 8 || p.k_bs % 8 || p.vt_bs % 8 || p.o_bs % 4) return 2;
    if (p.ldq < p.C || p.ldk < p.C || p.ldo < p.C || p.vt_ld < (p.N + 7) / 8 * 8) return 2;
    if ((long long)p.N * p.ldk * 2 >= (1ll << 31) || (long long)p.C * p.vt_ld * 2 >= (1ll << 31)) return 2;   // 32-bit offsets inside a sample
    if ((reinterpret_cast<uintptr_t>(p.Q) | reinterpret_cast<uintptr_t>(p.K) | reinterpret_cast<uintptr_t>(p.VT)) & 15 || reinterpret_cast<uintptr_t>(p.O) & 7) return 2;
    return prec == DT_BF16 ? launch_p<DT_BF16>(p, s) : launch_p<DT_F16>(p, s);
}
