// conv3x3(nearest_x2(x)) as four 2x2-tap phase convolutions over the SOURCE image -- 2-byte compute types (bf16 / fp16), gfx950.
//
// An output pixel (2y + py, 2x + px) of the upsampled conv sees only a 2x2 neighbourhood of the source: its nine taps collapse into
// four whose weights are sums of the original ones (rows: parity 0 reads {y-1, y} with {w[0], w[1] + w[2]}, parity 1 reads {y, y+1}
// with {w[0] + w[1], w[2]}; columns alike).  The zero padding of the 2H x 2W image maps onto the zero padding of the H x W source.
// So the nine-tap kernels (UPS = 1 of conv_patch*.hip) multiply every source value by weights it has already been multiplied by:
// 9 products where 4 do.  upfold_weights_kernel builds the four [N][4][Cin] matrices (fp32 sum of the stored weights, rounded once);
// conv3x3_upfold_kernel is conv_patch2.hip's wave-specialised schedule over the PLAIN geometry (16x16 source pixels per block, the
// 18x18 LDS patch whose row 0 is source row y0 - 1) with 4 units per channel chunk: tap (ty, tx) of phase (py, px) reads exactly
// where plain tap (py + ty, px + tx) reads, so the patch staging, zero fill and swizzle are conv_patch2.hip's.  What differs: the
// unit list (4 taps, the phase's matrix), the next chunk's patch pieces (all 11 requested at tap 0, stored at tap 2: the compute
// waves first read them in the second half of tap 3), the output address, and the grid (phase x tile, phase slowest, so that the
// blocks in flight share one phase's weight panels like the nine-tap launch shares its own).
// The second generation and not the fourth: its schedule is written per unit (a ring of three weight tiles, patch pieces as plain
// register loads), where conv_patch4.hip's is written around nine units per chunk (ring slot tap % 3, pieces spread over taps 1-7).
//
// Not bit-identical to the nine-tap path: every folded weight is rounded once more and the fp32 partial sums associate differently.
// On operands whose products, folded weights and sums are exact it is (tests/test_upfold_gpu.py).
#include <type_traits>

#include "conv_patch_common.h"

namespace {
using namespace patch_conv;

constexpr int NT = 512;            // threads: 4 compute waves + 4 loader waves
constexpr int NL = 256;            // loader threads
constexpr int BKE = 64;            // two-byte channels per LDS row
constexpr int W_IT = BN * 8 / NL;  // 5 16-byte pieces per loader thread and weight tile
constexpr int NWB = 3;             // weight tile buffers
constexpr int NTAP = 4;            // units per channel chunk

struct GeomUp : PatchGeomBase<0> {
    static constexpr int P_SLOTS = PROWS * 8;
    static constexpr int P_IT = (P_SLOTS + NL - 1) / NL;   // 11 pieces per loader thread
    static constexpr int SMEM = 2 * P_BYTES + NWB * W_TILE;
};
static_assert(GeomUp::P_IT == 11, "the loader's named staging registers");

// p: the launch in SOURCE geometry (launch_conv_upfold): Hout = Hin, Wout = Win, M = B * Hin * Win for the tile decode; p.W the four
// phase matrices [4][N][Kpad = 4 * Cin]; rows_per_sample / ldc those of the 2H x 2W output.
template <int P>
__global__ __launch_bounds__(NT) void conv3x3_upfold_kernel(GemmParams p) {
    using G = GeomUp;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sP = smem;                    // [2][PROWS][128]
    char* sW = smem + 2 * G::P_BYTES;   // [3][160][128]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;

    int ph;
    const PatchTile t = patch_phase_tile(p, ph);
    const int bn = t.bn, sample = t.sample, y0 = t.y0, x0 = t.x0, sy0 = t.sy0, sx0 = t.sx0;
    const int phy = ph >> 1, phx = ph & 1;

    const int nchunks = p.Cin / BKE;
    const int U = nchunks * NTAP;  // (chunk, tap) units; weights of unit (lc, tap) start at element tap*Cin + lc*BKE of the phase's rows

    if (wave >= 4) {
        // =============================================================== loader waves
        const int lt = tid - NL;
        const char* Ab = reinterpret_cast<const char*>(p.A);
        const char* Wb = reinterpret_cast<const char*>(p.W) + (size_t)ph * p.N * p.Kpad * 2;
        unsigned w_off[W_IT];
        int w_lds[W_IT];
#pragma unroll
        for (int j = 0; j < W_IT; ++j) {
            const int s = lt + NL * j;
            const int row = s >> 3, ch = s & 7;
            int n = bn * BN + row;
            n = n < p.N ? n : p.N - 1;      // channels >= N are never stored
            w_off[j] = (unsigned)(((size_t)n * p.Kpad + ch * 8) * 2);
            w_lds[j] = swz8(row, ch);
        }
        // patch slot j of this thread: LDS offset (-1: none), in-image flag, byte offset of channel chunk 0 in A
        auto patch_slot = [&](int j, int& lds, bool& ok, unsigned& off) __attribute__((always_inline)) {
            const int s = lt + NL * j;
            const int prow = s >> 3, ch = s & 7;
            const int iy = prow / G::PW, ix = prow - iy * G::PW;
            const int gy = sy0 + iy, gx = sx0 + ix;
            ok = s < G::P_SLOTS && (unsigned)gy < (unsigned)p.Hin && (unsigned)gx < (unsigned)p.Win;
            off = ok ? (unsigned)((((size_t)(sample * p.Hin + gy) * p.Win + gx) * p.lda + ch * 8) * 2) : 0u;
            lds = s < G::P_SLOTS ? swz8(prow, ch) : -1;
        };
        unsigned p_off[G::P_IT];
#pragma unroll
        for (int j = 0; j < G::P_IT; ++j) {
            int lds; bool ok;
            patch_slot(j, lds, ok, p_off[j]);
        }
        // staging registers are NAMED scalars (hipcc leaves indexed uint4 arrays of such loops in scratch memory)
        uint4 wr0, wr1, wr2, wr3, wr4, pr0, pr1, pr2, pr3, pr4, pr5, pr6, pr7, pr8, pr9, pr10;
#define PD_W5(X) X(0, wr0) X(1, wr1) X(2, wr2) X(3, wr3) X(4, wr4)
#define PD_P11(X) X(0, pr0) X(1, pr1) X(2, pr2) X(3, pr3) X(4, pr4) X(5, pr5) X(6, pr6) X(7, pr7) X(8, pr8) X(9, pr9) X(10, pr10)
#define W_LD(j, r) r = *reinterpret_cast<const uint4*>(bw + w_off[j]);
#define W_ST(j, r) *reinterpret_cast<uint4*>(dw + w_lds[j]) = r;
#define P_LD(j, r) r = *reinterpret_cast<const uint4*>(an + p_off[j]);
#define P_ST(j, r)                                                        \
    {                                                                     \
        int lds; bool ok; unsigned off;                                   \
        patch_slot(j, lds, ok, off);                                      \
        uint4 v = r;                                                      \
        if (!ok) v = make_uint4(0, 0, 0, 0);                              \
        if (lds >= 0) *reinterpret_cast<uint4*>(pn + lds) = v;            \
    }
        // weight tile of unit v (clamped to the last unit: requests stay unconditional, see conv_patch.hip)
        auto w_base = [&](int v) __attribute__((always_inline)) {
            v = v < U ? v : U - 1;
            const int lc = v / NTAP, tap = v - lc * NTAP;
            return Wb + ((size_t)tap * p.Cin + (size_t)lc * BKE) * 2;
        };
        // ---- prologue: patch of chunk 0 and the weight tiles of units 0 and 1
        {
            const char* an = Ab;
            char* pn = sP;
            PD_P11(P_LD)
            const char* bw = w_base(0);
            char* dw = sW;
            PD_W5(W_LD)
            PD_P11(P_ST)
            PD_W5(W_ST)
            bw = w_base(1);
            dw = sW + W_TILE;
            PD_W5(W_LD)
            PD_W5(W_ST)
        }
        __syncthreads();
        int wbuf = 2;   // buffer of tile u + 2
        for (int lc = 0; lc < nchunks; ++lc) {
            const bool nextc = lc + 1 < nchunks;
            const char* an = Ab + (size_t)(nextc ? lc + 1 : lc) * BKE * 2;
            char* pn = sP + ((lc + 1) & 1) * G::P_BYTES;   // next chunk's patch buffer (last read in chunk lc-1)
#pragma unroll
            for (int tap = 0; tap < NTAP; ++tap) {
                const int u = lc * NTAP + tap;
                // weight tile of unit u+2 first (L2), HBM-latency patch pieces after it: vmcnt retires in issue order
                const char* bw = w_base(u + 2);
                PD_W5(W_LD)
                if (tap == 0) { PD_P11(P_LD) }
                // stored one barrier before the compute waves' first read of them (second half of tap 3)
                if (tap == 2 && nextc) { PD_P11(P_ST) }
                // tile u+2 -> buffer (u+2) % 3, last read by the compute waves in unit u-1
                char* dw = sW + wbuf * W_TILE;
                PD_W5(W_ST)
                wbuf = wbuf == NWB - 1 ? 0 : wbuf + 1;
                __syncthreads();
            }
        }
#undef PD_W5
#undef PD_P11
#undef W_LD
#undef W_ST
#undef P_LD
#undef P_ST
        return;
    }

    // =================================================================== compute waves
    __builtin_amdgcn_s_setprio(1);
    const int wm = wave;   // patch rows wm*4 .. wm*4+3
    f32x4 acc[10][4];
#pragma unroll
    for (int n = 0; n < 10; ++n)
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[n][m] = f32x4{0.f, 0.f, 0.f, 0.f};

    // A fragment of patch row wm*4+m for tap (ty,tx), k-step ks: 16 consecutive LDS patch rows (16 x of one patch row); LDS patch
    // row 0 is source row y0 - 1, so the phase only shifts the window by (phy, phx)
    auto af_off = [&](int m, int ty, int tx, int ks, int frv) __attribute__((always_inline)) {
        const int prow = (wm * 4 + m + phy + ty) * G::PW + frv + phx + tx;
        return swz8(prow, ks * 4 + fq);
    };
    // W fragment of channel tile n: (row>>1)&7 of row n*16+fr does not depend on n -> one base + n*2048
    auto wf_off = [&](int ks, int frv) __attribute__((always_inline)) { return swz8(frv, ks * 4 + fq); };

    uint4 afA[4], afB[4];   // A fragments of the ks = 0 / ks = 1 half-unit
    // weight fragments: a ring of 4, requested 3 MFMA groups ahead of their use.  Fragment g of a unit: ks = g / 10, n = g % 10.
    uint4 w0, w1, w2, w3;
    auto WR = [&](auto G4) __attribute__((always_inline)) -> uint4& {
        constexpr int r = decltype(G4)::value & 3;
        if constexpr (r == 0) return w0; else if constexpr (r == 1) return w1; else if constexpr (r == 2) return w2; else return w3;
    };

    __syncthreads();        // prologue of the loader waves: patch 0 and weight tiles 0, 1 are in LDS
    {
        int frv = fr;
        asm volatile("" : "+v"(frv));
#pragma unroll
        for (int m = 0; m < 4; ++m) afA[m] = *reinterpret_cast<const uint4*>(sP + af_off(m, 0, 0, 0, frv));
        const int wo0 = wf_off(0, frv);
        w0 = *reinterpret_cast<const uint4*>(sW + wo0);
        w1 = *reinterpret_cast<const uint4*>(sW + wo0 + 1 * 16 * ROWB);
        w2 = *reinterpret_cast<const uint4*>(sW + wo0 + 2 * 16 * ROWB);
    }
    int wbuf = 0;
    auto unit = [&](auto TAPC, int lc) __attribute__((always_inline)) {
        constexpr int tap = decltype(TAPC)::value;
        constexpr int ty = tap / 2, tx = tap % 2;
        constexpr int ntap = tap == NTAP - 1 ? 0 : tap + 1, nty = ntap / 2, ntx = ntap % 2;
        const int u = lc * NTAP + tap;
        const char* pa = sP + (lc & 1) * G::P_BYTES;
        const char* wa = sW + wbuf * W_TILE;
        const int nwbuf = wbuf == NWB - 1 ? 0 : wbuf + 1;
        const char* pan = sP + ((tap == NTAP - 1 ? lc + 1 : lc) & 1) * G::P_BYTES;   // patch / weight buffers of unit u+1
        const char* wan = sW + nwbuf * W_TILE;
        const bool more = u + 1 < U;
        // keep the per-tap fragment addresses out of loop-invariant hoisting (they would take the accumulators' registers)
        int frv = fr;
        asm volatile("" : "+v"(frv));
        const int wo0 = wf_off(0, frv), wo1 = wf_off(1, frv);
        // fragments afA and ring slots 0..2 were requested during the previous unit.  The first fragments of unit u+1 are requested in
        // this unit's second half, BEFORE the barrier (its weight tile was completed one barrier ago, its patch -- another buffer only
        // at the last tap -- at tap 2).  Requests are unconditional (the last unit re-reads valid LDS of its own buffers): a branch
        // would split the scheduling region that the sched_group_barrier pattern below lays out
        const char* pan2 = more ? pan : pa;
        const char* wan2 = more ? wan : wa;
        static_for<20>([&](auto GI) __attribute__((always_inline)) {
            constexpr int g = decltype(GI)::value;
            constexpr int ks = g / 10, n = g % 10;
            constexpr int g3 = g + 3;            // fragment requested now
            if constexpr (g3 < 20) {
                constexpr int ks3 = g3 / 10, n3 = g3 % 10;
                WR(std::integral_constant<int, g3>{}) = *reinterpret_cast<const uint4*>(wa + (ks3 ? wo1 : wo0) + n3 * 16 * ROWB);
            } else {
                WR(std::integral_constant<int, g3>{}) = *reinterpret_cast<const uint4*>(wan2 + wo0 + (g3 - 20) * 16 * ROWB);
            }
            if constexpr (g < 4) afB[g] = *reinterpret_cast<const uint4*>(pa + af_off(g, ty, tx, 1, frv));
            if constexpr (g >= 12 && g < 16) afA[g - 12] = *reinterpret_cast<const uint4*>(pan2 + af_off(g - 12, nty, ntx, 0, frv));
            const uint4 wc = WR(GI);
#pragma unroll
            for (int m = 0; m < 4; ++m) mma<P>(wc, ks ? afB[m] : afA[m], acc[n][m]);
        });
        // pin the interleave (conv_patch2.hip): per MFMA group of 4, the LDS reads issued in front of it
        static_for<20>([&](auto GI) __attribute__((always_inline)) {
            constexpr int g = decltype(GI)::value;
            __builtin_amdgcn_sched_group_barrier(0x100, (g < 4 || (g >= 12 && g < 16)) ? 2 : 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        });
        wbuf = nwbuf;
        __syncthreads();
    };
    for (int lc = 0; lc < nchunks; ++lc) {
        unit(std::integral_constant<int, 0>{}, lc);
        unit(std::integral_constant<int, 1>{}, lc);
        unit(std::integral_constant<int, 2>{}, lc);
        unit(std::integral_constant<int, 3>{}, lc);
    }
    __builtin_amdgcn_s_setprio(0);

    // ---- epilogue: bias only (launch_conv_upfold refuses everything else); source pixel (y, x) -> output pixel (2y + phy, 2x + phx)
    const int Wo = 2 * p.Win;
#pragma unroll
    for (int n = 0; n < 10; ++n) {
        const int gn = min(bn * BN + n * 16 + fq * 4, p.N - 4);
        if (p.bias) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(p.bias + gn);
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[n][m] += b;
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int oy = 2 * (y0 + wm * 4 + m) + phy, ox = 2 * (x0 + fr) + phx;
        const size_t gm = (size_t)sample * p.rows_per_sample + (size_t)oy * Wo + ox;
#pragma unroll
        for (int n = 0; n < 10; ++n) {
            const int gn = bn * BN + n * 16 + fq * 4;
            if (gn >= p.N) continue;
            store4(p.C, gm * p.ldc + gn, p.c_dt, acc[n][m]);
        }
    }
}

// One thread per 8 channels of one (phase, output channel, tap): the fp32 sum of the 1, 2 or 4 stored weights it stands for, rounded once.
// S(parity, tap): parity 0 -> {0}, {1, 2}; parity 1 -> {0, 1}, {2}.
__global__ void upfold_weights_kernel(const uint16_t* __restrict__ w, uint16_t* __restrict__ wf, int dt, int N, int cin, int Kpad) {
    const int c8 = cin / 8;
    const long long total = 16ll * N * c8;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % c8) * 8;
    const int t = (int)((i / c8) % 4);
    const int n = (int)((i / (4ll * c8)) % N);
    const int ph = (int)(i / (4ll * c8 * N));
    const int py = ph >> 1, px = ph & 1, ty = t >> 1, tx = t & 1;
    const int ky0 = py + ty == 0 ? 0 : py + ty == 2 ? 2 : (py ? 0 : 1), nky = py + ty == 1 ? 2 : 1;
    const int kx0 = px + tx == 0 ? 0 : px + tx == 2 ? 2 : (px ? 0 : 1), nkx = px + tx == 1 ? 2 : 1;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int ky = ky0; ky < ky0 + nky; ++ky)
        for (int kx = kx0; kx < kx0 + nkx; ++kx) {
            const uint4 v = *reinterpret_cast<const uint4*>(w + (size_t)n * Kpad + (size_t)(ky * 3 + kx) * cin + c);
            const uint16_t* h = reinterpret_cast<const uint16_t*>(&v);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += cvt32_rt(h[j], dt);
        }
    uint4 o;
    uint16_t* oh = reinterpret_cast<uint16_t*>(&o);
#pragma unroll
    for (int j = 0; j < 8; ++j) oh[j] = cvt16_rt(s[j], dt);
    *reinterpret_cast<uint4*>(wf + ((size_t)ph * N + n) * (4 * (size_t)cin) + (size_t)t * cin + c) = o;
}

template <int P>
int launch_upfold(const GemmParams& q, hipStream_t s) {
    static unsigned long long attr_done = 0;
    if (ensure_dyn_smem(reinterpret_cast<const void*>(conv3x3_upfold_kernel<P>), GeomUp::SMEM, &attr_done)) return 1;
    hipLaunchKernelGGL(conv3x3_upfold_kernel<P>, dim3(4 * patch_grid_tiles(q)), dim3(NT), GeomUp::SMEM, s, q);
    return hipGetLastError() != hipSuccess;
}

}  // namespace

// the shape / epilogue gate of the phase conv (p: fill_gemm's nine-tap parameters of the upsampling call)
bool conv_upfold_eligible(const GemmParams& p, int prec) {
    if (prec != DT_F16 && prec != DT_BF16) return false;
    if (p.taps != 9 || p.stride != 1 || p.ups != 1 || p.pad_shift || p.splitk > 1) return false;
    if (p.Hin % TP || p.Win % TP || p.Hout != 2 * p.Hin || p.Wout != 2 * p.Win) return false;
    if (p.Cin % BKE || p.K != 9 * p.Cin || p.Cin * 8 > 24 * 1024 || p.N % 4 || p.a_dt != prec) return false;
    // bias-only epilogue
    if (p.R || p.rowvec || p.VT || p.vt_begin < p.N || p.act || p.a_silu || p.out_scale != 1.f || p.gn_coef || p.ln_stats || p.stats_out ||
        p.gate || p.c_sample_rows || p.a_sample_rows || p.a_scale || p.c_scale)
        return false;
    return true;
}
// blocks of the phase launch: 4 x B x (H/16)(W/16) x ceil(N/160)
int conv_upfold_tiles(const GemmParams& p) {
    return 4 * (p.M / (p.Hout * p.Wout)) * (p.Hin / TP) * (p.Win / TP) * ((p.N + BN - 1) / BN);
}

// w_up: the four phase matrices [4][N][4 * Cin] of launch_upfold_weights
int launch_conv_upfold(const GemmParams& p, const void* w_up, int prec, hipStream_t s) {
    if (!conv_upfold_eligible(p, prec) || !w_up) return 1;
    GemmParams q = p;
    q.W = w_up; q.Kpad = 4 * p.Cin; q.K = 4 * p.Cin;
    q.Hout = p.Hin; q.Wout = p.Win; q.M = (p.M / (p.Hout * p.Wout)) * p.Hin * p.Win; q.ups = 0;   // the tile decode runs over the source
    return prec == DT_F16 ? launch_upfold<DT_F16>(q, s) : launch_upfold<DT_BF16>(q, s);
}

int launch_upfold_weights(const void* w, void* w_up, int dt, int N, int cin_pad, int Kpad, hipStream_t s) {
    if ((dt != DT_F16 && dt != DT_BF16) || cin_pad % 8) return 1;
    const long long total = 16ll * N * (cin_pad / 8);
    hipLaunchKernelGGL(upfold_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const uint16_t*>(w),
                       reinterpret_cast<uint16_t*>(w_up), dt, N, cin_pad, Kpad);
    return hipGetLastError() != hipSuccess;
}
