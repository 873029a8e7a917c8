// What the three LDS-patch conv3x3 kernels (conv_patch.hip, conv_patch2.hip, conv_patch4.hip) share: the tile geometry -- which output
// pixels a block owns and where the LDS patch under them starts -- the split-K slice, and the host side (eligibility, grid,
// launcher).  A change to the tiling starts here; the schedules (who requests what when, the waits, the MFMA order) stay in the kernels.
//
// Tiling.  A block owns a TP x TP patch of output pixels of one sample x BN output channels.  Per 128-byte channel chunk (ROWB) the
// source pixels under the patch and its 1-pixel border -- PW x PW of them, at source resolution when the nearest-x2 upsample is fused --
// sit in LDS as PROWS rows of ROWB bytes, row-major ("LDS patch row" = iy * PW + ix, pixel (sy0 + iy, sx0 + ix) of the source), and all
// 9 taps run from them; the [BN x ROWB] weight tile of each (chunk, tap) unit streams from L2.
//
// Three uses of a PatchTile are still written out in each kernel, in the same words: the source address / in-image test of a patch
// piece, the LDS patch row of an output pixel for a tap, and the two-pass epilogue of generations 1 and 2.  As shared inline functions
// (by reference, by value, on scalars) each of them changed the instruction counts of at least two of the kernels -- hipcc's
// reassociation of the address arithmetic depends on where the expression is inlined from -- and these kernels are held to their
// parent's code, count for count.
#pragma once
#include "pd_common.h"
#include "pd_mma.h"

namespace patch_conv {

constexpr int TP = 16;             // patch is TP x TP output pixels
constexpr int BN = 160;            // output channels per block
constexpr int ROWB = 128;          // bytes of K per LDS row
constexpr int W_TILE = BN * ROWB;  // 20480

// each generation derives its own piece counts (and LDS size) from this
template <int UPS>
struct PatchGeomBase {
    static constexpr int PW = UPS ? TP / 2 + 2 : TP + 2;   // patch rows/cols held in LDS (source resolution)
    static constexpr int PROWS = PW * PW;
    static constexpr int P_BYTES = PROWS * ROWB;
};

// number of blocks (per split-K slice) of a launch
static inline int patch_grid_tiles(const GemmParams& p) {
    return (p.M / (p.Hout * p.Wout)) * (p.Hout / TP) * (p.Wout / TP) * ((p.N + BN - 1) / BN);
}

// patch_grid_tiles() when the shape qualifies for the patch kernels (generation 1 takes all of these), else 0
static inline int patch_eligible_tiles(const GemmParams& p, int prec) {
    const int bke = prec_f32_storage(prec) ? 32 : 64;
    if (p.taps != 9 || p.stride != 1) return 0;
    if (p.Hout % TP || p.Wout % TP || p.Cin % bke || p.K != 9 * p.Cin || p.act == 2 || p.vt_begin < p.N) return 0;
    if (p.a_dt != (prec_f32_storage(prec) ? (int)DT_F32 : prec) || p.a_silu) return 0;
    if (p.Cin * 8 > 24 * 1024) return 0;
    if (p.act == 5 && (p.ups || p.gn_coef)) return 0;   // ACT_RELU is instantiated for the plain conv only
    if ((p.Hin << p.ups) != p.Hout || (p.Win << p.ups) != p.Wout) return 0;
    return patch_grid_tiles(p);
}
// ... of which generations 2 and 4 take the 2-byte compute types without a fused GroupNorm
static inline bool conv_patch_eligible_2byte(const GemmParams& p, int prec) {
    return (prec == DT_F16 || prec == DT_BF16) && !p.gn_coef && patch_eligible_tiles(p, prec) > 0;
}

// One launcher for every instantiation of the three kernels: opt in to the dynamic LDS once per device, one block per tile x split-K
// slice, then the finalize pass of a split launch unless the consumer sums the slabs itself.
template <auto KFN, int NTHREADS>
int launch_patch_grid(const GemmParams& p, int smem, hipStream_t s) {
    static unsigned long long attr_done = 0;
    if (ensure_dyn_smem(reinterpret_cast<const void*>(KFN), smem, &attr_done)) return 1;
    hipLaunchKernelGGL(KFN, dim3(patch_grid_tiles(p), p.splitk > 1 ? p.splitk : 1), dim3(NTHREADS), smem, s, p);
    if (hipGetLastError() != hipSuccess) return 1;
    return (p.splitk > 1 && !p.defer_finalize) ? launch_splitk_finalize(p, s) : 0;
}

// The block's tile: channel tile bn, sample, patch origin (y0, x0) in output coordinates, and the source-resolution pixel (sy0, sx0)
// that LDS patch row 0 holds (outside the image along the top / left border).
struct PatchTile { int bn, sample, y0, x0, sy0, sx0; };

template <int UPS>
__device__ __forceinline__ PatchTile patch_tile(const GemmParams& p) {
    const int ptx = p.Wout / TP, pty = p.Hout / TP;
    const int mtiles = (p.M / (p.Hout * p.Wout)) * ptx * pty, ntiles = (p.N + BN - 1) / BN;
    const int bid = xcd_tile_order(blockIdx.x, mtiles * ntiles);
    const int bm = bid / ntiles;
    PatchTile t;
    t.bn = bid % ntiles;
    t.sample = bm / (ptx * pty);
    const int prem = bm - t.sample * (ptx * pty);
    t.y0 = (prem / ptx) * TP; t.x0 = (prem - (prem / ptx) * ptx) * TP;
    t.sy0 = (t.y0 - 1) >> UPS; t.sx0 = (t.x0 - 1) >> UPS;
    return t;
}

// The phase conv's tile (conv_upfold.hip): the grid is 4 x the plain grid over the source image, phase slowest -- the blocks in
// flight share one phase's weight panels -- and each phase's run of blocks takes the XCD order of a plain launch.
__device__ __forceinline__ PatchTile patch_phase_tile(const GemmParams& p, int& phase) {
    const int ptx = p.Wout / TP, pty = p.Hout / TP;
    const int mtiles = (p.M / (p.Hout * p.Wout)) * ptx * pty, ntiles = (p.N + BN - 1) / BN;
    phase = blockIdx.x / (mtiles * ntiles);
    const int bid = xcd_tile_order(blockIdx.x - phase * (mtiles * ntiles), mtiles * ntiles);
    const int bm = bid / ntiles;
    PatchTile t;
    t.bn = bid % ntiles;
    t.sample = bm / (ptx * pty);
    const int prem = bm - t.sample * (ptx * pty);
    t.y0 = (prem / ptx) * TP; t.x0 = (prem - (prem / ptx) * ptx) * TP;
    t.sy0 = t.y0 - 1; t.sx0 = t.x0 - 1;
    return t;
}

// split-K (blockIdx.y): slice `slice` of `splitk` owns the channel chunks [c0, c0 + nchunks) of chunks_all = Cin / BKE; the last
// slice may be shorter, none is empty (pd_engine::plan_gemm)
struct ChunkSlice { int c0, nchunks; };
__device__ __forceinline__ ChunkSlice patch_chunk_slice(int chunks_all, int splitk, int slice) {
    ChunkSlice k{0, chunks_all};
    if (splitk > 1) {
        const int per = (chunks_all + splitk - 1) / splitk;
        k.c0 = slice * per;
        k.nchunks = min(chunks_all, k.c0 + per) - k.c0;
    }
    return k;
}

}  // namespace patch_conv
