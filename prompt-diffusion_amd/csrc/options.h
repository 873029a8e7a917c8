// pdengine: the engine's options.  One struct (pd_engine::opt, per engine: nothing here is process-wide) and one table with a row per
// key (kOptions): pd_set_option / pd_get_option / pd_option_info in options.cpp read nothing else.  A new knob is one field and one row.
//
// Every field is an int, so that a row can point at any of them; the on / off knobs hold 0 / 1.  A default is written once, at its
// field: the table takes it from EngineOptions{}.  Tile-count options (splitk_tiles, dense_tiles, conv_patch2_tiles, patch_split_tiles,
// patch_split_fill) are stored as given, as numbers for a 256-CU part; ChipFill (engine.h) scales them to the device where the plan reads them.
#pragma once
#include <cstdint>

struct EngineOptions {
    int verbose = 0;           // 1: workspace sizes; 2: one stderr line per contraction launch (the dispatch trace)
    int two_streams = 1;       // ControlNet pass on a second stream beside the UNet encoder (forward_eps, sd3_forward)
    int cfg_share = 1;         // option "cfg_share": the layers in front of the first cross-attention once per CFG pair (forward_eps)
    int graph = 0;             // pd_ddim_sample: capture the step loop in a hipGraph and replay it on later calls with the same arguments
    int conv_patch = 1;        // use the LDS-patch conv3x3 kernel where eligible
    int conv_patch2 = 1;       // 2-byte modes: the wave-specialised second-generation patch kernel (conv_patch2.hip)
    int conv_patch2_tiles = 768;   // ... for launches of at least this many blocks (and every split-K patch launch)
    int patch4 = 1;            // 2-byte modes: the 4-wave patch kernel (conv_patch4.hip) for unsplit launches
    int patch_split = 1;       // LDS-patch conv with the channel chunks split over 2-4 slices (16x16 level)
    int patch_split_tiles = 64;
    int patch_split_fill = 256;    // slices are chosen to reach about this many blocks
    int patch_split_min = 4;       // ... each slice at least this many 128-byte channel chunks.  (min 1 / tiles 32 measured +2.3 % at batch 1 and
                                   // neutral at batch 8, but re-associates the sums of the 256x256 parity fixture's convs: its step-0 latent error
                                   // moves from 7.4e-4 to 1.02e-3 -- same arithmetic, other rounding pattern -- so the defaults stay)
    // apply GroupNorm(+SiLU) inside the patch conv's staging.  Measured neutral-to-negative in round 1 (the SiLU VALU work
    // lands on the MFMA waves and the halo is transformed 1.27x redundantly), so it is off by default.
    int gn_fuse = 0;
    int ln_fuse = -1;          // -1: on in the 2-byte modes, off in the fp32-storage modes; 0 / 1: forced
    int gn_single = 1;         // GroupNorm as one LDS-slab kernel where a sample's group bundle fits (32x32 and below)
    int gn_reg = 1;            // ... its register-resident form where it applies (norm.hip: gn_reg_vb)
    int big_tile = 1;          // 256-row GEMM tiles where the grid still fills the chip
    int wide_tile = 1;         // 256 x 320 GEMM tiles for large-M linear layers
    int dense_k = 40;          // linear layers with at most this many K steps and >= dense_tiles tiles: one 8-wave block per CU, no split-K
    int dense_tiles = 128;
    int short_k = 20;          // linear layers with at most this many K steps: 8-wave 128x160 tile at 16 waves per CU
    int splitk_tiles = 256;    // split K when the 128x160 tile grid has fewer blocks than this (one tile per CU needs no split:
                               // 384 sent the 16x16 level's 5120 -> 1280 feed-forward-out GEMM -- 256 tiles -- to split-K 2 + a finalize pass, 86 us; the ring
                               // GEMM takes it unsplit in ~60: +0.5 % end to end)
    int splitk_max = 16;       // (8 until the end of round 4: the 8x8 level at batch 1 -- M = 128, 8 tiles -- then ran on 64 blocks; 16: +1.5 % at batch 1, nothing at batch 8)
    int splitk_big = 0;        // split-K conv3x3 on 256 x 160 tiles where that still fills the chip (option "splitk_big")
    int splitk_fused = 0;      // split-K sums + epilogue run in the last-arriving slice instead of a finalize kernel
    int tile192 = 1;           // 256 x 192 GEMM tiles for widths that divide by 192 but not by 160 (MMDiT)
    int gemv = 1;              // Linear over <= 4 fp32 rows with a wide output (MMDiT modulation): weight-streaming kernel instead of a GEMM tile
    int sd3_fp8 = 0;           // SD3 path: QKV and feed-forward-in projections in PREC_FP8 (e4m3 operands, per-row scales).  0 off, 1: the AdaLN-fed
                               // projections, 2: also the feed-forward-out projections (e4m3 GELU output under a norm bound)
    int attn_legacy = 0;       // debug: single-buffered attention kernel
    int st_fuse = 1;           // 320-channel SpatialTransformer blocks: one kernel for everything after self-attention (2-byte modes)
    int ring = 80;             // linear layers with at most this many K steps (0: off) take gemm_ring.hip's persistent LDS-DMA ring kernel
    int ring_tile = -1;        // its tile: -1 auto, 0 = 128 x 160, 1 = 256 x 160
    int ring_geglu = 1;        // GEGLU projections too (256 x 160 on 8 x 1 waves)
    int ring_small = 4;        // small-M linear layers on 64 x 80 ring tiles instead of split-K (option "ring_small"): 0 off, d: where the 128 x 160 grid fills at most 1 / d of the chip
    int ring_pp = 1;           // its ping-pong form where it measures faster (long K, or one 256-row tile per CU)
    int slab_gn = 1;           // split-K conv1 -> single-kernel norm2 without a finalize pass (SlabDefer; option "slab_gn")
    int ups_fold = 1;          // decoder Upsample convs as four 2x2-tap phase convs (2-byte modes)
    int ups_fold_tiles = -1;   // ... when the phase grid has at least this many blocks; -1: where patch_unsplit() admits an unsplit launch
    int vae_flash = -1;        // option "vae_flash": -1 per VAE (VaeDesc::flash_auto), 0 / 1 forced; 2-byte modes only
    int pag_fork = 1;          // perturbed-attention guidance: the perturbed branch begins at the first perturbed block (1) or is a full third of
                               // the UNet's batch from conv_in on (0: the plain evaluation the fork is tested and timed against); kSwitches
    int gemm_tile = -1;        // test surface: GemmPlan::big_tile of every igemm-family launch (-1: the plan's own)
    int gemm_splitk = -1;      // ... its K slices: -1 the plan's own, 1 never, n >= 2 that many where launch_gemm takes a split launch
};

// How pd_set_option converts a value: value != 0; (int)value; value < 0 ? -1 : value != 0; a command with a body of its own ("profile")
enum OptKind { OPT_BOOL, OPT_INT, OPT_TRI, OPT_COMMAND };
// What a stored value invalidates besides the captured graphs
enum OptEffect { OPT_FX_NONE, OPT_FX_LN /* ln_dirty: the folded transformer / upsample weights */, OPT_FX_SD3_FP8 /* sd3_fp8_dirty: the e4m3 weights */ };

struct OptionRow {
    const char* key;
    int EngineOptions::*member;    // null: OPT_COMMAND
    OptKind kind;
    int64_t def;
    OptEffect effect = OPT_FX_NONE;
    bool (*accepts)(int64_t) = nullptr;      // null: every value (most knobs are unchecked: tests and tools pass values such as ring = 1000)
    const char* range_error = nullptr;       // the message of a refused value
};

// a row: key = the field's name, default = the field's initialiser; then, where they apply, effect, range check and its message
#define PD_OPT(name, kind, ...) {#name, &EngineOptions::name, kind, EngineOptions{}.name, __VA_ARGS__}
inline constexpr OptionRow kOptions[] = {
    PD_OPT(verbose, OPT_INT),
    {"profile", nullptr, OPT_COMMAND, 0},
    PD_OPT(two_streams, OPT_BOOL),
    PD_OPT(cfg_share, OPT_BOOL),
    PD_OPT(graph, OPT_BOOL),
    PD_OPT(conv_patch, OPT_BOOL),
    PD_OPT(conv_patch2, OPT_BOOL),
    PD_OPT(conv_patch2_tiles, OPT_INT),
    PD_OPT(patch4, OPT_BOOL),
    PD_OPT(patch_split, OPT_BOOL),
    PD_OPT(patch_split_tiles, OPT_INT),
    PD_OPT(patch_split_fill, OPT_INT),
    PD_OPT(patch_split_min, OPT_INT, OPT_FX_NONE, [](int64_t v) { return v >= 1; }, "patch_split_min must be >= 1"),
    PD_OPT(gn_fuse, OPT_BOOL),
    PD_OPT(ln_fuse, OPT_INT, OPT_FX_LN),
    PD_OPT(gn_single, OPT_BOOL),
    PD_OPT(gn_reg, OPT_BOOL),
    PD_OPT(big_tile, OPT_BOOL),
    PD_OPT(wide_tile, OPT_BOOL),
    PD_OPT(dense_k, OPT_INT),
    PD_OPT(dense_tiles, OPT_INT),
    PD_OPT(short_k, OPT_INT),
    PD_OPT(splitk_tiles, OPT_INT),
    PD_OPT(splitk_max, OPT_INT),
    PD_OPT(splitk_big, OPT_INT),
    PD_OPT(splitk_fused, OPT_BOOL),
    PD_OPT(tile192, OPT_BOOL),
    PD_OPT(gemv, OPT_BOOL),
    PD_OPT(sd3_fp8, OPT_INT, OPT_FX_SD3_FP8),
    PD_OPT(attn_legacy, OPT_BOOL),
    PD_OPT(st_fuse, OPT_BOOL, OPT_FX_LN),
    PD_OPT(ring, OPT_INT),
    PD_OPT(ring_tile, OPT_INT),
    PD_OPT(ring_geglu, OPT_INT),
    PD_OPT(ring_small, OPT_INT),
    PD_OPT(ring_pp, OPT_INT),
    PD_OPT(slab_gn, OPT_INT),
    PD_OPT(ups_fold, OPT_BOOL, OPT_FX_LN),
    PD_OPT(ups_fold_tiles, OPT_INT),
    PD_OPT(vae_flash, OPT_TRI),
    PD_OPT(gemm_tile, OPT_INT, OPT_FX_NONE, [](int64_t v) { return v >= -1 && v <= 4; }, "option gemm_tile: -1 (the plan's own) or a tile 0 .. 4"),
    PD_OPT(gemm_splitk, OPT_INT, OPT_FX_NONE, [](int64_t v) { return v >= -1 && v != 0 && v <= 64; },
           "option gemm_splitk: -1 (the plan's own), 1 (never) or 2 .. 64 slices"),
};
// Switches of pd_set_option / pd_get_option that pd_option_info does not enumerate: the enumerated table above is the documented list of
// tuning knobs; a row here is the A/B switch of one feature, documented with that feature
inline constexpr OptionRow kSwitches[] = {
    PD_OPT(pag_fork, OPT_BOOL),
};
#undef PD_OPT
