// pdengine: tiled and sliced VAE calls -- diffusers' AutoencoderKL.enable_tiling / enable_slicing (tiled_decode, tiled_encode, blend_v,
// blend_h), which the reference's pipeline switches on with enable_vae_tiling / enable_vae_slicing (pipeline_prompt_diffusion.py:242-272).
// The grid (vae_make_tile_plan) is diffusers' range(0, h, ov) walk.  Tiles of equal shape form a class and run through the layers of
// vae.cpp as one batch, tile_batch tiles at a time, between the two kernels of vae_tile.hip: the gather cuts the windows out of the
// caller's tensor, the blend assembles the output from the tile results in closed form (include/pdengine.h).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/pdengine_ops.h"
#include "engine.h"

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// ------------------------------------------------------------------------------------ the plan (host only)
int vae_make_tile_plan(int h, int w, int T, double f, int u, bool encode, VaeTilePlan& p) {
    p = VaeTilePlan();
    if (h < 1 || w < 1 || T < 1 || u < 1) { pd_set_error("vae tiling: bad size (h %d, w %d, tile_latent %d, u %d)", h, w, T, u); return 1; }
    if (!(f > 0.0) || f > 1.0 / 3.0) {
        pd_set_error("vae tiling: overlap_factor %g is not supported (0 < f <= 1/3: beyond that a pixel can depend on more than four tiles)", f);
        return 1;
    }
    if (encode && (h % u || w % u)) { pd_set_error("vae tiling: an encode needs H and W multiples of %d (got %d x %d)", u, h, w); return 1; }
    // diffusers' three numbers, in its own arithmetic (Python doubles, int() truncation)
    const int tin = encode ? T * u : T;                      // tile side in input pixels
    const int ov = (int)((double)tin * (1.0 - f));
    const int be = encode ? (int)((double)T * f) : (int)((double)(T * u) * f);
    const int limit = (encode ? T : T * u) - be;
    if (ov < 1 || (encode ? ov != limit * u : ov * u != limit)) {
        pd_set_error("vae tiling: tile_latent %d with overlap_factor %g leaves tiles that do not abut (tile_latent * overlap_factor must be an integer)", T, f);
        return 1;
    }
    if (h <= tin && w <= tin) return 0;   // not tiled
    p.tiled = true;
    p.limit = limit;
    p.be = be;
    p.nrow = (h + ov - 1) / ov;
    p.ncol = (w + ov - 1) / ov;
    auto out_of = [&](int n) { return encode ? n / u : n * u; };
    std::vector<std::pair<int, int>> shapes;
    p.tiles.resize((size_t)p.nrow * p.ncol);
    for (int ti = 0; ti < p.nrow; ++ti)
        for (int tj = 0; tj < p.ncol; ++tj) {
            pd_vae_tile& t = p.tiles[(size_t)ti * p.ncol + tj];
            memset(&t, 0, sizeof(t));
            t.y0 = ti * ov; t.x0 = tj * ov;
            t.h = std::min(tin, h - t.y0); t.w = std::min(tin, w - t.x0);
            t.th = out_of(t.h); t.tw = out_of(t.w);
            t.oy = ti * limit; t.ox = tj * limit;
            t.oh = std::min(limit, t.th); t.ow = std::min(limit, t.tw);
            if (ti > 0) t.ev = std::min({(int)p.tiles[(size_t)(ti - 1) * p.ncol + tj].th, (int)t.th, be});
            if (tj > 0) t.eh = std::min({(int)p.tiles[(size_t)ti * p.ncol + tj - 1].tw, (int)t.tw, be});
            const std::pair<int, int> s(t.h, t.w);
            size_t c = std::find(shapes.begin(), shapes.end(), s) - shapes.begin();
            if (c == shapes.size()) { shapes.push_back(s); p.members.emplace_back(); }
            t.cls = (int32_t)c;
            p.members[c].push_back(ti * p.ncol + tj);
        }
    p.nclass = (int)shapes.size();
    return 0;
}

extern "C" int pd_vae_tile_plan(int32_t h, int32_t w, int32_t tile_latent, double overlap_factor, int32_t u, int32_t encode, int32_t* rows,
                                int32_t* cols, int32_t* classes, pd_vae_tile* tiles, int32_t cap) {
    VaeTilePlan p;
    PD_TRY(vae_make_tile_plan(h, w, tile_latent, overlap_factor, u, encode != 0, p));
    if (rows) *rows = p.nrow;
    if (cols) *cols = p.ncol;
    if (classes) *classes = p.nclass;
    if (tiles) {
        if ((long long)cap < (long long)p.nrow * p.ncol) { pd_set_error("pd_vae_tile_plan: %d x %d tiles, room for %d", p.nrow, p.ncol, cap); return 1; }
        if (!p.tiles.empty()) memcpy(tiles, p.tiles.data(), p.tiles.size() * sizeof(pd_vae_tile));
    }
    return 0;
}

// ------------------------------------------------------------------------------------ state
static const int kDefaultTile[2] = {64, 128};   // diffusers: tile_sample_min_size = config.sample_size (512 / 1024 pixels)
static const double kDefaultOverlap = 0.25;
static const int kDefaultTileBatch = 4;         // the smallest of {1, 4, 16, all} within 3 % of the best at 1024^2 (profiles/vae_tiling_bench.json)

static int vae_u(const pd_engine* e, int which) {
    const VaeW& d = which == PD_VAE_SD3 ? e->sd3_vae : e->vae;
    const VaeEncW& n = which == PD_VAE_SD3 ? e->sd3_vae_enc : e->vae_enc;
    const int levels = d.built ? d.d.num_levels : n.built ? n.d.num_levels : 4;
    return 1 << (levels - 1);
}

extern "C" int pd_vae_set_tiling(pd_engine* e, int32_t which, int32_t on, int32_t tile_latent, double overlap_factor, int32_t tile_batch) {
    if (!e || (which != PD_VAE_SD15 && which != PD_VAE_SD3)) { pd_set_error("pd_vae_set_tiling: bad argument (which: PD_VAE_SD15 / PD_VAE_SD3)"); return 1; }
    if (tile_latent < 0 || tile_batch < 0 || !std::isfinite(overlap_factor) || overlap_factor < 0.0) {
        pd_set_error("pd_vae_set_tiling: tile_latent, overlap_factor and tile_batch must be >= 0 (0: the default)");
        return 1;
    }
    pd_engine::VaeTiling s = e->vae_tiling[which];
    s.tiling = on != 0;
    // switching on replaces the parameters (0: back to the default); switching off keeps whatever a 0 stands for
    if (on || tile_latent) s.tile = tile_latent;
    if (on || overlap_factor != 0.0) s.overlap = overlap_factor;
    if (on || tile_batch) s.batch = tile_batch;
    // both directions must be plannable: a size that needs no tiling runs the parameter checks only
    const int T = s.tile ? s.tile : kDefaultTile[which], u = vae_u(e, which);
    const double f = s.overlap != 0.0 ? s.overlap : kDefaultOverlap;
    VaeTilePlan p;
    PD_TRY(vae_make_tile_plan(1, 1, T, f, u, false, p));
    PD_TRY(vae_make_tile_plan(u, u, T, f, u, true, p));
    e->vae_tiling[which] = s;
    return 0;
}

extern "C" int pd_vae_set_slicing(pd_engine* e, int32_t which, int32_t on) {
    if (!e || (which != PD_VAE_SD15 && which != PD_VAE_SD3)) { pd_set_error("pd_vae_set_slicing: bad argument (which: PD_VAE_SD15 / PD_VAE_SD3)"); return 1; }
    e->vae_tiling[which].slicing = on != 0;
    return 0;
}

extern "C" int pd_vae_get_tiling(pd_engine* e, int32_t which, int32_t* tiling, int32_t* slicing, int32_t* tile_latent, double* overlap_factor,
                                 int32_t* tile_batch) {
    if (!e || (which != PD_VAE_SD15 && which != PD_VAE_SD3)) { pd_set_error("pd_vae_get_tiling: bad argument (which: PD_VAE_SD15 / PD_VAE_SD3)"); return 1; }
    const pd_engine::VaeTiling& s = e->vae_tiling[which];
    if (tiling) *tiling = s.tiling;
    if (slicing) *slicing = s.slicing;
    if (tile_latent) *tile_latent = s.tile ? s.tile : kDefaultTile[which];
    if (overlap_factor) *overlap_factor = s.overlap != 0.0 ? s.overlap : kDefaultOverlap;
    if (tile_batch) *tile_batch = s.batch ? s.batch : kDefaultTileBatch;
    return 0;
}

VaeTilePlan pd_engine::vae_plan_for(int which, int h, int w, int u, bool encode) const {
    VaeTilePlan p;
    const VaeTiling& s = vae_tiling[which];
    if (!s.tiling) return p;
    if (vae_make_tile_plan(h, w, s.tile ? s.tile : kDefaultTile[which], s.overlap != 0.0 ? s.overlap : kDefaultOverlap, u, encode, p)) p = VaeTilePlan();
    return p;
}

// A tile whose token count is no multiple of 8 cannot materialise its attention scores: it needs the flash kernel
int pd_engine::vae_check_tiles(const VaeTilePlan& p, const VaeDesc& d, int C, const char* who) const {
    const int dn = 1 << (d.num_levels - 1);
    for (const pd_vae_tile& t : p.tiles) {
        const int lh = std::min<int>(t.h, t.th), lw = std::min<int>(t.w, t.tw);   // the tile at latent resolution, either direction
        if ((lh * lw) % 8 == 0) continue;
        if (!f32 && vae_attention_eligible(T, C) && opt.vae_flash != 0) continue;
        pd_set_error("%s: tile at (%d, %d) is %d x %d latent pixels, no multiple of 8 tokens; its mid-block attention needs the flash kernel, "
                     "which this engine does not run (fp32 storage, option \"vae_flash\" 0 or %d channels); choose a size or tile_latent "
                     "that leaves an even remainder", who, t.y0 / (t.h > t.th ? dn : 1), t.x0 / (t.h > t.th ? dn : 1), lh, lw, C);
        return 1;
    }
    return 0;
}

// ------------------------------------------------------------------------------------ one run
// Tile results and the device tables on the workspace stack; in a dry pass only the sizes count
int pd_engine::vae_tile_setup(const VaeTilePlan& p, int B, int cpad, VaeTileRun& run) {
    const int nt = p.nrow * p.ncol;
    run.res.resize(p.nclass);
    run.origin_at.resize(p.nclass);
    std::vector<long long> class_off(p.nclass);
    for (int c = 0; c < p.nclass; ++c) {
        const pd_vae_tile& t = p.tiles[p.members[c][0]];
        run.res[c] = reinterpret_cast<float*>(arena.alloc(p.members[c].size() * (size_t)B * t.th * t.tw * cpad * sizeof(float)));
        class_off[c] = run.res[c] - run.res[0];
    }
    // distinct extents -> weight tables (1 - y / e, then y / e), computed in double like Python's and rounded once
    std::vector<int> ext, ext_off;
    std::vector<float> wtab;
    auto table_of = [&](int e) {
        if (e <= 0) return 0;
        for (size_t i = 0; i < ext.size(); ++i) if (ext[i] == e) return ext_off[i];
        ext.push_back(e);
        ext_off.push_back((int)wtab.size());
        for (int y = 0; y < e; ++y) wtab.push_back((float)(1.0 - (double)y / (double)e));
        for (int y = 0; y < e; ++y) wtab.push_back((float)((double)y / (double)e));
        return ext_off.back();
    };
    std::vector<int> rows(4 * p.nrow, 0), cols(4 * p.ncol, 0), origins(2 * nt);
    std::vector<long long> off(nt);
    for (int ti = 0; ti < p.nrow; ++ti) {
        const pd_vae_tile& t = p.tiles[(size_t)ti * p.ncol];
        rows[4 * ti] = t.th; rows[4 * ti + 1] = t.ev; rows[4 * ti + 2] = table_of(t.ev);
    }
    for (int tj = 0; tj < p.ncol; ++tj) {
        const pd_vae_tile& t = p.tiles[tj];
        cols[4 * tj] = t.tw; cols[4 * tj + 1] = t.eh; cols[4 * tj + 2] = table_of(t.eh);
    }
    int at = 0;
    for (int c = 0; c < p.nclass; ++c) {
        run.origin_at[c] = at;
        for (size_t k = 0; k < p.members[c].size(); ++k, ++at) {
            const pd_vae_tile& t = p.tiles[p.members[c][k]];
            origins[2 * at] = t.y0; origins[2 * at + 1] = t.x0;
            off[p.members[c][k]] = class_off[c] + (long long)k * B * t.th * t.tw * cpad;
        }
    }
    if (wtab.empty()) wtab.push_back(0.f);
    const size_t b_off = off.size() * sizeof(long long), b_rows = rows.size() * sizeof(int), b_cols = cols.size() * sizeof(int),
                 b_org = origins.size() * sizeof(int), b_w = wtab.size() * sizeof(float);
    const size_t o_rows = round_up((int)b_off, 16), o_cols = o_rows + round_up((int)b_rows, 16), o_org = o_cols + round_up((int)b_cols, 16),
                 o_w = o_org + round_up((int)b_org, 16), total = o_w + b_w;
    char* dev = reinterpret_cast<char*>(arena.alloc(total));
    run.tile_off = reinterpret_cast<long long*>(dev);
    run.rows = reinterpret_cast<int*>(dev + o_rows);
    run.cols = reinterpret_cast<int*>(dev + o_cols);
    run.origins = reinterpret_cast<int*>(dev + o_org);
    run.wtab = reinterpret_cast<float*>(dev + o_w);
    if (arena.dry) return 0;
    PD_TRY(check_arena());
    vae_tile_blob.assign(total, 0);
    memcpy(vae_tile_blob.data(), off.data(), b_off);
    memcpy(vae_tile_blob.data() + o_rows, rows.data(), b_rows);
    memcpy(vae_tile_blob.data() + o_cols, cols.data(), b_cols);
    memcpy(vae_tile_blob.data() + o_org, origins.data(), b_org);
    memcpy(vae_tile_blob.data() + o_w, wtab.data(), b_w);
    // (pageable memory: the blob stays alive and unchanged until the call's own final stream synchronisation)
    if (hipMemcpyAsync(dev, vae_tile_blob.data(), total, hipMemcpyHostToDevice, stream) != hipSuccess) { pd_set_error("vae tiling: table upload failed"); return 1; }
    return 0;
}

int pd_engine::vae_tile_blend(const VaeTilePlan& p, const VaeTileRun& run, int B, int C, int cpad, bool nchw, float* out) {
    const pd_vae_tile& last = p.tiles.back();
    VaeBlendParams bp{};
    bp.tiles = run.res[0]; bp.tile_off = run.tile_off; bp.rows = run.rows; bp.cols = run.cols; bp.wtab = run.wtab; bp.out = out;
    bp.B = B; bp.C = C; bp.Cpad = cpad; bp.H = last.oy + last.oh; bp.W = last.ox + last.ow;
    bp.nrow = p.nrow; bp.ncol = p.ncol; bp.limit = p.limit; bp.nchw = nchw ? 1 : 0;
    PD_LAUNCH(this, launch_vae_tile_blend(bp, stream), "vae tiling: blend launch failed");
    return 0;
}

// decode of B samples, sliced and / or tiled as the state says; src / dout NULL in the dry pass
int pd_engine::vae_decode_managed(VaeW& v, int which, const float* src, int B, int h, int w, float* dout, float scale, float shift) {
    const VaeDesc& d = v.d;
    const VaeTiling& st = vae_tiling[which];
    const int u = 1 << (d.num_levels - 1), cpad = round_up(d.out_ch, 4);
    const int Bs = st.slicing ? 1 : B;
    const VaeTilePlan p = vae_plan_for(which, h, w, u, false);
    if (!p.tiled && Bs == B) return vae_forward(v, src, B, h, w, dout, scale, shift);
    VaeTileRun run;
    if (p.tiled) {
        PD_TRY(vae_check_tiles(p, d, v.attn.C, which == PD_VAE_SD3 ? "pd_sd3_vae_decode" : "pd_vae_decode"));
        PD_TRY(vae_tile_setup(p, Bs, cpad, run));
    }
    const int tb = st.batch ? st.batch : kDefaultTileBatch;
    const size_t n_in = (size_t)Bs * d.z * h * w, n_out = (size_t)Bs * d.out_ch * h * u * w * u;
    for (int s = 0; s < B / Bs; ++s) {
        const float* in = src ? src + s * n_in : nullptr;
        float* out = dout ? dout + s * n_out : nullptr;
        const size_t mk = arena.mark();
        if (!p.tiled) {
            PD_TRY(vae_forward(v, in, Bs, h, w, out, scale, shift));
        } else {
            vae_tile_odd_flash = true;
            int r = 0;
            for (int c = 0; c < p.nclass && !r; ++c) {
                const pd_vae_tile& t = p.tiles[p.members[c][0]];
                const int n = (int)p.members[c].size();
                const size_t tile_elems = (size_t)Bs * t.th * t.tw * cpad;
                for (int k0 = 0; k0 < n && !r; k0 += tb) {
                    const int g = std::min(tb, n - k0);
                    const size_t mk2 = arena.mark();
                    Act z = new_act(g * Bs, t.h, t.w, d.zpad, T);
                    if (!arena.dry) {
                        r = check_arena();
                        ++launches;
                        vae_tiles_run += g;
                        if (!r && launch_vae_tile_gather(in, z.p, T, run.origins + 2 * (run.origin_at[c] + k0), g, Bs, d.z, h, w, t.h, t.w, d.zpad, scale,
                                                         shift, stream)) { pd_set_error("vae tiling: gather launch failed"); r = 1; }
                    }
                    Act img;
                    img.p = run.res[c] + (size_t)k0 * tile_elems; img.B = g * Bs; img.H = t.th; img.W = t.tw; img.C = cpad; img.dt = DT_F32;
                    if (!r) r = vae_decode_layers(v, z, img);
                    arena.release(mk2);
                }
            }
            vae_tile_odd_flash = false;
            if (r) return r;
            PD_TRY(vae_tile_blend(p, run, Bs, d.out_ch, cpad, true, out));
        }
        arena.release(mk);
    }
    return 0;
}

// encode: the moments of every slice / tile land in one [B][h][w][cpad] buffer, the posterior is taken once from it
int pd_engine::vae_encode_managed(VaeEncW& v, int which, const float* src, int B, int H, int W, int what, const float* noise, float* dout,
                                  float scale, float shift) {
    const VaeDesc& d = v.d;
    const VaeTiling& st = vae_tiling[which];
    const int u = 1 << (d.num_levels - 1), cpad = d.quant ? v.quant.m.N : v.conv_out.m.N, cin_pad = v.conv_in.m.cin_pad;
    const int Bs = st.slicing ? 1 : B;
    const VaeTilePlan p = vae_plan_for(which, H, W, u, true);
    if (!p.tiled && Bs == B) return vae_encoder_forward(v, src, B, H, W, what, noise, dout, scale, shift);
    const int h = H / u, w = W / u;
    VaeTileRun run;
    Act mom = new_act(B, h, w, cpad, DT_F32);
    if (p.tiled) {
        PD_TRY(vae_check_tiles(p, d, v.attn.C, which == PD_VAE_SD3 ? "pd_sd3_vae_encode" : "pd_vae_encode"));
        PD_TRY(vae_tile_setup(p, Bs, cpad, run));
    }
    const int tb = st.batch ? st.batch : kDefaultTileBatch;
    const size_t n_in = (size_t)Bs * d.out_ch * H * W, n_mom = (size_t)Bs * h * w * cpad;
    for (int s = 0; s < B / Bs; ++s) {
        const float* in = src ? src + s * n_in : nullptr;
        Act ms = mom;
        ms.B = Bs;
        ms.p = reinterpret_cast<float*>(mom.p) + s * n_mom;
        const size_t mk = arena.mark();
        if (!p.tiled) {
            Act x = new_act(Bs, H, W, cin_pad, T);
            PD_LAUNCH(this, launch_nchw_to_nhwc(in, x.p, T, Bs, d.out_ch, H, W, x.C, stream), "image upload launch failed");
            PD_TRY(vae_encode_layers(v, x, ms));
        } else {
            vae_tile_odd_flash = true;
            int r = 0;
            for (int c = 0; c < p.nclass && !r; ++c) {
                const pd_vae_tile& t = p.tiles[p.members[c][0]];
                const int n = (int)p.members[c].size();
                const size_t tile_elems = (size_t)Bs * t.th * t.tw * cpad;
                for (int k0 = 0; k0 < n && !r; k0 += tb) {
                    const int g = std::min(tb, n - k0);
                    const size_t mk2 = arena.mark();
                    Act x = new_act(g * Bs, t.h, t.w, cin_pad, T);
                    if (!arena.dry) {
                        r = check_arena();
                        ++launches;
                        vae_tiles_run += g;
                        if (!r && launch_vae_tile_gather(in, x.p, T, run.origins + 2 * (run.origin_at[c] + k0), g, Bs, d.out_ch, H, W, t.h, t.w, cin_pad,
                                                         1.f, 0.f, stream)) { pd_set_error("vae tiling: gather launch failed"); r = 1; }
                    }
                    Act tm;
                    tm.p = run.res[c] + (size_t)k0 * tile_elems; tm.B = g * Bs; tm.H = t.th; tm.W = t.tw; tm.C = cpad; tm.dt = DT_F32;
                    if (!r) r = vae_encode_layers(v, x, tm);
                    arena.release(mk2);
                }
            }
            vae_tile_odd_flash = false;
            if (r) return r;
            PD_TRY(vae_tile_blend(p, run, Bs, cpad, cpad, false, reinterpret_cast<float*>(ms.p)));
        }
        arena.release(mk);
    }
    PD_LAUNCH(this, launch_vae_posterior(mom.p, DT_F32, mom.C, noise, dout, B, d.z, h * w, what, scale, stream, rng_dev, shift), "posterior launch failed");
    return 0;
}

// ------------------------------------------------------------------------------------ test hook
extern "C" int pd_op_vae_tile_blend(pd_engine* e, const float* tiles, const pd_vae_tile* plan, int rows, int cols, int B, int C, int Cpad, int nchw,
                                    float* out) {
    if (!e || !tiles || !plan || !out || rows < 1 || cols < 1 || B < 1 || C < 1 || Cpad < C || Cpad % 4) { pd_set_error("pd_op_vae_tile_blend: bad argument"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    // the kernel trusts its tables: check what it will index with
    VaeTilePlan p;
    p.tiled = true; p.nrow = rows; p.ncol = cols; p.nclass = rows * cols;
    p.tiles.assign(plan, plan + (size_t)rows * cols);
    p.limit = plan[0].oh > plan[0].ow ? plan[0].oh : plan[0].ow;
    for (int ti = 0; ti < rows; ++ti)
        for (int tj = 0; tj < cols; ++tj) {
            const pd_vae_tile& t = p.tiles[(size_t)ti * cols + tj];
            const pd_vae_tile& r0 = p.tiles[(size_t)ti * cols];
            const pd_vae_tile& c0 = p.tiles[tj];
            bool ok = t.th >= 1 && t.tw >= 1 && t.th == r0.th && t.tw == c0.tw && t.ev == r0.ev && t.eh == c0.eh && t.oh >= 1 && t.ow >= 1 &&
                      t.oh <= t.th && t.ow <= t.tw && t.oh <= p.limit && t.ow <= p.limit && t.oy == ti * p.limit && t.ox == tj * p.limit &&
                      (ti == rows - 1 || t.oh == p.limit) && (tj == cols - 1 || t.ow == p.limit) && t.ev >= 0 && t.eh >= 0 && t.ev <= t.th &&
                      t.eh <= t.tw;
            if (ok && ti > 0) ok = t.ev <= p.tiles[(size_t)(ti - 1) * cols + tj].th;
            if (ok && tj > 0) ok = t.eh <= p.tiles[(size_t)ti * cols + tj - 1].tw;
            if (ok && ti == 0) ok = t.ev == 0;
            if (ok && tj == 0) ok = t.eh == 0;
            if (!ok) { pd_set_error("pd_op_vae_tile_blend: tile (%d, %d) of the plan is inconsistent", ti, tj); return 1; }
            p.members.push_back({ti * cols + tj});
        }
    const pd_vae_tile& last = p.tiles.back();
    const int H = last.oy + last.oh, W = last.ox + last.ow;
    const size_t n_out = (size_t)B * (nchw ? C : Cpad) * H * W;
    return e->side_call("VAE", [&](SideCall& f) {
        VaeTileRun run;
        PD_TRY(e->vae_tile_setup(p, B, Cpad, run));   // one class per tile, in plan order: the caller's layout
        const float* src = tiles;
        for (int c = 0; c < p.nclass; ++c) {
            const size_t n = (size_t)B * p.tiles[c].th * p.tiles[c].tw * Cpad;
            PD_TRY(f.upload(run.res[c], src, n * sizeof(float)));
            src += n;
        }
        return e->vae_tile_blend(p, run, B, C, Cpad, nchw != 0, f.dst(out, n_out, PD_MEM_HOST));
    });
}
