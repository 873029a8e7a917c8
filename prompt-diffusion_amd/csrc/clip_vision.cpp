// pdengine: the CLIP image tower (transformers' CLIPVisionModelWithProjection) and the safety checker on top of it -- what the
// reference pipeline's image_encoder / safety_checker / feature_extractor run.
//   encode_image            pipeline_prompt_diffusion.py:490-513   (image_embeds, or hidden_states[-2])
//   run_safety_checker      pipeline_prompt_diffusion.py:514-528   (feature_extractor -> StableDiffusionSafetyChecker)
//   CLIPImageProcessor      resize (shortest edge, PIL BICUBIC) -> centre crop -> / 255 -> normalise
// The module: patch embedding (Conv2d(3, C, p, stride p, bias = False)) as a GEMM over a patch matrix, class row + position embedding,
// pre_layrnorm, the text stack's pre-LN blocks without the causal mask (text.cpp: clip_block), post_layernorm on the class row,
// visual_projection.  The uint8 path writes the patch matrix straight from the resampler (clip_vision.hip): no fp32 picture in between.
#include <algorithm>
#include <cstring>

#include "engine.h"

namespace {

int round_up(int x, int m) { return (x + m - 1) / m * m; }

// get_resize_output_image_size (shortest edge, default_to_square = False) and center_crop of transformers' image_transforms
int prep_geometry(int H, int W, int S, int* Hr, int* Wr, int* top, int* left) {
    if (H < 1 || W < 1 || S < 1) { pd_set_error("clip preprocess: sizes must be >= 1 (%d x %d -> %d)", H, W, S); return 1; }
    const int shorter = std::min(H, W), longer = std::max(H, W);
    const int new_long = (int)((double)S * (double)longer / (double)shorter);
    *Hr = H <= W ? S : new_long;
    *Wr = H <= W ? new_long : S;
    *top = (*Hr - S) / 2;
    *left = (*Wr - S) / 2;
    return 0;
}

// whether pd_clip_preprocess takes H x W pictures at all: sizes, and no axis reduced beyond PD_RESAMPLE_MAX_SCALE (error set otherwise).
// Callers ask before they enqueue anything.
int prep_check(int H, int W, int S) {
    int Hr, Wr, top, left, ks;
    PD_TRY(prep_geometry(H, W, S, &Hr, &Wr, &top, &left));
    std::vector<int32_t> b, k;
    if (Wr != W) PD_TRY(pd_resample_axis(W, Wr, PD_RESAMPLE_BICUBIC, &ks, b, k));
    if (Hr != H) PD_TRY(pd_resample_axis(H, Hr, PD_RESAMPLE_BICUBIC, &ks, b, k));
    return 0;
}

bool dh_known(int dh) { return dh == 8 || dh == 16 || dh == 32 || dh == 40 || dh == 64 || dh == 80 || dh == 160; }

}  // namespace

extern "C" int pd_clip_preprocess_geometry(int32_t H, int32_t W, int32_t image_size, int32_t* Hr, int32_t* Wr, int32_t* top, int32_t* left) {
    if (!Hr || !Wr || !top || !left) { pd_set_error("pd_clip_preprocess_geometry: null argument"); return 1; }
    int a, b, c, d;
    PD_TRY(prep_geometry(H, W, image_size, &a, &b, &c, &d));
    *Hr = a; *Wr = b; *top = c; *left = d;
    return 0;
}

extern "C" int pd_clip_patch_width(int32_t patch) { return patch < 1 ? 0 : round_up(3 * patch * patch, 8); }

int pd_engine::clip_preprocess_dev(const uint8_t* src, int B, int H, int W, int S, int patch, const float* mean, const float* stdv, int mode,
                                   void* dst) {
    int Hr, Wr, top, left;
    PD_TRY(prep_geometry(H, W, S, &Hr, &Wr, &top, &left));
    const bool need_h = Wr != W, need_v = Hr != H;
    // tables of the crop rows / columns only: [bounds_h | kk_h | bounds_v | kk_v]
    int ks_h = 0, ks_v = 0;
    std::vector<int32_t> bh, kh, bv, kv;
    if (need_h) PD_TRY(pd_resample_axis(W, Wr, PD_RESAMPLE_BICUBIC, &ks_h, bh, kh));
    if (need_v) PD_TRY(pd_resample_axis(H, Hr, PD_RESAMPLE_BICUBIC, &ks_v, bv, kv));
    const size_t off_kh = need_h ? (size_t)2 * S : 0, off_bv = off_kh + (size_t)ks_h * (need_h ? S : 0);
    const size_t off_kv = off_bv + (need_v ? (size_t)2 * S : 0), n_tab = off_kv + (size_t)ks_v * (need_v ? S : 0);
    // source rows the vertical pass reads (bounds are monotonic in the output row)
    int r0 = top, Hn = S;
    if (need_v) {
        r0 = bv[2 * top];
        int r1 = 0;
        for (int y = top; y < top + S; ++y) { r0 = std::min(r0, bv[2 * y]); r1 = std::max(r1, bv[2 * y] + bv[2 * y + 1]); }
        Hn = r1 - r0;
    }
    if (arena.dry) return 0;
    if (n_tab) {
        const int32_t key[3] = {H, W, S};
        const bool same = clip_tab.p && key[0] == clip_tab_key[0] && key[1] == clip_tab_key[1] && key[2] == clip_tab_key[2];
        if (!same) {
            HIP_OK(hipStreamSynchronize(stream));   // an earlier upload may still read the host copy
            clip_tab_host.assign(n_tab, 0);
            int32_t* t = clip_tab_host.data();
            if (need_h) {
                memcpy(t, bh.data() + (size_t)2 * left, (size_t)2 * S * sizeof(int32_t));
                memcpy(t + off_kh, kh.data() + (size_t)left * ks_h, (size_t)S * ks_h * sizeof(int32_t));
            }
            if (need_v) {
                memcpy(t + off_bv, bv.data() + (size_t)2 * top, (size_t)2 * S * sizeof(int32_t));
                memcpy(t + off_kv, kv.data() + (size_t)top * ks_v, (size_t)S * ks_v * sizeof(int32_t));
            }
            clip_tab_key[0] = clip_tab_key[1] = clip_tab_key[2] = 0;
            PD_TRY(image_grow(clip_tab, n_tab * sizeof(int32_t)));
            HIP_OK(hipMemcpyAsync(clip_tab.p, t, n_tab * sizeof(int32_t), hipMemcpyHostToDevice, stream));
            for (int i = 0; i < 3; ++i) clip_tab_key[i] = key[i];
        }
    }
    const int32_t* tab = reinterpret_cast<const int32_t*>(clip_tab.p);
    const uint8_t* in = src;
    int Hin = H, Win = W, x_off = left, row_off = need_v ? 0 : top;
    if (need_h) {
        PD_TRY(image_grow(clip_tmp, (size_t)B * Hn * S * 3));
        ++launches;
        if (launch_clipv_hpass(src, reinterpret_cast<uint8_t*>(clip_tmp.p), tab, tab + off_kh, ks_h, B, H, W, r0, Hn, S, stream)) {
            pd_set_error("clip preprocess: horizontal pass launch failed");
            return 1;
        }
        in = reinterpret_cast<const uint8_t*>(clip_tmp.p);
        Hin = Hn; Win = S; x_off = 0; row_off = need_v ? r0 : 0;
    }
    ++launches;
    if (launch_clipv_vpass(in, dst, mode, T, need_v ? tab + off_bv : nullptr, need_v ? tab + off_kv : nullptr, ks_v, B, S, Hin, Win, x_off,
                           row_off, patch, mean, stdv, stream)) {
        pd_set_error("clip preprocess: vertical pass / pack launch failed (%d x %d -> %d, patch %d)", H, W, S, patch);
        return 1;
    }
    return 0;
}

extern "C" int pd_clip_preprocess(pd_engine* e, const pd_clip_preprocess_args* a) {
    if (!e || !a || !a->src || !a->dst) { pd_set_error("pd_clip_preprocess: null argument"); return 1; }
    const int B = a->B, H = a->H, W = a->W, S = a->image_size;
    if (B < 1 || H < 1 || W < 1 || S < 1) { pd_set_error("pd_clip_preprocess: sizes must be >= 1 ([%d, %d, %d, 3] -> %d)", B, H, W, S); return 1; }
    if (a->out_mode != PD_CLIP_OUT_PIXEL_VALUES && a->out_mode != PD_CLIP_OUT_PATCHES && a->out_mode != PD_CLIP_OUT_BYTES) {
        pd_set_error("pd_clip_preprocess: unknown out_mode %d (PD_CLIP_OUT_*)", a->out_mode);
        return 1;
    }
    if (a->out_mode == PD_CLIP_OUT_PATCHES && (a->patch < 1 || S % a->patch)) {
        pd_set_error("pd_clip_preprocess: image_size %d must be a multiple of patch %d", S, a->patch);
        return 1;
    }
    for (int c = 0; c < 3; ++c)
        if (!(a->std[c] > 0.f)) { pd_set_error("pd_clip_preprocess: std[%d] must be > 0", c); return 1; }
    if (e->ses.active) { pd_set_error("pd_clip_preprocess: end the sampling session first"); return 1; }
    PD_TRY(prep_check(H, W, S));   // refuse before anything is enqueued
    HIP_OK(hipSetDevice(e->device));
    const size_t n_src = (size_t)B * H * W * 3;
    size_t n_dst;
    if (a->out_mode == PD_CLIP_OUT_PATCHES) n_dst = (size_t)B * (S / a->patch) * (S / a->patch) * pd_clip_patch_width(a->patch) * dt_size(e->T);
    else if (a->out_mode == PD_CLIP_OUT_BYTES) n_dst = (size_t)B * S * S * 3;
    else n_dst = (size_t)B * 3 * S * S * sizeof(float);
    const uint8_t* src = a->src;
    if (a->mem_src != PD_MEM_DEVICE) {
        PD_TRY(e->image_grow(e->img_u8, n_src));
        HIP_OK(hipMemcpyAsync(e->img_u8.p, a->src, n_src, hipMemcpyHostToDevice, e->stream));
        src = reinterpret_cast<const uint8_t*>(e->img_u8.p);
    }
    void* dst = a->dst;
    if (a->mem_dst != PD_MEM_DEVICE) {
        PD_TRY(e->image_grow(e->clip_out, n_dst));
        dst = e->clip_out.p;
    }
    PD_TRY(e->clip_preprocess_dev(src, B, H, W, S, a->patch, a->mean, a->std, a->out_mode, dst));
    if (a->mem_dst != PD_MEM_DEVICE) HIP_OK(hipMemcpyAsync(a->dst, dst, n_dst, hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    return 0;
}

// ------------------------------------------------------------------------------------------------------------ the tower
ClipVisionW* pd_engine::find_clip_vision(const char* prefix) {
    if (!prefix) return nullptr;
    for (ClipVisionW& v : clip_vision)
        if (v.built && v.prefix == prefix) return &v;
    return nullptr;
}

extern "C" int pd_clip_vision_configure(pd_engine* e, const pd_clip_vision_config* c) {
    if (!e || !c) { pd_set_error("bad argument"); return 1; }
    if (!memchr(c->prefix, 0, sizeof(c->prefix))) { pd_set_error("pd_clip_vision_configure: prefix is not terminated"); return 1; }
    if (ClipVisionW* old = e->find_clip_vision(c->prefix)) {
        if (old->broken) { pd_set_error("pd_clip_vision_configure: the weight allocation of '%s' failed earlier; create a new engine", c->prefix); return 1; }
        return 0;
    }
    int slot = -1;
    for (int i = 0; i < 2 && slot < 0; ++i)
        if (!e->clip_vision[i].built) slot = i;
    auto check = [&]() -> int {
        if (slot < 0) { pd_set_error("pd_clip_vision_configure: both image towers of this engine are taken"); return 1; }
        if (c->layers < 1 || c->heads < 1 || c->hidden < 8 || c->hidden % 8 || c->hidden % c->heads || !dh_known(c->hidden / c->heads) || c->hidden > 2048 ||
            c->ff < 8 || c->ff % 8 || c->patch < 1 || c->image_size < c->patch || c->image_size % c->patch || c->proj_dim < 1 || !(c->eps > 0.f) ||
            (c->act != PD_CLIP_ACT_QUICK_GELU && c->act != PD_CLIP_ACT_GELU)) {
            pd_set_error("pd_clip_vision_configure: need hidden = heads * dh <= 2048 with dh in {8, 16, 32, 40, 64, 80, 160}, hidden and ff multiples of 8, "
                         "image_size a multiple of patch, proj_dim >= 1, eps > 0, a known act");
            return 1;
        }
        for (int k = 0; k < 3; ++k)
            if (!(c->std[k] > 0.f)) { pd_set_error("pd_clip_vision_configure: std[%d] must be > 0", k); return 1; }
        return 0;
    };
    const WeightGroup group = slot == 0 ? GROUP_CLIP_VISION_0 : GROUP_CLIP_VISION_1;
    return e->configure("pd_clip_vision_configure", group, check, [&] {
        ClipVisionW& v = e->clip_vision[slot];
        v.c = *c;
        v.prefix = c->prefix;
        v.group = group;
        const int C = c->hidden, p = c->patch, G = c->image_size / p;
        v.patches = G * G;
        ClipW& t = v.t;
        t.hidden = C; t.ff = c->ff; t.heads = c->heads; t.positions = v.patches + 1; t.proj_dim = c->proj_dim;
        t.act = c->act == PD_CLIP_ACT_GELU ? ACT_ERF_GELU : ACT_QUICK_GELU;
        t.causal = false;
        t.eps = c->eps;
        t.layers.resize(c->layers);
        const std::string V = v.prefix + "vision_model.";
        e->reg_vec(V + "embeddings.class_embedding", C, &v.cls, 'b');
        // Conv2d(3, C, p, stride p) without a bias, as a linear layer over the patch matrix: the flattened [C][3 p p] rows as they are
        e->make_mat(v.patch, C, 3 * p * p, 1, 3 * p * p, false);
        e->reg_mat(V + "embeddings.patch_embedding.weight", {C, 3, p, p}, &v.patch, 0, false);
        e->reg_vec(V + "embeddings.position_embedding.weight", t.positions * C, &v.pos, 'b');
        e->params.back().shape = {t.positions, C};
        e->reg_vec(V + "pre_layrnorm.weight", C, &v.pre_g, 'g');
        e->reg_vec(V + "pre_layrnorm.bias", C, &v.pre_b, 'e');
        e->build_clip_layers(V, t);
        e->reg_vec(V + "post_layernorm.weight", C, &t.fln_g, 'g');
        e->reg_vec(V + "post_layernorm.bias", C, &t.fln_b, 'e');
        // visual_projection sits next to the outermost vision_model: "safety_checker.vision_model." -> "safety_checker.visual_projection.weight"
        std::string outer = v.prefix;
        const std::string tail = "vision_model.";
        if (outer.size() >= tail.size() && outer.compare(outer.size() - tail.size(), tail.size(), tail) == 0) outer.resize(outer.size() - tail.size());
        e->make_mat(t.proj, t.proj_dim, C, 1, C, false);
        e->reg_mat(outer + "visual_projection.weight", {t.proj_dim, C}, &t.proj, 0, false);
        t.built = true;
        v.built = true;
        v.broken = e->alloc_failed;   // the names are registered, so the slot stays taken; every later use of it is refused
    });
}

extern "C" int pd_clip_vision_weights_missing(pd_engine* e, const char* prefix) {
    ClipVisionW* v = e ? e->find_clip_vision(prefix) : nullptr;
    return v ? e->missing((WeightGroup)v->group) : 0;
}

int pd_engine::clip_vision_forward(ClipVisionW& v, const void* patches, int B, int k, float* hid, float* pooled, float* embeds) {
    ClipW& t = v.t;
    const int C = t.hidden, P = v.patches, L = P + 1, n = (int)t.layers.size();
    const size_t mk0 = arena.mark();
    Act pm;
    pm.p = const_cast<void*>(patches); pm.B = B; pm.H = P; pm.W = 1; pm.C = v.patch.cin_pad; pm.dt = T;
    Act po = new_act(B, P, 1, C, DT_F32);
    PD_TRY(gemm(v.patch, pm, po));
    Act e0 = new_act(B, L, 1, C, DT_F32);
    PD_LAUNCH(this, launch_clipv_embed(reinterpret_cast<const float*>(po.p), v.cls, v.pos, reinterpret_cast<float*>(e0.p), B, P, C, stream),
              "CLIP vision embedding launch failed");
    Act x = new_act(B, L, 1, C, v.c.stream_f32 ? (int)DT_F32 : S);   // the residual stream
    PD_TRY(layernorm(e0, x, v.pre_g, v.pre_b, t.eps));
    int done = 0;
    if (hid) {
        PD_TRY(clip_blocks(t, 0, k, x));
        done = k;
        PD_LAUNCH(this, launch_clipv_rows(x.p, x.dt, hid, B, L, C, L, stream), "CLIP vision hidden-state read-out launch failed");
    }
    if (pooled || embeds) {
        PD_TRY(clip_blocks(t, done, n, x));
        // post_layernorm is per row: gather the class rows first
        Act rows = new_act(B, 1, 1, C, DT_F32), lnr = new_act(B, 1, 1, C, DT_F32);
        PD_LAUNCH(this, launch_clipv_rows(x.p, x.dt, reinterpret_cast<float*>(rows.p), B, L, C, 1, stream), "CLIP vision class-row gather launch failed");
        PD_TRY(layernorm(rows, lnr, t.fln_g, t.fln_b, t.eps));
        if (pooled && !arena.dry) HIP_OK(hipMemcpyAsync(pooled, lnr.p, lnr.bytes(), hipMemcpyDeviceToDevice, stream));
        for (int b0 = 0; embeds && b0 < B; b0 += 4)   // launch_gemv streams the weights once per <= 4 rows
            PD_LAUNCH(this, launch_gemv(reinterpret_cast<const float*>(lnr.p) + (size_t)b0 * C, C, t.proj.w, T, t.proj.Kpad, nullptr,
                                        embeds + (size_t)b0 * t.proj_dim, t.proj_dim, std::min(4, B - b0), t.proj_dim, C, 0, stream),
                      "CLIP visual_projection launch failed");
    }
    arena.release(mk0);
    return 0;
}

extern "C" int pd_clip_vision_forward(pd_engine* e, const pd_clip_vision_args* a) {
    if (!e || !a || !a->input || a->B < 1 || (!a->image_embeds && !a->pooler_output && !a->hidden)) { pd_set_error("pd_clip_vision_forward: bad argument"); return 1; }
    ClipVisionW* vp = e->find_clip_vision(a->prefix);
    if (!vp) { pd_set_error("pd_clip_vision_forward: no image tower under '%s' (pd_clip_vision_configure)", a->prefix ? a->prefix : "(null)"); return 1; }
    ClipVisionW& v = *vp;
    if (v.broken) { pd_set_error("pd_clip_vision_forward: the weight allocation of '%s' failed at configure time", a->prefix); return 1; }
    const int B = a->B, S = v.c.image_size, C = v.t.hidden, L = v.patches + 1, D = v.t.proj_dim, n = (int)v.t.layers.size();
    const bool u8 = a->input_kind == PD_CLIP_IN_U8;
    if (!u8 && a->input_kind != PD_CLIP_IN_PIXEL_VALUES) { pd_set_error("pd_clip_vision_forward: unknown input_kind %d (PD_CLIP_IN_*)", a->input_kind); return 1; }
    if (a->H < 1 || a->W < 1 || (!u8 && (a->H != S || a->W != S))) {
        pd_set_error("pd_clip_vision_forward: pixel_values must be [B, 3, %d, %d] (got %d x %d)", S, S, a->H, a->W);
        return 1;
    }
    int k = a->hidden_layer;
    if (a->hidden) {
        if (k < 0) k += n + 1;
        if (k < 0 || k > n) { pd_set_error("pd_clip_vision_forward: hidden_layer %d out of range [-%d, %d]", a->hidden_layer, n + 1, n); return 1; }
    }
    if (e->ses.active) { pd_set_error("pd_clip_vision_forward: end the sampling session first"); return 1; }
    PD_TRY(e->require_loaded((WeightGroup)v.group, "CLIP image tower"));
    if (u8) PD_TRY(prep_check(a->H, a->W, S));   // refuse before anything is enqueued
    HIP_OK(hipSetDevice(e->device));
    const size_t n_in = u8 ? (size_t)B * a->H * a->W * 3 : (size_t)B * 3 * S * S * sizeof(float);   // bytes
    return e->side_call("CLIP vision", [&](SideCall& f) {
        const uint8_t* in;
        PD_TRY(f.src(&in, reinterpret_cast<const uint8_t*>(a->input), n_in, a->mem));
        void* pm = f.scratch<char>((size_t)B * v.patches * v.patch.cin_pad * dt_size(e->T));
        float* dh = a->hidden ? f.dst(a->hidden, (size_t)B * L * C, a->mem) : nullptr;
        float* dp = a->pooler_output ? f.dst(a->pooler_output, (size_t)B * C, a->mem) : nullptr;
        float* de = a->image_embeds ? f.dst(a->image_embeds, (size_t)B * D, a->mem) : nullptr;
        if (!u8) {
            PD_LAUNCH(e, launch_clipv_patchify(reinterpret_cast<const float*>(in), pm, e->T, B, S, v.c.patch, e->stream),
                      "pd_clip_vision_forward: patchify launch failed");
        } else if (!e->arena.dry) {   // (takes nothing from the workspace: its resampling tables are made once, in the real pass)
            PD_TRY(e->check_arena());
            PD_TRY(e->clip_preprocess_dev(in, B, a->H, a->W, S, v.c.patch, v.c.mean, v.c.std, PD_CLIP_OUT_PATCHES, pm));
        }
        return e->clip_vision_forward(v, pm, B, k, dh, dp, de);
    });
}

// ------------------------------------------------------------------------------------------------------------ the checker
extern "C" int pd_safety_configure(pd_engine* e) {
    if (!e) { pd_set_error("bad argument"); return 1; }
    if (e->safety.built) {
        if (e->safety.broken) { pd_set_error("pd_safety_configure: the weight allocation failed earlier; create a new engine"); return 1; }
        return 0;
    }
    ClipVisionW* v = e->find_clip_vision("safety_checker.vision_model.");
    if (!v || v->broken) { pd_set_error("pd_safety_configure: configure the tower under 'safety_checker.vision_model.' first (pd_clip_vision_configure)"); return 1; }
    return e->configure("pd_safety_configure", GROUP_SAFETY, [&] {
        SafetyW& s = e->safety;
        s.D = v->t.proj_dim;
        e->reg_vec("safety_checker.concept_embeds", PD_SAFETY_CONCEPTS * s.D, &s.cpt, 'w');
        e->params.back().shape = {PD_SAFETY_CONCEPTS, s.D};
        e->reg_vec("safety_checker.special_care_embeds", PD_SAFETY_SPECIAL * s.D, &s.spc, 'w');
        e->params.back().shape = {PD_SAFETY_SPECIAL, s.D};
        e->reg_vec("safety_checker.concept_embeds_weights", PD_SAFETY_CONCEPTS, &s.cpt_thr, 'b');
        e->reg_vec("safety_checker.special_care_embeds_weights", PD_SAFETY_SPECIAL, &s.spc_thr, 'b');
        s.built = true;
        s.broken = e->alloc_failed;
    });
}

extern "C" int pd_safety_weights_missing(pd_engine* e) { return e && e->safety.built ? e->missing(GROUP_SAFETY) : 0; }

extern "C" int pd_safety_check(pd_engine* e, const float* embeds, int32_t B, int32_t mem, int32_t* flags, float* scores) {
    if (!e || !embeds || !flags || B < 1) { pd_set_error("pd_safety_check: bad argument"); return 1; }
    if (!e->safety.built || e->safety.broken) { pd_set_error("this engine has no safety checker (pd_safety_configure)"); return 1; }
    PD_TRY(e->require_loaded(GROUP_SAFETY, "safety checker"));
    if (e->ses.active) { pd_set_error("pd_safety_check: end the sampling session first"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    const SafetyW& s = e->safety;
    const int R = PD_SAFETY_SPECIAL + PD_SAFETY_CONCEPTS;
    return e->side_call("safety checker", [&](SideCall& f) {
        const float* src;
        PD_TRY(f.src(&src, embeds, (size_t)B * s.D, mem));
        int* df = f.dst(flags, (size_t)B, mem);
        float* ds = scores ? f.dst(scores, (size_t)B * R, mem) : nullptr;
        PD_LAUNCH(e, launch_safety_check(src, s.spc, s.cpt, s.spc_thr, s.cpt_thr, B, s.D, df, ds, e->stream), "pd_safety_check: launch failed");
        return 0;
    });
}

extern "C" int pd_safety_blank(pd_engine* e, float* images, int32_t B, int64_t per_image, const int32_t* flags, int32_t mem_flags, float value) {
    if (!e || !images || !flags || B < 1 || per_image < 1) { pd_set_error("pd_safety_blank: bad argument"); return 1; }
    if (e->ses.active) { pd_set_error("pd_safety_blank: end the sampling session first"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    const int* df = flags;
    if (mem_flags != PD_MEM_DEVICE) {
        PD_TRY(e->image_grow(e->clip_out, (size_t)B * sizeof(int)));
        HIP_OK(hipMemcpyAsync(e->clip_out.p, flags, (size_t)B * sizeof(int), hipMemcpyHostToDevice, e->stream));
        df = reinterpret_cast<const int*>(e->clip_out.p);
    }
    ++e->launches;
    if (launch_safety_blank(images, df, B, (long long)per_image, value, e->stream)) { pd_set_error("pd_safety_blank: launch failed"); return 1; }
    HIP_OK(hipStreamSynchronize(e->stream));
    return 0;
}
