// pdengine: the SD3 text encoders -- what the reference's encode_prompt runs around its tokenizers.
//   _get_clip_prompt_embeds   promptdiffusioncontrolnetpipeline_sd3.py:295-348  (the CLIP stack of text.cpp, twice: CLIP-L, CLIP-G)
//   _get_t5_prompt_embeds     promptdiffusioncontrolnetpipeline_sd3.py:238-292  (T5EncoderModel(ids)[0], no attention mask)
//   encode_prompt             promptdiffusioncontrolnetpipeline_sd3.py:457-471  (cat / pad / cat: written in place here, no host concat)
// T5: token embedding without positions, pre-RMSNorm blocks, softmax(Q K^T + bias) V with scale 1 (text.cpp's self_attention with the
// Toeplitz bias rows of attention.hip's BIAS instantiation: block 0's table, shared by all blocks), feed-forward
// wo(gelu_new(wi_0 x) * wi_1 x) in one gated GEMM epilogue.
#include "engine.h"

namespace {
constexpr int kClipLen = 77;
}  // namespace

void pd_engine::build_sd3_t5(const std::string& prefix) {
    Sd3T5W& t = sd3_t5;
    const pd_sd3_t5_config& c = t.c;
    const int D = c.d_model, I = c.heads * c.d_kv, F = c.d_ff;
    make_mat(t.tok, c.vocab, D, 1, D, false);
    reg_mat(prefix + "shared.weight", {c.vocab, D}, &t.tok, 0, false);
    t.layers.resize(c.layers);
    for (int i = 0; i < c.layers; ++i) {
        T5LayerW& l = t.layers[i];
        const std::string Bp = prefix + "encoder.block." + std::to_string(i) + ".";
        make_mat(l.qkv, 3 * I, D, 1, D, false);   // rows [0,I) q, [I,2I) k, [2I,3I) v; no biases in T5
        const char* nm[3] = {"q", "k", "v"};
        for (int j = 0; j < 3; ++j) reg_mat(Bp + "layer.0.SelfAttention." + nm[j] + ".weight", {I, D}, &l.qkv, j * I, false);
        make_mat(l.o, D, I, 1, I, false);
        reg_mat(Bp + "layer.0.SelfAttention.o.weight", {D, I}, &l.o, 0, false);
        if (i == 0) {
            make_mat(t.relbias, c.num_buckets, c.heads, 1, c.heads, false);
            reg_mat(Bp + "layer.0.SelfAttention.relative_attention_bias.weight", {c.num_buckets, c.heads}, &t.relbias, 0, false);
        }
        reg_vec(Bp + "layer.0.layer_norm.weight", D, &l.ln1, 'g');
        // wi_0 (through gelu_new) is the gate half, wi_1 the linear half of one GEGLU-packed matrix (gemm.hip, ACT_GATED_TANH_GELU)
        make_mat(l.wi, 2 * F, D, 1, D, false, true);
        reg_mat(Bp + "layer.1.DenseReluDense.wi_0.weight", {F, D}, &l.wi, F, false);
        reg_mat(Bp + "layer.1.DenseReluDense.wi_1.weight", {F, D}, &l.wi, 0, false);
        make_mat(l.wo, D, F, 1, F, false);
        reg_mat(Bp + "layer.1.DenseReluDense.wo.weight", {D, F}, &l.wo, 0, false);
        reg_vec(Bp + "layer.1.layer_norm.weight", D, &l.ln2, 'g');
    }
    reg_vec(prefix + "encoder.final_layer_norm.weight", D, &t.fln, 'g');
    t.built = true;
}

extern "C" int pd_sd3_text_configure(pd_engine* e, const pd_sd3_text_config* c) {
    if (!e || !c) { pd_set_error("bad argument"); return 1; }
    if (e->sd3_clip[0].built || e->sd3_clip[1].built || e->sd3_t5.built) { pd_set_error("pd_sd3_text_configure: already configured"); return 1; }
    const pd_sd3_clip_config* cl[2] = {&c->clip_l, &c->clip_g};
    const pd_sd3_t5_config& t = c->t5;
    auto check = [&]() -> int {
        int clip_width = 0;
        for (int i = 0; i < 2; ++i) {
            const pd_sd3_clip_config& k = *cl[i];
            if (k.layers == 0) continue;
            if (k.layers < 0 || k.vocab < 1 || k.hidden < 64 || k.heads < 1 || k.hidden != 64 * k.heads || k.ff < 8 || k.ff % 8 || k.max_positions != kClipLen ||
                k.proj_dim < 1 || k.hidden > 2048 || (k.act != PD_CLIP_ACT_QUICK_GELU && k.act != PD_CLIP_ACT_GELU)) {
                pd_set_error("pd_sd3_text_configure: CLIP slot %d: need hidden = 64 * heads <= 2048, ff a multiple of 8, max_positions 77, proj_dim >= 1, a known act", i);
                return 1;
            }
            clip_width += k.hidden;
        }
        if (t.layers != 0) {
            if (t.layers < 0 || t.vocab < 1 || t.d_kv != 64 || t.heads < 1 || t.d_model < 8 || t.d_model % 8 || t.d_ff < 8 || t.d_ff % 8 || t.num_buckets < 4 ||
                t.num_buckets % 2 || t.max_distance <= t.num_buckets / 4 || !(t.eps > 0.f)) {
                pd_set_error("pd_sd3_text_configure: T5: need d_kv 64, d_model and d_ff multiples of 8, an even num_buckets >= 4, max_distance > num_buckets / 4, eps > 0");
                return 1;
            }
            if (c->joint_dim != t.d_model) { pd_set_error("pd_sd3_text_configure: joint_dim %d must equal T5's d_model %d (the reference concatenates them row-wise)", c->joint_dim, t.d_model); return 1; }
        }
        if (c->joint_dim < clip_width || c->joint_dim % 4) { pd_set_error("pd_sd3_text_configure: joint_dim %d must be a multiple of 4 and hold both CLIP hidden states (%d)", c->joint_dim, clip_width); return 1; }
        return 0;
    };
    return e->configure("pd_sd3_text_configure", GROUP_SD3_TEXT, check, [&] {
        e->sd3_text_joint = c->joint_dim;
        const std::string prefix[2] = {"text_encoder.", "text_encoder_2."};
        for (int i = 0; i < 2; ++i) {
            const pd_sd3_clip_config& k = *cl[i];
            if (k.layers == 0) continue;
            ClipW& w = e->sd3_clip[i];
            w.vocab = k.vocab; w.hidden = k.hidden; w.ff = k.ff; w.heads = k.heads; w.positions = k.max_positions;
            w.proj_dim = k.proj_dim; w.eos_token_id = k.eos_token_id;
            w.act = k.act == PD_CLIP_ACT_GELU ? ACT_ERF_GELU : ACT_QUICK_GELU;
            w.layers.resize(k.layers);
            e->build_clip(prefix[i] + "text_model.", w);
            e->make_mat(w.proj, w.proj_dim, w.hidden, 1, w.hidden, false);
            e->reg_mat(prefix[i] + "text_projection.weight", {w.proj_dim, w.hidden}, &w.proj, 0, false);
        }
        if (t.layers > 0) { e->sd3_t5.c = t; e->build_sd3_t5("text_encoder_3."); }
    });
}

extern "C" int pd_sd3_text_weights_missing(pd_engine* e) { return e ? e->missing(GROUP_SD3_TEXT) : 0; }

int pd_engine::rmsnorm(const Act& x, void* y, int y_dt, const float* w, float eps, int y_sample_rows, int y_row_off, int y_ld) {
    PD_LAUNCH(this, x.dt != DT_F32 || launch_rmsnorm_rows(reinterpret_cast<const float*>(x.p), y, y_dt, w, x.rows(), x.C, eps, x.H * x.W, y_sample_rows,
                                                          y_row_off, y_ld ? y_ld : x.C, stream),
              "rmsnorm launch failed (C=%d)", x.C);
    return 0;
}

int pd_engine::t5_block(const T5LayerW& l, Act& x, const float* relbias) {
    const pd_sd3_t5_config& c = sd3_t5.c;
    const int B = x.B, L = x.H, D = x.C;
    const size_t mk = arena.mark();
    Act ln = new_act(B, L, 1, D, T), att;
    PD_TRY(rmsnorm(x, ln.p, T, l.ln1, c.eps));
    PD_TRY(self_attention(l.qkv, ln, c.heads * c.d_kv, c.heads, /*causal=*/false, relbias, /*scale=*/1.0f, att));
    Act h1 = new_act(B, L, 1, D, DT_F32);
    PD_TRY(gemm(l.o, att, h1, {.R = &x}));
    PD_TRY(rmsnorm(h1, ln.p, T, l.ln2, c.eps));
    Act f = new_act(B, L, 1, c.d_ff, T);
    PD_TRY(gemm(l.wi, ln, f, {.act = ACT_GATED_TANH_GELU}));
    Act h2 = new_act(B, L, 1, D, DT_F32);
    PD_TRY(gemm(l.wo, f, h2, {.R = &h1}));
    if (!arena.dry) HIP_OK(hipMemcpyAsync(x.p, h2.p, x.bytes(), hipMemcpyDeviceToDevice, stream));
    arena.release(mk);
    return 0;
}

int pd_engine::sd3_t5_forward(const int* ids_dev, int B, int Lt, float* out, int out_rows, int row_off) {
    Sd3T5W& t = sd3_t5;
    const pd_sd3_t5_config& c = t.c;
    const int D = c.d_model, H = c.heads, L = Lt;
    const size_t mk0 = arena.mark();
    // the bias rows of this call: relbias[h][key - query + L - 1] (130 KB at XXL, L = 256), instead of [H, L, L] re-read by every block
    const int nrel = 2 * L - 1;
    int* bucket_dev = reinterpret_cast<int*>(arena.alloc((size_t)nrel * sizeof(int)));
    float* relbias = reinterpret_cast<float*>(arena.alloc((size_t)H * nrel * sizeof(float)));
    Act x = new_act(B, L, 1, D, DT_F32);
    if (!arena.dry) {
        PD_TRY(check_arena());
        HIP_OK(hipStreamSynchronize(stream));   // an earlier call's upload may still read the host table
        t5_bucket_host.resize(nrel);
        PD_TRY(pd_t5_relative_buckets(L, c.num_buckets, c.max_distance, t5_bucket_host.data()));
        HIP_OK(hipMemcpyAsync(bucket_dev, t5_bucket_host.data(), (size_t)nrel * sizeof(int), hipMemcpyHostToDevice, stream));
        launches += 2;
        if (launch_t5_relbias(bucket_dev, t.relbias.w, t.relbias.Kpad, T, relbias, H, nrel, stream) ||
            launch_embed_rows(ids_dev, t.tok.w, t.tok.Kpad, T, reinterpret_cast<float*>(x.p), (long long)B * L, D, c.vocab, stream)) {
            pd_set_error("T5 embedding / bias launch failed");
            return 1;
        }
    }
    for (const T5LayerW& l : t.layers) PD_TRY(t5_block(l, x, relbias));
    PD_TRY(rmsnorm(x, out, DT_F32, t.fln, c.eps, out_rows, row_off, D));
    arena.release(mk0);
    return 0;
}

namespace {
int text_ready(pd_engine* e, const char* who) {
    if (e->ses.active) { pd_set_error("%s: end the sampling session first", who); return 1; }
    return e->require_loaded(GROUP_SD3_TEXT, "SD3 text-encoder");
}
}  // namespace

extern "C" int pd_sd3_encode_prompt(pd_engine* e, const pd_sd3_text_args* a, float* prompt_embeds, float* pooled) {
    if (!e || !a || !prompt_embeds || !pooled) { pd_set_error("pd_sd3_encode_prompt: bad argument"); return 1; }
    if (!e->sd3_clip[0].built || !e->sd3_clip[1].built) {
        pd_set_error("pd_sd3_encode_prompt: this engine has no SD3 text encoders (pd_sd3_text_configure with both CLIP slots)");
        return 1;
    }
    const bool t5 = e->sd3_t5.built;
    if (a->batch < 1 || a->clip_skip < 0 || !a->ids_clip_l || !a->ids_clip_g || (t5 && (!a->ids_t5 || a->t5_len < 1 || a->t5_len > 512))) {
        pd_set_error("pd_sd3_encode_prompt: need batch >= 1, clip_skip >= 0, both CLIP id arrays%s", t5 ? ", T5 ids with t5_len in [1, 512]" : "");
        return 1;
    }
    for (int i = 0; i < 2; ++i)
        if (a->clip_skip > (int)e->sd3_clip[i].layers.size() - 1) { pd_set_error("pd_sd3_encode_prompt: clip_skip %d out of range [0, %d]", a->clip_skip, (int)e->sd3_clip[i].layers.size() - 1); return 1; }
    PD_TRY(text_ready(e, "pd_sd3_encode_prompt"));
    HIP_OK(hipSetDevice(e->device));
    const int B = a->batch, Lt = t5 ? a->t5_len : 0, J = e->sd3_text_joint, rows = kClipLen + Lt;
    const int Cl = e->sd3_clip[0].hidden, Pl = e->sd3_clip[0].proj_dim, Pg = e->sd3_clip[1].proj_dim;
    const size_t n_pe = (size_t)B * rows * J, n_po = (size_t)B * (Pl + Pg);
    return e->side_call("SD3 text", [&](SideCall& f) {
        const int *il, *ig, *it = nullptr;
        PD_TRY(f.src(&il, a->ids_clip_l, (size_t)B * kClipLen, a->mem));
        PD_TRY(f.src(&ig, a->ids_clip_g, (size_t)B * kClipLen, a->mem));
        if (t5) PD_TRY(f.src(&it, a->ids_t5, (size_t)B * Lt, a->mem));
        float* dpe = f.dst(prompt_embeds, n_pe, a->mem);
        float* dpo = f.dst(pooled, n_po, a->mem);
        // rows 0..76: CLIP-L | CLIP-G | zeros up to joint_dim (the second write carries the pad); rows 77..: T5
        PD_TRY(e->sd3_clip_forward(e->sd3_clip[0], il, B, a->clip_skip, dpe, rows, J, 0, Cl, dpo, Pl + Pg));
        PD_TRY(e->sd3_clip_forward(e->sd3_clip[1], ig, B, a->clip_skip, dpe, rows, J, Cl, J - Cl, dpo + Pl, Pl + Pg));
        if (t5) PD_TRY(e->sd3_t5_forward(it, B, Lt, dpe, rows, kClipLen));
        return 0;
    });
}

extern "C" int pd_sd3_text_encoder(pd_engine* e, int32_t which, const int32_t* ids, int32_t B, int32_t len, int32_t clip_skip, int32_t mem,
                                   float* hidden, float* pooled) {
    if (!e || !ids || B < 1 || which < 0 || which > 2 || clip_skip < 0 || (!hidden && !pooled)) { pd_set_error("pd_sd3_text_encoder: bad argument"); return 1; }
    const bool t5 = which == 2;
    if (t5 ? !e->sd3_t5.built : !e->sd3_clip[which].built) { pd_set_error("pd_sd3_text_encoder: encoder %d is not configured (pd_sd3_text_configure)", which); return 1; }
    if (t5 && (pooled || !hidden || len < 1 || len > 512)) { pd_set_error("pd_sd3_text_encoder: T5 has no pooled output and takes 1 to 512 tokens"); return 1; }
    if (!t5 && clip_skip > (int)e->sd3_clip[which].layers.size() - 1) { pd_set_error("pd_sd3_text_encoder: clip_skip %d out of range [0, %d]", clip_skip, (int)e->sd3_clip[which].layers.size() - 1); return 1; }
    PD_TRY(text_ready(e, "pd_sd3_text_encoder"));
    HIP_OK(hipSetDevice(e->device));
    const int L = t5 ? len : kClipLen, C = t5 ? e->sd3_t5.c.d_model : e->sd3_clip[which].hidden, Pd = t5 ? 0 : e->sd3_clip[which].proj_dim;
    return e->side_call("SD3 text", [&](SideCall& f) {
        const int* di;
        PD_TRY(f.src(&di, ids, (size_t)B * L, mem));
        float* dh = hidden ? f.dst(hidden, (size_t)B * L * C, mem) : nullptr;
        float* dp = pooled ? f.dst(pooled, (size_t)B * Pd, mem) : nullptr;
        return t5 ? e->sd3_t5_forward(di, B, L, dh, L, 0) : e->sd3_clip_forward(e->sd3_clip[which], di, B, clip_skip, dh, L, C, 0, C, dp, Pd);
    });
}
