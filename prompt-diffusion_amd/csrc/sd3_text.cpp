// pdengine: the SD3 text encoders -- what the reference's encode_prompt runs around its tokenizers.
//   _get_clip_prompt_embeds   promptdiffusioncontrolnetpipeline_sd3.py:295-348  (hidden_states[-(clip_skip + 2)] and text_embeds of
//                                                                                CLIPTextModelWithProjection, twice: CLIP-L, CLIP-G)
//   _get_t5_prompt_embeds     promptdiffusioncontrolnetpipeline_sd3.py:238-292  (T5EncoderModel(ids)[0], no attention mask)
//   encode_prompt             promptdiffusioncontrolnetpipeline_sd3.py:457-471  (cat / pad / cat: written in place here, no host concat)
// The CLIP stacks are text.cpp's block with an fp32 residual stream and a per-encoder MLP activation; one pass serves both outputs (the
// hidden state is captured at the skip layer, the stack carries on to the final LayerNorm, EOS row and text_projection).  T5: token
// embedding without positions, pre-RMSNorm blocks, softmax(Q K^T + bias) V with scale 1 and the Toeplitz bias rows of attention.hip's
// BIAS instantiation (block 0's table, shared by all blocks), feed-forward wo(gelu_new(wi_0 x) * wi_1 x) in one gated GEMM epilogue.
#include <algorithm>

#include "engine.h"

namespace {
constexpr int kTextGroup = 6;
constexpr int kClipLen = 77;
inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
}  // namespace

void pd_engine::build_sd3_clip(const std::string& prefix, Sd3ClipW& t) {
    const pd_sd3_clip_config& c = t.c;
    const std::string P = prefix + "text_model.";
    const int C = c.hidden, F = c.ff, L = c.max_positions;
    make_mat(t.tok, c.vocab, C, 1, C, false);
    reg_mat(P + "embeddings.token_embedding.weight", {c.vocab, C}, &t.tok, 0, false);
    make_mat(t.pos, L, C, 1, C, false);
    reg_mat(P + "embeddings.position_embedding.weight", {L, C}, &t.pos, 0, false);
    t.layers.resize(c.layers);   // never resized again (Params point into it)
    for (int i = 0; i < c.layers; ++i) {
        TextLayerW& l = t.layers[i];
        const std::string Lp = P + "encoder.layers." + std::to_string(i) + ".";
        make_mat(l.qkv, 3 * C, C, 1, C, true);   // rows [0,C) q, [C,2C) k, [2C,3C) v -- the attention kernel's layout
        const char* nm[3] = {"k_proj", "v_proj", "q_proj"};   // module order of the checkpoint
        const int off[3] = {C, 2 * C, 0};
        for (int j = 0; j < 3; ++j) {
            reg_mat(Lp + "self_attn." + nm[j] + ".weight", {C, C}, &l.qkv, off[j], false);
            reg_bias(Lp + "self_attn." + nm[j] + ".bias", &l.qkv, off[j], C);
        }
        make_mat(l.out, C, C, 1, C, true);
        reg_mat(Lp + "self_attn.out_proj.weight", {C, C}, &l.out, 0, false);
        reg_bias(Lp + "self_attn.out_proj.bias", &l.out, 0, C);
        reg_vec(Lp + "layer_norm1.weight", C, &l.ln1_g, 'g');
        reg_vec(Lp + "layer_norm1.bias", C, &l.ln1_b, 'e');
        make_mat(l.fc1, F, C, 1, C, true);
        reg_mat(Lp + "mlp.fc1.weight", {F, C}, &l.fc1, 0, false);
        reg_bias(Lp + "mlp.fc1.bias", &l.fc1, 0, F);
        make_mat(l.fc2, C, F, 1, F, true);
        reg_mat(Lp + "mlp.fc2.weight", {C, F}, &l.fc2, 0, false);
        reg_bias(Lp + "mlp.fc2.bias", &l.fc2, 0, C);
        reg_vec(Lp + "layer_norm2.weight", C, &l.ln2_g, 'g');
        reg_vec(Lp + "layer_norm2.bias", C, &l.ln2_b, 'e');
    }
    reg_vec(P + "final_layer_norm.weight", C, &t.fln_g, 'g');
    reg_vec(P + "final_layer_norm.bias", C, &t.fln_b, 'e');
    make_mat(t.proj, c.proj_dim, C, 1, C, false);
    reg_mat(prefix + "text_projection.weight", {c.proj_dim, C}, &t.proj, 0, false);
    t.built = true;
}

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
    if (e->ses.active) { pd_set_error("pd_sd3_text_configure: end the sampling session first"); return 1; }
    const pd_sd3_clip_config* cl[2] = {&c->clip_l, &c->clip_g};
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
    const pd_sd3_t5_config& t = c->t5;
    if (t.layers != 0) {
        if (t.layers < 0 || t.vocab < 1 || t.d_kv != 64 || t.heads < 1 || t.d_model < 8 || t.d_model % 8 || t.d_ff < 8 || t.d_ff % 8 || t.num_buckets < 4 ||
            t.num_buckets % 2 || t.max_distance <= t.num_buckets / 4 || !(t.eps > 0.f)) {
            pd_set_error("pd_sd3_text_configure: T5: need d_kv 64, d_model and d_ff multiples of 8, an even num_buckets >= 4, max_distance > num_buckets / 4, eps > 0");
            return 1;
        }
        if (c->joint_dim != t.d_model) { pd_set_error("pd_sd3_text_configure: joint_dim %d must equal T5's d_model %d (the reference concatenates them row-wise)", c->joint_dim, t.d_model); return 1; }
    }
    if (c->joint_dim < clip_width || c->joint_dim % 4) { pd_set_error("pd_sd3_text_configure: joint_dim %d must be a multiple of 4 and hold both CLIP hidden states (%d)", c->joint_dim, clip_width); return 1; }
    HIP_OK(hipSetDevice(e->device));
    e->alloc_failed = false;
    e->reg_group = kTextGroup;
    e->sd3_text_joint = c->joint_dim;
    const char* prefix[2] = {"text_encoder.", "text_encoder_2."};
    for (int i = 0; i < 2; ++i)
        if (cl[i]->layers > 0) { e->sd3_clip[i].c = *cl[i]; e->build_sd3_clip(prefix[i], e->sd3_clip[i]); }
    if (t.layers > 0) { e->sd3_t5.c = t; e->build_sd3_t5("text_encoder_3."); }
    e->reg_group = 0;
    if (e->alloc_failed) { pd_set_error("pd_sd3_text_configure: weight allocation failed"); return 1; }
    return 0;
}

extern "C" int pd_sd3_text_weights_missing(pd_engine* e) {
    int n = 0;
    if (e)
        for (auto& p : e->params) n += (p.group == kTextGroup && !p.loaded) ? 1 : 0;
    return n;
}

int pd_engine::rmsnorm(const Act& x, void* y, int y_dt, const float* w, float eps, int y_sample_rows, int y_row_off, int y_ld) {
    if (arena.dry) return 0;
    PD_TRY(check_arena());
    ++launches;
    if (x.dt != DT_F32 || launch_rmsnorm_rows(reinterpret_cast<const float*>(x.p), y, y_dt, w, x.rows(), x.C, eps, x.H * x.W, y_sample_rows, y_row_off,
                                              y_ld ? y_ld : x.C, stream)) {
        pd_set_error("rmsnorm launch failed (C=%d)", x.C);
        return 1;
    }
    return 0;
}

int pd_engine::sd3_clip_forward(Sd3ClipW& t, const int* ids_dev, int B, int clip_skip, float* hid, int hid_rows, int hid_ld, int c_off, int width,
                                float* pooled, int pooled_ld) {
    const pd_sd3_clip_config& c = t.c;
    const int C = c.hidden, F = c.ff, L = c.max_positions, H = c.heads, n = c.layers;
    const Activation act = c.act == PD_CLIP_ACT_GELU ? ACT_ERF_GELU : ACT_QUICK_GELU;
    const size_t eb = dt_size(T);
    const size_t mk0 = arena.mark();
    Act x = new_act(B, L, 1, C, DT_F32);   // the residual stream: fp32 in every mode
    if (!arena.dry) {
        PD_TRY(check_arena());
        ++launches;
        if (launch_embed_tokens(ids_dev, t.tok.w, t.tok.Kpad, t.pos.w, t.pos.Kpad, T, x.p, DT_F32, B, L, C, c.vocab, stream)) {
            pd_set_error("CLIP embedding launch failed");
            return 1;
        }
    }
    const int lpad = round_up(L, 8);
    const int capture = n - 1 - clip_skip;   // blocks run before hidden_states[-(clip_skip + 2)] is complete
    auto write_hidden = [&]() -> int {
        if (!hid || arena.dry) return 0;
        ++launches;
        if (launch_joint_write(reinterpret_cast<const float*>(x.p), hid, B, L, C, width, hid_rows, hid_ld, c_off, stream)) {
            pd_set_error("CLIP hidden-state write launch failed");
            return 1;
        }
        return 0;
    };
    if (capture == 0) PD_TRY(write_hidden());
    const int n_run = pooled ? n : capture;   // the pooled output needs the whole stack
    for (int li = 0; li < n_run; ++li) {
        TextLayerW& l = t.layers[li];
        const size_t mk = arena.mark();
        Act ln = new_act(B, L, 1, C, T);
        PD_TRY(layernorm(x, ln, l.ln1_g, l.ln1_b));
        Act qk = new_act(B, L, 1, 2 * C, T);
        Act vt = new_act(B, C, 1, lpad, T);
        if (!arena.dry && lpad != L) HIP_OK(hipMemsetAsync(vt.p, 0, vt.bytes(), stream));   // pad keys of V^T must read as 0
        PD_TRY(gemm(l.qkv, ln, qk, {.VT = vt.p, .vt_begin = 2 * C, .vt_ld = lpad}));
        Act att = new_act(B, L, 1, C, T);
        PD_TRY(attention(qk.p, 2 * C, reinterpret_cast<char*>(qk.p) + (size_t)C * eb, 2 * C, vt.p, lpad, att.p, C, B, L, L, C, H, /*causal=*/true));
        Act h1 = new_act(B, L, 1, C, DT_F32);
        PD_TRY(gemm(l.out, att, h1, {.R = &x}));
        PD_TRY(layernorm(h1, ln, l.ln2_g, l.ln2_b));
        Act f = new_act(B, L, 1, F, T);
        PD_TRY(gemm(l.fc1, ln, f, {.act = act}));
        Act h2 = new_act(B, L, 1, C, DT_F32);
        PD_TRY(gemm(l.fc2, f, h2, {.R = &h1}));
        if (!arena.dry) HIP_OK(hipMemcpyAsync(x.p, h2.p, x.bytes(), hipMemcpyDeviceToDevice, stream));
        arena.release(mk);
        if (li + 1 == capture) PD_TRY(write_hidden());
    }
    if (pooled) {
        // last_hidden_state[b, eos(b)] @ text_projection^T: LayerNorm is per row, so the EOS rows are gathered first
        Act rows = new_act(B, 1, 1, C, DT_F32), lnr = new_act(B, 1, 1, C, DT_F32);
        if (!arena.dry) {
            PD_TRY(check_arena());
            ++launches;
            if (launch_eos_gather(ids_dev, reinterpret_cast<const float*>(x.p), reinterpret_cast<float*>(rows.p), B, L, C, c.eos_token_id, stream)) {
                pd_set_error("CLIP EOS gather launch failed");
                return 1;
            }
        }
        PD_TRY(layernorm(rows, lnr, t.fln_g, t.fln_b));
        if (!arena.dry) {
            for (int b0 = 0; b0 < B; b0 += 4) {   // launch_gemv streams the weights once per <= 4 rows
                ++launches;
                if (launch_gemv(reinterpret_cast<const float*>(lnr.p) + (size_t)b0 * C, C, t.proj.w, T, t.proj.Kpad, nullptr, pooled + (size_t)b0 * pooled_ld,
                                pooled_ld, std::min(4, B - b0), c.proj_dim, C, 0, stream)) {
                    pd_set_error("CLIP text_projection launch failed");
                    return 1;
                }
            }
        }
    }
    arena.release(mk0);
    return 0;
}

int pd_engine::sd3_t5_forward(const int* ids_dev, int B, int Lt, float* out, int out_rows, int row_off) {
    Sd3T5W& t = sd3_t5;
    const pd_sd3_t5_config& c = t.c;
    const int D = c.d_model, I = c.heads * c.d_kv, F = c.d_ff, H = c.heads, L = Lt;
    const size_t eb = dt_size(T);
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
    const int lpad = round_up(L, 8);
    for (size_t li = 0; li < t.layers.size(); ++li) {
        T5LayerW& l = t.layers[li];
        const size_t mk = arena.mark();
        Act ln = new_act(B, L, 1, D, T);
        PD_TRY(rmsnorm(x, ln.p, T, l.ln1, c.eps));
        Act qk = new_act(B, L, 1, 2 * I, T);
        Act vt = new_act(B, I, 1, lpad, T);
        if (!arena.dry && lpad != L) HIP_OK(hipMemsetAsync(vt.p, 0, vt.bytes(), stream));   // pad keys of V^T must read as 0
        PD_TRY(gemm(l.qkv, ln, qk, {.VT = vt.p, .vt_begin = 2 * I, .vt_ld = lpad}));
        Act att = new_act(B, L, 1, I, T);
        PD_TRY(attention(qk.p, 2 * I, reinterpret_cast<char*>(qk.p) + (size_t)I * eb, 2 * I, vt.p, lpad, att.p, I, B, L, L, I, H, /*causal=*/false, 0, 0, 0,
                         relbias, /*scale=*/1.0f));
        Act h1 = new_act(B, L, 1, D, DT_F32);
        PD_TRY(gemm(l.o, att, h1, {.R = &x}));
        PD_TRY(rmsnorm(h1, ln.p, T, l.ln2, c.eps));
        Act f = new_act(B, L, 1, F, T);
        PD_TRY(gemm(l.wi, ln, f, {.act = ACT_GATED_TANH_GELU}));
        Act h2 = new_act(B, L, 1, D, DT_F32);
        PD_TRY(gemm(l.wo, f, h2, {.R = &h1}));
        if (!arena.dry) HIP_OK(hipMemcpyAsync(x.p, h2.p, x.bytes(), hipMemcpyDeviceToDevice, stream));
        arena.release(mk);
    }
    PD_TRY(rmsnorm(x, out, DT_F32, t.fln, c.eps, out_rows, row_off, D));
    arena.release(mk0);
    return 0;
}

namespace {
int text_ready(pd_engine* e, const char* who) {
    if (e->ses.active) { pd_set_error("%s: end the sampling session first", who); return 1; }
    for (auto& p : e->params)
        if (p.group == kTextGroup && !p.loaded) { pd_set_error("SD3 text-encoder weights not loaded: '%s' (and possibly more)", p.name.c_str()); return 1; }
    return 0;
}
// ids to the workspace (int32, `mem` space) -> device pointer
int upload_ids(pd_engine* e, const int32_t* ids, size_t n, int mem, int** dev) {
    *dev = reinterpret_cast<int*>(e->arena.alloc(n * sizeof(int)));
    if (e->arena.dry) return 0;
    PD_TRY(e->check_arena());
    if (hipMemcpyAsync(*dev, ids, n * sizeof(int), mem == PD_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream) != hipSuccess) {
        pd_set_error("token upload failed");
        return 1;
    }
    return 0;
}
int download(pd_engine* e, float* dst, const float* src, size_t n, int mem) {
    if (hipMemcpyAsync(dst, src, n * sizeof(float), mem == PD_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e->stream) != hipSuccess) {
        pd_set_error("embedding read-back failed");
        return 1;
    }
    return 0;
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
        if (a->clip_skip > e->sd3_clip[i].c.layers - 1) { pd_set_error("pd_sd3_encode_prompt: clip_skip %d out of range [0, %d]", a->clip_skip, e->sd3_clip[i].c.layers - 1); return 1; }
    PD_TRY(text_ready(e, "pd_sd3_encode_prompt"));
    HIP_OK(hipSetDevice(e->device));
    const int B = a->batch, Lt = t5 ? a->t5_len : 0, J = e->sd3_text_joint, rows = kClipLen + Lt;
    const int Cl = e->sd3_clip[0].c.hidden, Pl = e->sd3_clip[0].c.proj_dim, Pg = e->sd3_clip[1].c.proj_dim;
    const size_t n_pe = (size_t)B * rows * J, n_po = (size_t)B * (Pl + Pg), n_ids = (size_t)B * (2 * kClipLen + Lt);
    auto body = [&](bool dry) -> int {
        int *il = nullptr, *ig = nullptr, *it = nullptr;
        PD_TRY(upload_ids(e, a->ids_clip_l, (size_t)B * kClipLen, a->mem, &il));
        PD_TRY(upload_ids(e, a->ids_clip_g, (size_t)B * kClipLen, a->mem, &ig));
        if (t5) PD_TRY(upload_ids(e, a->ids_t5, (size_t)B * Lt, a->mem, &it));
        float* dpe = reinterpret_cast<float*>(e->arena.alloc(n_pe * sizeof(float)));
        float* dpo = reinterpret_cast<float*>(e->arena.alloc(n_po * sizeof(float)));
        // rows 0..76: CLIP-L | CLIP-G | zeros up to joint_dim (the second write carries the pad); rows 77..: T5
        PD_TRY(e->sd3_clip_forward(e->sd3_clip[0], il, B, a->clip_skip, dpe, rows, J, 0, Cl, dpo, Pl + Pg));
        PD_TRY(e->sd3_clip_forward(e->sd3_clip[1], ig, B, a->clip_skip, dpe, rows, J, Cl, J - Cl, dpo + Pl, Pl + Pg));
        if (t5) PD_TRY(e->sd3_t5_forward(it, B, Lt, dpe, rows, kClipLen));
        if (dry) return 0;
        PD_TRY(download(e, prompt_embeds, dpe, n_pe, a->mem));
        PD_TRY(download(e, pooled, dpo, n_po, a->mem));
        HIP_OK(hipStreamSynchronize(e->stream));
        return 0;
    };
    return e->vae_in_workspace((n_pe + n_po) * sizeof(float) + n_ids * sizeof(int) + 4096, [&] { return body(true); }, [&] { return body(false); });
}

extern "C" int pd_sd3_text_encoder(pd_engine* e, int32_t which, const int32_t* ids, int32_t B, int32_t len, int32_t clip_skip, int32_t mem,
                                   float* hidden, float* pooled) {
    if (!e || !ids || B < 1 || which < 0 || which > 2 || clip_skip < 0 || (!hidden && !pooled)) { pd_set_error("pd_sd3_text_encoder: bad argument"); return 1; }
    const bool t5 = which == 2;
    if (t5 ? !e->sd3_t5.built : !e->sd3_clip[which].built) { pd_set_error("pd_sd3_text_encoder: encoder %d is not configured (pd_sd3_text_configure)", which); return 1; }
    if (t5 && (pooled || !hidden || len < 1 || len > 512)) { pd_set_error("pd_sd3_text_encoder: T5 has no pooled output and takes 1 to 512 tokens"); return 1; }
    if (!t5 && clip_skip > e->sd3_clip[which].c.layers - 1) { pd_set_error("pd_sd3_text_encoder: clip_skip %d out of range [0, %d]", clip_skip, e->sd3_clip[which].c.layers - 1); return 1; }
    PD_TRY(text_ready(e, "pd_sd3_text_encoder"));
    HIP_OK(hipSetDevice(e->device));
    const int L = t5 ? len : kClipLen, C = t5 ? e->sd3_t5.c.d_model : e->sd3_clip[which].c.hidden, Pd = t5 ? 0 : e->sd3_clip[which].c.proj_dim;
    const size_t n_h = hidden ? (size_t)B * L * C : 0, n_p = pooled ? (size_t)B * Pd : 0;
    auto body = [&](bool dry) -> int {
        int* di = nullptr;
        PD_TRY(upload_ids(e, ids, (size_t)B * L, mem, &di));
        float* dh = hidden ? reinterpret_cast<float*>(e->arena.alloc(n_h * sizeof(float))) : nullptr;
        float* dp = pooled ? reinterpret_cast<float*>(e->arena.alloc(n_p * sizeof(float))) : nullptr;
        if (t5) PD_TRY(e->sd3_t5_forward(di, B, L, dh, L, 0));
        else PD_TRY(e->sd3_clip_forward(e->sd3_clip[which], di, B, clip_skip, dh, L, C, 0, C, dp, Pd));
        if (dry) return 0;
        if (hidden) PD_TRY(download(e, hidden, dh, n_h, mem));
        if (pooled) PD_TRY(download(e, pooled, dp, n_p, mem));
        HIP_OK(hipStreamSynchronize(e->stream));
        return 0;
    };
    return e->vae_in_workspace((n_h + n_p) * sizeof(float) + (size_t)B * L * sizeof(int) + 4096, [&] { return body(true); }, [&] { return body(false); });
}
