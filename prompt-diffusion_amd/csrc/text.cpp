// pdengine: the CLIP text transformer (SURVEY.md §8f "next" row N3), built from the same kernels as the loop.  One stack serves the
// SD1.5 cond stage and SD3's CLIP-L / CLIP-G (configured and called from sd3_text.cpp):
//   FrozenCLIPEmbedder.forward            ldm/modules/encoders/modules.py:118-128  (layer "last": last_hidden_state)
//   (D) PromptDiffusionPipeline.encode_prompt  pipeline_prompt_diffusion.py:308-487 (text_encoder(ids)[0])
//   _get_clip_prompt_embeds   promptdiffusioncontrolnetpipeline_sd3.py:295-348  (hidden_states[-(clip_skip + 2)] and text_embeds of
//                                                                                CLIPTextModelWithProjection, twice: CLIP-L, CLIP-G)
// The module behind all of them is transformers' CLIPTextModel: token + position embeddings, pre-LN blocks (causal multi-head
// self-attention with biased q/k/v/out projections, quick-GELU or erf-GELU MLP), final LayerNorm.  SD1.5 ("openai/clip-vit-large-patch14",
// weights cond_stage_model.transformer.text_model.*) keeps the residual stream in the engine's stream type; the SD3 encoders keep it in fp32.
// Tokenisation (BPE vocabulary files) stays with the caller: the boundary takes token ids.
#include <algorithm>

#include "engine.h"

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

void pd_engine::build_clip(const std::string& P, ClipW& t) {
    const int C = t.hidden, L = t.positions;
    make_mat(t.tok, t.vocab, C, 1, C, false);
    reg_mat(P + "embeddings.token_embedding.weight", {t.vocab, C}, &t.tok, 0, false);
    make_mat(t.pos, L, C, 1, C, false);
    reg_mat(P + "embeddings.position_embedding.weight", {L, C}, &t.pos, 0, false);
    build_clip_layers(P, t);
    reg_vec(P + "final_layer_norm.weight", C, &t.fln_g, 'g');
    reg_vec(P + "final_layer_norm.bias", C, &t.fln_b, 'e');
    t.built = true;
}

void pd_engine::build_clip_layers(const std::string& P, ClipW& t) {
    const int C = t.hidden, F = t.ff;
    for (size_t i = 0; i < t.layers.size(); ++i) {
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
}

void pd_engine::build_text() {
    if (cfg.text_layers <= 0) return;
    ClipW& t = text;
    t.vocab = cfg.text_vocab; t.hidden = cfg.context_dim; t.ff = cfg.text_ff; t.heads = cfg.text_heads; t.positions = cfg.context_len;
    t.layers.resize(cfg.text_layers);
    RegGroup rg(*this, GROUP_TEXT);
    build_clip("cond_stage_model.transformer.text_model.", t);
}

// token + position embeddings of ids [B, L] int32 (device) -> the residual stream x [B, L, 1, C]
int pd_engine::clip_embed(const ClipW& t, const int* ids_dev, Act& x) {
    PD_LAUNCH(this, launch_embed_tokens(ids_dev, t.tok.w, t.tok.Kpad, t.pos.w, t.pos.Kpad, T, x.p, x.dt, x.B, x.H, x.C, t.vocab, stream),
              "CLIP embedding launch failed");
    return 0;
}

int pd_engine::self_attention(const WMat& qkv, const Act& ln, int inner, int heads, bool causal, const float* relbias, float scale, Act& att) {
    const int B = ln.B, L = ln.H, lpad = round_up(L, 8);
    Act qk = new_act(B, L, 1, 2 * inner, T);
    Act vt = new_act(B, inner, 1, lpad, T);
    if (!arena.dry && lpad != L) HIP_OK(hipMemsetAsync(vt.p, 0, vt.bytes(), stream));   // pad keys of V^T must read as 0
    PD_TRY(gemm(qkv, ln, qk, {.VT = vt.p, .vt_begin = 2 * inner, .vt_ld = lpad}));
    att = new_act(B, L, 1, inner, T);
    const void* K = reinterpret_cast<char*>(qk.p) + (size_t)inner * dt_size(T);   // q | k rows: k starts `inner` columns in
    return attention(qk.p, 2 * inner, K, 2 * inner, vt.p, lpad, att.p, inner, B, L, L, inner, heads, causal, 0, 0, 0, relbias, scale);
}

int pd_engine::clip_block(const TextLayerW& l, Act& x, int heads, Activation act, bool causal, float eps) {
    const int B = x.B, L = x.H, C = x.C;
    const size_t mk = arena.mark();
    Act ln = new_act(B, L, 1, C, T), att;
    PD_TRY(layernorm(x, ln, l.ln1_g, l.ln1_b, eps));
    PD_TRY(self_attention(l.qkv, ln, C, heads, causal, nullptr, 0.f, att));
    Act h1 = new_act(B, L, 1, C, x.dt);
    PD_TRY(gemm(l.out, att, h1, {.R = &x}));
    PD_TRY(layernorm(h1, ln, l.ln2_g, l.ln2_b, eps));
    Act f = new_act(B, L, 1, l.fc1.Nout, T);
    PD_TRY(gemm(l.fc1, ln, f, {.act = act}));
    Act h2 = new_act(B, L, 1, C, x.dt);
    PD_TRY(gemm(l.fc2, f, h2, {.R = &h1}));
    // carry the block output down to the slot below this block's temporaries
    if (!arena.dry) HIP_OK(hipMemcpyAsync(x.p, h2.p, x.bytes(), hipMemcpyDeviceToDevice, stream));
    arena.release(mk);
    return 0;
}

int pd_engine::clip_blocks(const ClipW& t, int first, int last, Act& x) {
    for (int li = first; li < last; ++li) PD_TRY(clip_block(t.layers[li], x, t.heads, t.act, t.causal, t.eps));
    return 0;
}

// tokens [B, L] int32 (device) -> last_hidden_state [B, L, C] fp32 (device)
int pd_engine::text_forward(const int* ids_dev, int B, float* out_dev, int clip_skip) {
    ClipW& t = text;
    Act x = new_act(B, t.positions, 1, t.hidden, S);
    PD_TRY(clip_embed(t, ids_dev, x));
    PD_TRY(clip_blocks(t, 0, (int)t.layers.size() - clip_skip, x));   // hidden_states[-(clip_skip+1)]: output of block n - clip_skip
    Act out = new_act(B, t.positions, 1, t.hidden, DT_F32);
    PD_TRY(layernorm(x, out, t.fln_g, t.fln_b));
    if (!arena.dry) HIP_OK(hipMemcpyAsync(out_dev, out.p, out.bytes(), hipMemcpyDeviceToDevice, stream));
    return 0;
}

// One pass serves both outputs: the hidden state is written at the skip layer; the pooled output carries on through the rest of the
// stack to the final LayerNorm, EOS row and text_projection.
int pd_engine::sd3_clip_forward(ClipW& t, const int* ids_dev, int B, int clip_skip, float* hid, int hid_rows, int hid_ld, int c_off, int width,
                                float* pooled, int pooled_ld) {
    const int C = t.hidden, L = t.positions, n = (int)t.layers.size();
    const size_t mk0 = arena.mark();
    Act x = new_act(B, L, 1, C, DT_F32);   // the residual stream: fp32 in every mode
    PD_TRY(clip_embed(t, ids_dev, x));
    const int capture = n - 1 - clip_skip;   // blocks run before hidden_states[-(clip_skip + 2)] is complete
    PD_TRY(clip_blocks(t, 0, capture, x));
    if (hid)
        PD_LAUNCH(this, launch_joint_write(reinterpret_cast<const float*>(x.p), hid, B, L, C, width, hid_rows, hid_ld, c_off, stream),
                  "CLIP hidden-state write launch failed");
    if (pooled) {
        PD_TRY(clip_blocks(t, capture, n, x));
        // last_hidden_state[b, eos(b)] @ text_projection^T: LayerNorm is per row, so the EOS rows are gathered first
        Act rows = new_act(B, 1, 1, C, DT_F32), lnr = new_act(B, 1, 1, C, DT_F32);
        PD_LAUNCH(this, launch_eos_gather(ids_dev, reinterpret_cast<const float*>(x.p), reinterpret_cast<float*>(rows.p), B, L, C, t.eos_token_id, stream),
                  "CLIP EOS gather launch failed");
        PD_TRY(layernorm(rows, lnr, t.fln_g, t.fln_b));
        for (int b0 = 0; b0 < B; b0 += 4)   // launch_gemv streams the weights once per <= 4 rows
            PD_LAUNCH(this, launch_gemv(reinterpret_cast<const float*>(lnr.p) + (size_t)b0 * C, C, t.proj.w, T, t.proj.Kpad, nullptr,
                                        pooled + (size_t)b0 * pooled_ld, pooled_ld, std::min(4, B - b0), t.proj_dim, C, 0, stream),
                      "CLIP text_projection launch failed");
    }
    arena.release(mk0);
    return 0;
}

extern "C" int pd_text_weights_missing(pd_engine* e) { return e ? e->missing(GROUP_TEXT) : 0; }

extern "C" int pd_text_encode_ex(pd_engine* e, const int32_t* ids, int32_t B, int32_t mem, int32_t clip_skip, float* out) {
    if (!e || !ids || !out || B < 1) { pd_set_error("bad argument"); return 1; }
    if (clip_skip < 0 || (e->text.built && clip_skip > (int)e->text.layers.size())) {   // k = text_layers: hidden_states[0], the embeddings
        pd_set_error("clip_skip %d out of range [0, %d]", clip_skip, e->cfg.text_layers);
        return 1;
    }
    if (!e->text.built) { pd_set_error("this engine was created without a text transformer (text_layers = 0)"); return 1; }
    if (e->ses.active) { pd_set_error("pd_text_encode: end the sampling session first"); return 1; }
    PD_TRY(e->require_loaded(GROUP_TEXT, "text transformer"));
    HIP_OK(hipSetDevice(e->device));
    const size_t n_in = (size_t)B * e->text.positions, n_out = n_in * e->text.hidden;
    return e->side_call("text", [&](SideCall& f) {
        const int* din;
        PD_TRY(f.src(&din, ids, n_in, mem));
        return e->text_forward(din, B, f.dst(out, n_out, mem), clip_skip);
    });
}

extern "C" int pd_text_encode(pd_engine* e, const int32_t* ids, int32_t B, int32_t mem, float* out) {
    return pd_text_encode_ex(e, ids, B, mem, 0, out);
}
