// pdengine: first-stage KL-VAE decoder (SURVEY.md §8f "next" row N1) and encoder, built from the same kernels as the loop.
//   LatentDiffusion.decode_first_stage   ldm/models/diffusion/ddpm.py:820-828   (z / scale_factor)
//   AutoencoderKL.decode                 ldm/models/autoencoder.py:89-92        (post_quant_conv, decoder)
//   Decoder.forward                      ldm/modules/diffusionmodules/model.py:619-653
//   ResnetBlock / AttnBlock / Upsample   model.py:82-141, 144-202, 45-65        (GroupNorm eps 1e-6, swish)
//   AutoencoderKL.encode                 autoencoder.py:83-87                   (encoder, quant_conv, posterior)
//   Encoder.forward / Downsample         model.py:508-544, 68-88                (pad (0,1,0,1) + stride-2 conv)
//   DiagonalGaussianDistribution         ldm/modules/distributions/distributions.py:24-62
#include <climits>
#include <cmath>

#include "engine.h"

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

void pd_engine::build_vres(const std::string& prefix, ResW& r, int cin, int cout, bool diffusers) {
    r.cin = cin;
    r.cout = cout;
    r.eps = 1e-6f;
    reg_vec(prefix + "norm1.weight", cin, &r.gn1_g, 'g');
    reg_vec(prefix + "norm1.bias", cin, &r.gn1_b, 'e');
    build_conv(prefix + "conv1.", r.conv1, cin, cout, 3, 1);
    reg_vec(prefix + "norm2.weight", cout, &r.gn2_g, 'g');
    reg_vec(prefix + "norm2.bias", cout, &r.gn2_b, 'e');
    build_conv(prefix + "conv2.", r.conv2, cout, cout, 3, 1);
    r.has_skip = cin != cout;
    if (r.has_skip) build_conv(prefix + (diffusers ? "conv_shortcut." : "nin_shortcut."), r.skip, cin, cout, 1, 1);
}

// diffusers' Attention keeps ldm's four 1x1 convs as Linear layers: the same rows, shape [C, C] instead of [C, C, 1, 1]
void pd_engine::build_vattn(const std::string& prefix, VaeAttnW& a, int C, bool diffusers) {
    a.C = C;
    reg_vec(prefix + (diffusers ? "group_norm.weight" : "norm.weight"), C, &a.g, 'g');
    reg_vec(prefix + (diffusers ? "group_norm.bias" : "norm.bias"), C, &a.b, 'e');
    make_mat(a.qkv, 3 * C, C, 1, C, true);
    const char* nm[3] = {"q", "k", "v"};
    const char* nd[3] = {"to_q", "to_k", "to_v"};
    for (int i = 0; i < 3; ++i) {
        const std::string n = prefix + (diffusers ? nd[i] : nm[i]);
        if (diffusers) reg_mat(n + ".weight", {C, C}, &a.qkv, i * C, false);
        else reg_mat(n + ".weight", {C, C, 1, 1}, &a.qkv, i * C, true);
        reg_bias(n + ".bias", &a.qkv, i * C, C);
    }
    if (diffusers) {
        ConvW& c = a.proj_out;
        c.cin = C; c.cout = C; c.k = 1; c.stride = 1;
        make_mat(c.m, C, C, 1, C, true);
        reg_mat(prefix + "to_out.0.weight", {C, C}, &c.m, 0, false);
        reg_bias(prefix + "to_out.0.bias", &c.m, 0, C);
    } else {
        build_conv(prefix + "proj_out.", a.proj_out, C, C, 1, 1);
    }
}

void pd_engine::build_vae() {
    if (cfg.vae_ch <= 0) return;
    VaeDesc& d = vae.d;
    d.z = cfg.in_channels;
    d.zpad = 8;
    d.ch = cfg.vae_ch;
    d.num_levels = cfg.vae_num_levels;
    for (int i = 0; i < PD_MAX_LEVELS; ++i) d.ch_mult[i] = cfg.vae_ch_mult[i];
    d.num_res_blocks = cfg.vae_num_res_blocks;
    d.out_ch = cfg.vae_out_ch;
    d.scaling = cfg.scale_factor;
    d.group = GROUP_VAE;
    d.enc_group = GROUP_VAE_ENCODER;
    build_vae_decoder(vae, "first_stage_model.");
}

void pd_engine::build_vae_decoder(VaeW& v, const std::string& P) {
    const VaeDesc& d = v.d;
    const bool dif = d.diffusers;
    RegGroup rg(*this, d.group);
    const std::string D = P + "decoder.";
    const int nl = d.num_levels;
    const int top = d.ch * d.ch_mult[nl - 1];
    v.top = top;
    build_conv(D + "conv_in.", v.conv_in, d.z, top, 3, 1);
    build_vres(D + (dif ? "mid_block.resnets.0." : "mid.block_1."), v.mid1, top, top, dif);
    build_vattn(D + (dif ? "mid_block.attentions.0." : "mid.attn_1."), v.attn, top, dif);
    build_vres(D + (dif ? "mid_block.resnets.1." : "mid.block_2."), v.mid2, top, top, dif);
    // parameters are registered in module order up.0 .. up.N-1; execution runs the highest level first
    std::vector<std::vector<std::pair<int, int>>> io(nl);
    std::vector<int> chs(nl);
    int block_in = top;
    for (int lvl = nl - 1; lvl >= 0; --lvl) {
        const int block_out = d.ch * d.ch_mult[lvl];
        for (int j = 0; j <= d.num_res_blocks; ++j) {
            io[lvl].push_back({block_in, block_out});
            block_in = block_out;
        }
        chs[lvl] = block_in;
    }
    v.levels.resize(nl);   // index = execution order
    for (int lvl = 0; lvl < nl; ++lvl) {
        VaeLevel& L = v.levels[nl - 1 - lvl];
        L.blocks.resize(io[lvl].size());   // never resized again
        L.ch = chs[lvl];
        // diffusers numbers the levels in execution order: up_blocks.{i} is ldm's up.{nl - 1 - i}
        const std::string pl = dif ? D + "up_blocks." + std::to_string(nl - 1 - lvl) + "." : D + "up." + std::to_string(lvl) + ".";
        for (size_t j = 0; j < io[lvl].size(); ++j)
            build_vres(pl + (dif ? "resnets." : "block.") + std::to_string(j) + ".", L.blocks[j], io[lvl][j].first, io[lvl][j].second, dif);
        L.up = lvl != 0;
        if (L.up) build_conv(pl + (dif ? "upsamplers.0.conv." : "upsample.conv."), L.upconv, L.ch, L.ch, 3, 1);
    }
    reg_vec(D + (dif ? "conv_norm_out.weight" : "norm_out.weight"), d.ch, &v.out_g, 'g');
    reg_vec(D + (dif ? "conv_norm_out.bias" : "norm_out.bias"), d.ch, &v.out_b, 'e');
    build_conv(D + "conv_out.", v.conv_out, d.ch, d.out_ch, 3, 1);
    if (d.quant) build_conv(P + "post_quant_conv.", v.post_quant, d.z, d.z, 1, 1);
    v.built = true;
}

// Encoder.__init__ (model.py:452-506) with double_z and attn_resolutions = [] (models/cldm_v15.yaml:64-85), then quant_conv =
// Conv2d(2 z, 2 embed_dim, 1) (autoencoder.py:33).  Registered in module order under the checkpoint's names.
void pd_engine::build_vae_encoder() {
    if (!cfg.vae_encoder || cfg.vae_ch <= 0) return;
    vae_enc.d = vae.d;
    build_vae_encoder(vae_enc, "first_stage_model.");
}

void pd_engine::build_vae_encoder(VaeEncW& v, const std::string& P) {
    const VaeDesc& d = v.d;
    const bool dif = d.diffusers;
    RegGroup rg(*this, d.enc_group);
    const std::string E = P + "encoder.";
    const int nl = d.num_levels, z2 = 2 * d.z;
    build_conv(E + "conv_in.", v.conv_in, d.out_ch, d.ch, 3, 1);
    v.levels.resize(nl);   // never resized again
    int block_in = d.ch;
    for (int lvl = 0; lvl < nl; ++lvl) {
        VaeEncLevel& L = v.levels[lvl];
        const int block_out = d.ch * d.ch_mult[lvl];
        L.blocks.resize(d.num_res_blocks);
        const std::string pl = E + (dif ? "down_blocks." : "down.") + std::to_string(lvl) + ".";
        for (int j = 0; j < d.num_res_blocks; ++j) {
            build_vres(pl + (dif ? "resnets." : "block.") + std::to_string(j) + ".", L.blocks[j], block_in, block_out, dif);
            block_in = block_out;
        }
        L.down = lvl != nl - 1;
        if (L.down) {
            build_conv(pl + (dif ? "downsamplers.0.conv." : "downsample.conv."), L.downconv, block_in, block_in, 3, 2);
            L.downconv.pad_shift = 1;   // F.pad(x, (0, 1, 0, 1)), padding 0 (model.py:80-85)
        }
    }
    v.top = block_in;
    build_vres(E + (dif ? "mid_block.resnets.0." : "mid.block_1."), v.mid1, block_in, block_in, dif);
    build_vattn(E + (dif ? "mid_block.attentions.0." : "mid.attn_1."), v.attn, block_in, dif);
    build_vres(E + (dif ? "mid_block.resnets.1." : "mid.block_2."), v.mid2, block_in, block_in, dif);
    reg_vec(E + (dif ? "conv_norm_out.weight" : "norm_out.weight"), block_in, &v.out_g, 'g');
    reg_vec(E + (dif ? "conv_norm_out.bias" : "norm_out.bias"), block_in, &v.out_b, 'e');
    build_conv(E + "conv_out.", v.conv_out, block_in, z2, 3, 1);
    if (d.quant) build_conv(P + "quant_conv.", v.quant, z2, z2, 1, 1);
    v.built = true;
}

// Which path the mid-block attention takes.  Measured on an MI355X at C = 512 (profiles/sd3_vae_bench.json): the flash kernel is SLOWER
// than the three materialised launches where those fit comfortably -- 3.57 ms against 1.88 ms at N = 16384 (1024^2 images), 0.45 against
// 0.19 at N = 4096 -- so by itself it only takes over where the score buffers (fp32 [N, N] + compute-type [N, npad]) pass 2 GiB, or where
// the materialised GEMMs cannot run at all (N no multiple of 8).
bool pd_engine::vae_flash_on(const VaeDesc& d, int C, long long N) const {
    if (f32 || !vae_attention_eligible(T, C)) return false;
    if (opt.vae_flash >= 0) return opt.vae_flash != 0;
    if (!d.flash_auto) return vae_tile_odd_flash && N % 8 != 0;   // (a tile of a tiled call that cannot materialise its scores)
    const long long score_bytes = N * N * 4 + N * ((N + 63) / 64 * 64) * (long long)dt_size(T);
    return score_bytes > (2ll << 30) || N % 8 != 0;
}

int pd_engine::vae_attn_product(const void* qk, int ld, const void* vt, int npad, void* att, int B, int N, int C, bool flash, float* sc, void* pr) {
    const size_t eb = dt_size(T);
    if (flash) {
        VaeAttnParams a{};
        a.Q = qk; a.K = reinterpret_cast<const char*>(qk) + (size_t)C * eb; a.VT = vt; a.O = att;
        a.ldq = ld; a.ldk = ld; a.ldo = C; a.vt_ld = npad;
        a.q_bs = (long long)N * ld; a.k_bs = a.q_bs; a.vt_bs = (long long)C * npad; a.o_bs = (long long)N * C;
        a.B = B; a.N = N; a.C = C; a.scale = (float)(1.0 / std::sqrt((double)C));
        if (launch_vae_attention(a, T, stream)) { pd_set_error("vae attention: flash kernel launch failed (N %d, C %d)", N, C); return 1; }
        ++launches;
        ++vae_flash_launches;
        return 0;
    }
    const int bke = 128 / (int)eb;
    for (int b = 0; b < B; ++b) {
        const char* qb = reinterpret_cast<const char*>(qk) + (size_t)b * N * ld * eb;
        GemmParams p{};
        // scores = (q k^T) * C^-0.5 : A = q rows, "weights" = k rows of the same buffer (row stride ld)
        p.A = qb; p.W = qb + (size_t)C * eb; p.C = sc;
        p.M = N; p.N = N; p.K = C; p.Kpad = round_up(C, bke); p.ldw = ld;
        p.lda = ld; p.ldc = N; p.a_dt = T; p.c_dt = DT_F32; p.r_dt = DT_F32;
        p.taps = 1; p.Cin = C; p.Hin = N; p.Win = 1; p.Hout = N; p.Wout = 1; p.stride = 1;
        p.rows_per_sample = N; p.out_scale = (float)(1.0 / std::sqrt((double)C));
        p.vt_begin = INT_MAX; p.Nout = N; p.splitk = 1; p.big_tile = N >= 1024 ? 1 : 0;
        if (launch_gemm(p, P, stream)) { pd_set_error("vae attention: score GEMM launch failed"); return 1; }
        if (launch_softmax_rows(sc, pr, T, N, N, stream)) { pd_set_error("vae attention: softmax launch failed"); return 1; }
        // out = P v : A = P [N, N], "weights" = V^T [C][npad]; the K tiles past N read zeros on both sides
        GemmParams o{};
        o.A = pr; o.W = reinterpret_cast<const char*>(vt) + (size_t)b * C * npad * eb;
        o.C = reinterpret_cast<char*>(att) + (size_t)b * N * C * eb;
        o.M = N; o.N = C; o.K = N; o.Kpad = round_up(N, bke); o.ldw = npad;
        o.lda = N; o.ldc = C; o.a_dt = T; o.c_dt = T; o.r_dt = DT_F32;
        o.taps = 1; o.Cin = N; o.Hin = N; o.Win = 1; o.Hout = N; o.Wout = 1; o.stride = 1;
        o.rows_per_sample = N; o.out_scale = 1.f; o.vt_begin = INT_MAX; o.Nout = C; o.splitk = 1;
        o.big_tile = N >= 1024 ? 1 : 0;
        if (launch_gemm(o, P, stream)) { pd_set_error("vae attention: value GEMM launch failed"); return 1; }
        launches += 3;
    }
    return 0;
}

// AttnBlock.forward: one head over all C channels, N = H*W tokens.  Materialised: the scores of one sample at a time (fp32 [N,N])
// exactly like the reference's bmm + softmax; at 512x512 that is 64 MiB, once per image.  Flash (vae_flash_on): no score buffers.
int pd_engine::vae_attention(const VaeAttnW& v, const VaeDesc& d, const Act& x, Act& out) {
    const int B = x.B, H = x.H, W = x.W, C = v.C, N = H * W;
    const bool flash = vae_flash_on(d, C, N);
    if (!flash && N % 8) { pd_set_error("vae attention: the materialised path needs h * w a multiple of 8 (got %d x %d)", H, W); return 1; }
    out = new_act(B, H, W, C, S);
    const size_t mk = arena.mark();
    Act a = new_act(B, H, W, C, T);
    PD_TRY(groupnorm(x, a, v.g, v.b, 1e-6f, false));
    Act qk = new_act(B, H, W, 2 * C, T);
    const int npad = flash ? round_up(N, 8) : round_up(N, 64);
    Act vt = new_act(B, C, 1, npad, T);
    if (!arena.dry && !flash && npad != N) HIP_OK(hipMemsetAsync(vt.p, 0, vt.bytes(), stream));   // the value GEMM's K tiles run to npad
    PD_TRY(gemm(v.qkv, a, qk, {.VT = vt.p, .vt_begin = 2 * C, .vt_ld = npad}));
    Act att = new_act(B, H, W, C, T);
    float* sc = nullptr;
    void* pr = nullptr;
    if (!flash) {
        sc = reinterpret_cast<float*>(arena.alloc((size_t)N * N * sizeof(float)));
        pr = arena.alloc((size_t)N * npad * dt_size(T));
    }
    if (!arena.dry) {
        PD_TRY(check_arena());
        if (!flash && npad != N) HIP_OK(hipMemsetAsync(pr, 0, (size_t)N * npad * dt_size(T), stream));
        PD_TRY(vae_attn_product(qk.p, 2 * C, vt.p, npad, att.p, B, N, C, flash, sc, pr));
    }
    PD_TRY(conv(v.proj_out, att, out, {.R = &x}));
    arena.release(mk);
    return 0;
}

int pd_engine::vae_forward(VaeW& v, const float* latents_dev, int B, int h, int w, float* out_dev, float scale, float shift) {
    const VaeDesc& d = v.d;
    Act z = new_act(B, h, w, d.zpad, T);
    if (!arena.dry) {
        ++launches;
        if (launch_nchw_to_nhwc(latents_dev, z.p, T, B, d.z, h, w, d.zpad, stream, scale, shift)) return 1;
    }
    Act img = new_act(B, h << (d.num_levels - 1), w << (d.num_levels - 1), round_up(d.out_ch, 4), DT_F32);
    PD_TRY(vae_decode_layers(v, z, img));
    if (!arena.dry) {
        ++launches;
        if (launch_nhwc_to_nchw(img.p, DT_F32, out_dev, B, d.out_ch, img.H, img.W, img.C, 1.f, stream)) return 1;
    }
    return 0;
}

// post_quant_conv and conv_in .. conv_out of Decoder.forward on z, into the caller's img
int pd_engine::vae_decode_layers(VaeW& v, const Act& z, Act& img) {
    const VaeDesc& d = v.d;
    Act zq = z;
    if (d.quant) {
        zq = new_act(z.B, z.H, z.W, d.zpad, T);   // post_quant_conv writes channels 0..z-1; the pad channels must read as 0
        if (!arena.dry) HIP_OK(hipMemsetAsync(zq.p, 0, zq.bytes(), stream));
        PD_TRY(conv(v.post_quant, z, zq));
    }
    Act hcur = new_act(zq.B, zq.H, zq.W, v.top, S);
    PD_TRY(conv(v.conv_in, zq, hcur));
    Act t;
    PD_TRY(resblock(v.mid1, hcur, t, nullptr, 0));
    hcur = t;
    PD_TRY(vae_attention(v.attn, d, hcur, t));
    hcur = t;
    PD_TRY(resblock(v.mid2, hcur, t, nullptr, 0));
    hcur = t;
    for (VaeLevel& L : v.levels) {
        for (ResW& r : L.blocks) {
            PD_TRY(resblock(r, hcur, t, nullptr, 0));
            hcur = t;
        }
        if (L.up) {
            Act u = new_act(hcur.B, hcur.H * 2, hcur.W * 2, hcur.C, S);
            PD_TRY(conv(L.upconv, hcur, u, {.ups = 1}));   // nearest x2 then conv, model.py:62-64
            hcur = u;
        }
    }
    if (img.B != hcur.B || img.H != hcur.H || img.W != hcur.W) { pd_set_error("internal: VAE decoder output is %d x %d, the caller expects %d x %d", hcur.H, hcur.W, img.H, img.W); return 1; }
    PD_TRY(conv_gn(v.conv_out, hcur, img, v.out_g, v.out_b, 1e-6f, true));
    return 0;
}

extern "C" int pd_vae_weights_missing(pd_engine* e) { return e ? e->missing(GROUP_VAE) : 0; }

int pd_engine::vae_decode_call(VaeW& v, int which, const float* latents, int B, int h, int w, int mem, float scale, float shift, float* images_out) {
    HIP_OK(hipSetDevice(device));
    const int up = 1 << (v.d.num_levels - 1);
    const int H = up * h, W = up * w;
    const size_t n_in = (size_t)B * v.d.z * h * w, n_out = (size_t)B * v.d.out_ch * H * W;
    // tiling / slicing (pd_vae_set_tiling): vae_decode_managed; with both off, vae_forward as ever
    const bool managed = vae_tiling[which].tiling || vae_tiling[which].slicing;
    return side_call("VAE", [&](SideCall& f) {
        const float* src;
        PD_TRY(f.src(&src, latents, n_in, mem));
        float* dout = f.dst(images_out, n_out, mem);
        return managed ? vae_decode_managed(v, which, src, B, h, w, dout, scale, shift) : vae_forward(v, src, B, h, w, dout, scale, shift);
    });
}

extern "C" int pd_vae_decode(pd_engine* e, const float* latents, int32_t B, int32_t h, int32_t w, int32_t mem, float* images_out) {
    if (!e || !latents || !images_out || B < 1 || h < 1 || w < 1) { pd_set_error("bad argument"); return 1; }
    if (!e->vae.built) { pd_set_error("this engine was created without a VAE decoder (vae_ch = 0)"); return 1; }
    if (e->ses.active) { pd_set_error("pd_vae_decode: end the sampling session first"); return 1; }
    // (a tiled call checks its tiles instead: vae_check_tiles)
    if (!e->vae_plan_for(PD_VAE_SD15, h, w, 8, false).tiled && (h * w) % 64) {
        pd_set_error("pd_vae_decode: h*w must be a multiple of 64 (latents of 64x64-pixel multiples)");
        return 1;
    }
    PD_TRY(e->require_loaded(GROUP_VAE, "VAE"));
    return e->vae_decode_call(e->vae, PD_VAE_SD15, latents, B, h, w, mem, (float)(1.0 / e->cfg.scale_factor), 0.f, images_out);
}

// AutoencoderKL.encode (autoencoder.py:83-87): Encoder.forward (model.py:508-544) -> quant_conv -> DiagonalGaussianDistribution
// (distributions.py:24-62), the posterior reduced on the device to what `what` asks for (PD_VAE_*)
int pd_engine::vae_encoder_forward(VaeEncW& v, const float* images_dev, int B, int H, int W, int what, const float* noise_dev, float* out_dev,
                                   float scale, float shift) {
    const VaeDesc& d = v.d;
    const int cin = d.out_ch, z = d.z;
    Act x = new_act(B, H, W, v.conv_in.m.cin_pad, T);
    PD_LAUNCH(this, launch_nchw_to_nhwc(images_dev, x.p, T, B, cin, H, W, x.C, stream), "image upload launch failed");
    const int dn = 1 << (d.num_levels - 1);
    Act mom = new_act(B, H / dn, W / dn, d.quant ? v.quant.m.N : v.conv_out.m.N, DT_F32);
    PD_TRY(vae_encode_layers(v, x, mom));
    PD_LAUNCH(this, launch_vae_posterior(mom.p, DT_F32, mom.C, noise_dev, out_dev, B, z, mom.H * mom.W, what, scale, stream, rng_dev, shift),
              "posterior launch failed");
    return 0;
}

// conv_in .. conv_out of Encoder.forward and quant_conv on x, into the caller's mom (the moments stay fp32)
int pd_engine::vae_encode_layers(VaeEncW& v, const Act& x, Act& mom) {
    const VaeDesc& d = v.d;
    Act hcur = new_act(x.B, x.H, x.W, d.ch, S);
    PD_TRY(conv(v.conv_in, x, hcur));
    Act t;
    for (VaeEncLevel& L : v.levels) {
        for (ResW& r : L.blocks) {
            PD_TRY(resblock(r, hcur, t, nullptr, 0));
            hcur = t;
        }
        if (L.down) {   // Downsample: F.pad(x, (0, 1, 0, 1)) then conv3x3 stride 2, padding 0 (model.py:80-85)
            Act d = new_act(hcur.B, hcur.H / 2, hcur.W / 2, hcur.C, S);
            PD_TRY(conv(L.downconv, hcur, d));
            hcur = d;
        }
    }
    PD_TRY(resblock(v.mid1, hcur, t, nullptr, 0));
    hcur = t;
    PD_TRY(vae_attention(v.attn, d, hcur, t));
    hcur = t;
    PD_TRY(resblock(v.mid2, hcur, t, nullptr, 0));
    hcur = t;
    // norm_out + swish + conv_out, then quant_conv; the moments stay fp32 from here on
    if (mom.B != hcur.B || mom.H != hcur.H || mom.W != hcur.W) { pd_set_error("internal: VAE encoder output is %d x %d, the caller expects %d x %d", hcur.H, hcur.W, mom.H, mom.W); return 1; }
    if (!d.quant) return conv_gn(v.conv_out, hcur, mom, v.out_g, v.out_b, 1e-6f, true);
    Act h = new_act(hcur.B, hcur.H, hcur.W, v.conv_out.m.N, DT_F32);
    PD_TRY(conv_gn(v.conv_out, hcur, h, v.out_g, v.out_b, 1e-6f, true));
    return conv(v.quant, h, mom);
}

extern "C" int pd_vae_encoder_weights_missing(pd_engine* e) { return e ? e->missing(GROUP_VAE_ENCODER) : 0; }

int pd_engine::vae_encode_call(VaeEncW& v, int which, const float* images, int B, int H, int W, int mem, int what, const float* noise, float scale,
                               float shift, float* out) {
    HIP_OK(hipSetDevice(device));
    const int dn = 1 << (v.d.num_levels - 1);
    const int h = H / dn, w = W / dn, z = v.d.z;
    const size_t n_in = (size_t)B * v.d.out_ch * H * W, n_lat = (size_t)B * z * h * w;
    // (noise NULL with PD_VAE_SAMPLE: the posterior kernel draws at (PD_RNG_VAE, draw 0) itself)
    const size_t n_noise = (what == PD_VAE_SAMPLE && noise) ? n_lat : 0, n_out = what == PD_VAE_MOMENTS ? 2 * n_lat : n_lat;
    const bool managed = vae_tiling[which].tiling || vae_tiling[which].slicing;
    return side_call("VAE", [&](SideCall& f) {
        const float *src, *nz = nullptr;
        PD_TRY(f.src(&src, images, n_in, mem));
        if (n_noise) PD_TRY(f.src(&nz, noise, n_noise, mem));
        float* dout = f.dst(out, n_out, mem);
        return managed ? vae_encode_managed(v, which, src, B, H, W, what, nz, dout, scale, shift)
                       : vae_encoder_forward(v, src, B, H, W, what, nz, dout, scale, shift);
    });
}

extern "C" int pd_vae_encode(pd_engine* e, const float* images, int32_t B, int32_t H, int32_t W, int32_t mem, int32_t what,
                             const float* noise, float* out) {
    if (!e || !images || !out || B < 1 || H < 1 || W < 1) { pd_set_error("bad argument"); return 1; }
    if (!e->vae_enc.built) { pd_set_error("this engine was created without a VAE encoder (vae_encoder = 0)"); return 1; }
    PD_TRY(e->require_loaded(GROUP_VAE_ENCODER, "VAE encoder"));
    if (e->ses.active) { pd_set_error("pd_vae_encode: end the sampling session first"); return 1; }
    if (H % 8 || W % 8 || (!e->vae_plan_for(PD_VAE_SD15, H, W, 8, true).tiled && ((H / 8) * (W / 8)) % 64)) {
        pd_set_error("pd_vae_encode: H and W must be multiples of 8 and (H/8)*(W/8) a multiple of 64 (got %d x %d)", H, W);
        return 1;
    }
    if (what != PD_VAE_MEAN && what != PD_VAE_SAMPLE && what != PD_VAE_MOMENTS) {
        pd_set_error("pd_vae_encode: unknown `what` %d (PD_VAE_MEAN / PD_VAE_SAMPLE / PD_VAE_MOMENTS)", what);
        return 1;
    }
    return e->vae_encode_call(e->vae_enc, PD_VAE_SD15, images, B, H, W, mem, what, noise, (float)e->cfg.scale_factor, 0.f, out);
}
