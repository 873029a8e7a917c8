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

void pd_engine::build_vres(const std::string& prefix, ResW& r, int cin, int cout) {
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
    if (r.has_skip) build_conv(prefix + "nin_shortcut.", r.skip, cin, cout, 1, 1);
}

void pd_engine::build_vattn(const std::string& prefix, VaeAttnW& a, int C) {
    a.C = C;
    reg_vec(prefix + "norm.weight", C, &a.g, 'g');
    reg_vec(prefix + "norm.bias", C, &a.b, 'e');
    make_mat(a.qkv, 3 * C, C, 1, C, true);
    const char* nm[3] = {"q", "k", "v"};
    for (int i = 0; i < 3; ++i) {
        reg_mat(prefix + nm[i] + ".weight", {C, C, 1, 1}, &a.qkv, i * C, true);
        reg_bias(prefix + nm[i] + ".bias", &a.qkv, i * C, C);
    }
    build_conv(prefix + "proj_out.", a.proj_out, C, C, 1, 1);
}

void pd_engine::build_vae() {
    if (cfg.vae_ch <= 0) return;
    reg_group = GROUP_VAE;
    const std::string P = "first_stage_model.", D = P + "decoder.";
    const int nl = cfg.vae_num_levels;
    const int top = cfg.vae_ch * cfg.vae_ch_mult[nl - 1];
    VaeW& v = vae;
    v.top = top;
    build_conv(D + "conv_in.", v.conv_in, cfg.in_channels, top, 3, 1);
    build_vres(D + "mid.block_1.", v.mid1, top, top);
    build_vattn(D + "mid.attn_1.", v.attn, top);
    build_vres(D + "mid.block_2.", v.mid2, top, top);
    // parameters are registered in module order up.0 .. up.N-1; execution runs the highest level first
    std::vector<std::vector<std::pair<int, int>>> io(nl);
    std::vector<int> chs(nl);
    int block_in = top;
    for (int lvl = nl - 1; lvl >= 0; --lvl) {
        const int block_out = cfg.vae_ch * cfg.vae_ch_mult[lvl];
        for (int j = 0; j <= cfg.vae_num_res_blocks; ++j) {
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
        for (size_t j = 0; j < io[lvl].size(); ++j)
            build_vres(D + "up." + std::to_string(lvl) + ".block." + std::to_string(j) + ".", L.blocks[j], io[lvl][j].first,
                       io[lvl][j].second);
        L.up = lvl != 0;
        if (L.up) build_conv(D + "up." + std::to_string(lvl) + ".upsample.conv.", L.upconv, L.ch, L.ch, 3, 1);
    }
    reg_vec(D + "norm_out.weight", cfg.vae_ch, &v.out_g, 'g');
    reg_vec(D + "norm_out.bias", cfg.vae_ch, &v.out_b, 'e');
    build_conv(D + "conv_out.", v.conv_out, cfg.vae_ch, cfg.vae_out_ch, 3, 1);
    build_conv(P + "post_quant_conv.", v.post_quant, cfg.in_channels, cfg.in_channels, 1, 1);
    v.built = true;
    reg_group = GROUP_SAMPLER;
}

// Encoder.__init__ (model.py:452-506) with double_z and attn_resolutions = [] (models/cldm_v15.yaml:64-85), then quant_conv =
// Conv2d(2 z, 2 embed_dim, 1) (autoencoder.py:33).  Registered in module order under the checkpoint's names.
void pd_engine::build_vae_encoder() {
    if (!cfg.vae_encoder || cfg.vae_ch <= 0) return;
    reg_group = GROUP_VAE_ENCODER;
    const std::string P = "first_stage_model.", E = P + "encoder.";
    const int nl = cfg.vae_num_levels, z2 = 2 * cfg.in_channels;
    VaeEncW& v = vae_enc;
    build_conv(E + "conv_in.", v.conv_in, cfg.vae_out_ch, cfg.vae_ch, 3, 1);
    v.levels.resize(nl);   // never resized again
    int block_in = cfg.vae_ch;
    for (int lvl = 0; lvl < nl; ++lvl) {
        VaeEncLevel& L = v.levels[lvl];
        const int block_out = cfg.vae_ch * cfg.vae_ch_mult[lvl];
        L.blocks.resize(cfg.vae_num_res_blocks);
        const std::string pl = E + "down." + std::to_string(lvl) + ".";
        for (int j = 0; j < cfg.vae_num_res_blocks; ++j) {
            build_vres(pl + "block." + std::to_string(j) + ".", L.blocks[j], block_in, block_out);
            block_in = block_out;
        }
        L.down = lvl != nl - 1;
        if (L.down) {
            build_conv(pl + "downsample.conv.", L.downconv, block_in, block_in, 3, 2);
            L.downconv.pad_shift = 1;   // F.pad(x, (0, 1, 0, 1)), padding 0 (model.py:80-85)
        }
    }
    v.top = block_in;
    build_vres(E + "mid.block_1.", v.mid1, block_in, block_in);
    build_vattn(E + "mid.attn_1.", v.attn, block_in);
    build_vres(E + "mid.block_2.", v.mid2, block_in, block_in);
    reg_vec(E + "norm_out.weight", block_in, &v.out_g, 'g');
    reg_vec(E + "norm_out.bias", block_in, &v.out_b, 'e');
    build_conv(E + "conv_out.", v.conv_out, block_in, z2, 3, 1);
    build_conv(P + "quant_conv.", v.quant, z2, z2, 1, 1);
    v.built = true;
    reg_group = GROUP_SAMPLER;
}

// AttnBlock.forward: one head over all C channels, N = H*W tokens.  Scores are materialised per sample (fp32
// [N,N]) exactly like the reference's bmm + softmax; at 512x512 that is 64 MiB per sample, once per image.
int pd_engine::vae_attention(const VaeAttnW& v, const Act& x, Act& out) {
    const int B = x.B, H = x.H, W = x.W, C = v.C, N = H * W;
    out = new_act(B, H, W, C, S);
    const size_t mk = arena.mark();
    Act a = new_act(B, H, W, C, T);
    PD_TRY(groupnorm(x, a, v.g, v.b, 1e-6f, false));
    Act qk = new_act(B, H, W, 2 * C, T);
    const int npad = round_up(N, 8);
    Act vt = new_act(B, C, 1, npad, T);
    PD_TRY(gemm(v.qkv, a, qk, {.VT = vt.p, .vt_begin = 2 * C, .vt_ld = npad}));
    Act att = new_act(B, H, W, C, T);
    float* sc = reinterpret_cast<float*>(arena.alloc((size_t)N * N * sizeof(float)));
    void* pr = arena.alloc((size_t)N * npad * dt_size(T));
    if (!arena.dry) {
        if (npad != N) HIP_OK(hipMemsetAsync(pr, 0, (size_t)N * npad * dt_size(T), stream));
        const size_t eb = dt_size(T);
        const int bke = 128 / (int)eb;
        for (int b = 0; b < B; ++b) {
            const char* qb = reinterpret_cast<const char*>(qk.p) + (size_t)b * N * 2 * C * eb;
            GemmParams p{};
            // scores = (q k^T) * C^-0.5 : A = q rows, "weights" = k rows of the same buffer (row stride 2C)
            p.A = qb; p.W = qb + (size_t)C * eb; p.C = sc;
            p.M = N; p.N = N; p.K = C; p.Kpad = round_up(C, bke); p.ldw = 2 * C;
            p.lda = 2 * C; p.ldc = N; p.a_dt = T; p.c_dt = DT_F32; p.r_dt = DT_F32;
            p.taps = 1; p.Cin = C; p.Hin = N; p.Win = 1; p.Hout = N; p.Wout = 1; p.stride = 1;
            p.rows_per_sample = N; p.out_scale = (float)(1.0 / std::sqrt((double)C));
            p.vt_begin = INT_MAX; p.Nout = N; p.splitk = 1; p.big_tile = N >= 1024 ? 1 : 0;
            if (launch_gemm(p, P, stream)) { pd_set_error("vae attention: score GEMM launch failed"); return 1; }
            if (launch_softmax_rows(sc, pr, T, N, N, stream)) { pd_set_error("vae attention: softmax launch failed"); return 1; }
            // out = P v : A = P [N, N] (row stride npad when padded), "weights" = V^T [C][npad]
            GemmParams o{};
            o.A = pr; o.W = reinterpret_cast<const char*>(vt.p) + (size_t)b * C * npad * eb;
            o.C = reinterpret_cast<char*>(att.p) + (size_t)b * N * C * eb;
            o.M = N; o.N = C; o.K = N; o.Kpad = round_up(N, bke); o.ldw = npad;
            o.lda = N; o.ldc = C; o.a_dt = T; o.c_dt = T; o.r_dt = DT_F32;
            o.taps = 1; o.Cin = N; o.Hin = N; o.Win = 1; o.Hout = N; o.Wout = 1; o.stride = 1;
            o.rows_per_sample = N; o.out_scale = 1.f; o.vt_begin = INT_MAX; o.Nout = C; o.splitk = 1;
            o.big_tile = N >= 1024 ? 1 : 0;
            if (launch_gemm(o, P, stream)) { pd_set_error("vae attention: value GEMM launch failed"); return 1; }
            launches += 3;
        }
    }
    PD_TRY(conv(v.proj_out, att, out, {.R = &x}));
    arena.release(mk);
    return 0;
}

int pd_engine::vae_forward(const float* latents_dev, int B, int h, int w, float* out_dev) {
    VaeW& v = vae;
    Act z = new_act(B, h, w, 8, T);
    if (!arena.dry) {
        ++launches;
        if (launch_nchw_to_nhwc(latents_dev, z.p, T, B, cfg.in_channels, h, w, 8, stream, (float)(1.0 / cfg.scale_factor))) return 1;
    }
    Act zq = new_act(B, h, w, 8, T);   // post_quant_conv writes channels 0..in_ch-1; the pad channels must read as 0
    if (!arena.dry) HIP_OK(hipMemsetAsync(zq.p, 0, zq.bytes(), stream));
    PD_TRY(conv(v.post_quant, z, zq));
    Act hcur = new_act(B, h, w, v.top, S);
    PD_TRY(conv(v.conv_in, zq, hcur));
    Act t;
    PD_TRY(resblock(v.mid1, hcur, t, nullptr, 0));
    hcur = t;
    PD_TRY(vae_attention(v.attn, hcur, t));
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
    Act img = new_act(hcur.B, hcur.H, hcur.W, round_up(cfg.vae_out_ch, 4), DT_F32);
    PD_TRY(conv_gn(v.conv_out, hcur, img, v.out_g, v.out_b, 1e-6f, true));
    if (!arena.dry) {
        ++launches;
        if (launch_nhwc_to_nchw(img.p, DT_F32, out_dev, B, cfg.vae_out_ch, img.H, img.W, img.C, 1.f, stream)) return 1;
    }
    return 0;
}

extern "C" int pd_vae_weights_missing(pd_engine* e) { return e ? e->missing(GROUP_VAE) : 0; }

extern "C" int pd_vae_decode(pd_engine* e, const float* latents, int32_t B, int32_t h, int32_t w, int32_t mem, float* images_out) {
    if (!e || !latents || !images_out || B < 1 || h < 1 || w < 1) { pd_set_error("bad argument"); return 1; }
    if (!e->vae.built) { pd_set_error("this engine was created without a VAE decoder (vae_ch = 0)"); return 1; }
    if (e->ses.active) { pd_set_error("pd_vae_decode: end the sampling session first"); return 1; }
    if ((h * w) % 64) { pd_set_error("pd_vae_decode: h*w must be a multiple of 64 (latents of 64x64-pixel multiples)"); return 1; }
    PD_TRY(e->require_loaded(GROUP_VAE, "VAE"));
    HIP_OK(hipSetDevice(e->device));
    const int H = 8 * h, W = 8 * w;
    const size_t n_in = (size_t)B * e->cfg.in_channels * h * w, n_out = (size_t)B * e->cfg.vae_out_ch * H * W;
    return e->in_side_workspace("VAE", (n_in + n_out) * sizeof(float), [&] { return e->vae_forward(nullptr, B, h, w, nullptr); }, [&] {
        int r = 0;
        float* din = reinterpret_cast<float*>(e->arena.alloc(n_in * sizeof(float)));
        float* dout = reinterpret_cast<float*>(e->arena.alloc(n_out * sizeof(float)));
        const float* src = latents;
        if (mem != PD_MEM_DEVICE) {
            if (hipMemcpyAsync(din, latents, n_in * sizeof(float), hipMemcpyHostToDevice, e->stream) != hipSuccess ||
                hipStreamSynchronize(e->stream) != hipSuccess) { pd_set_error("latent upload failed"); r = 1; }
            src = din;
        }
        if (!r) r = e->vae_forward(src, B, h, w, dout);
        if (!r) {
            if (hipMemcpyAsync(images_out, dout, n_out * sizeof(float),
                               mem == PD_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
                hipStreamSynchronize(e->stream) != hipSuccess) { pd_set_error("image read-back failed"); r = 1; }
        }
        return r;
    });
}

// AutoencoderKL.encode (autoencoder.py:83-87): Encoder.forward (model.py:508-544) -> quant_conv -> DiagonalGaussianDistribution
// (distributions.py:24-62), the posterior reduced on the device to what `what` asks for (PD_VAE_*)
int pd_engine::vae_encoder_forward(const float* images_dev, int B, int H, int W, int what, const float* noise_dev, float* out_dev) {
    VaeEncW& v = vae_enc;
    const int cin = cfg.vae_out_ch, z = cfg.in_channels;
    Act x = new_act(B, H, W, v.conv_in.m.cin_pad, T);
    if (!arena.dry) {
        PD_TRY(check_arena());
        ++launches;
        if (launch_nchw_to_nhwc(images_dev, x.p, T, B, cin, H, W, x.C, stream)) { pd_set_error("image upload launch failed"); return 1; }
    }
    Act hcur = new_act(B, H, W, cfg.vae_ch, S);
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
    PD_TRY(vae_attention(v.attn, hcur, t));
    hcur = t;
    PD_TRY(resblock(v.mid2, hcur, t, nullptr, 0));
    hcur = t;
    // norm_out + swish + conv_out, then quant_conv; the moments stay fp32 from here on
    Act h = new_act(hcur.B, hcur.H, hcur.W, v.conv_out.m.N, DT_F32);
    PD_TRY(conv_gn(v.conv_out, hcur, h, v.out_g, v.out_b, 1e-6f, true));
    Act mom = new_act(h.B, h.H, h.W, v.quant.m.N, DT_F32);
    PD_TRY(conv(v.quant, h, mom));
    if (!arena.dry) {
        PD_TRY(check_arena());
        ++launches;
        if (launch_vae_posterior(mom.p, DT_F32, mom.C, noise_dev, out_dev, B, z, mom.H * mom.W, what, (float)cfg.scale_factor, stream,
                                 rng_dev)) {
            pd_set_error("posterior launch failed");
            return 1;
        }
    }
    return 0;
}

extern "C" int pd_vae_encoder_weights_missing(pd_engine* e) { return e ? e->missing(GROUP_VAE_ENCODER) : 0; }

extern "C" int pd_vae_encode(pd_engine* e, const float* images, int32_t B, int32_t H, int32_t W, int32_t mem, int32_t what,
                             const float* noise, float* out) {
    if (!e || !images || !out || B < 1 || H < 1 || W < 1) { pd_set_error("bad argument"); return 1; }
    if (!e->vae_enc.built) { pd_set_error("this engine was created without a VAE encoder (vae_encoder = 0)"); return 1; }
    PD_TRY(e->require_loaded(GROUP_VAE_ENCODER, "VAE encoder"));
    if (e->ses.active) { pd_set_error("pd_vae_encode: end the sampling session first"); return 1; }
    if (H % 8 || W % 8 || ((H / 8) * (W / 8)) % 64) {
        pd_set_error("pd_vae_encode: H and W must be multiples of 8 and (H/8)*(W/8) a multiple of 64 (got %d x %d)", H, W);
        return 1;
    }
    if (what != PD_VAE_MEAN && what != PD_VAE_SAMPLE && what != PD_VAE_MOMENTS) {
        pd_set_error("pd_vae_encode: unknown `what` %d (PD_VAE_MEAN / PD_VAE_SAMPLE / PD_VAE_MOMENTS)", what);
        return 1;
    }
    HIP_OK(hipSetDevice(e->device));
    const int h = H / 8, w = W / 8, z = e->cfg.in_channels;
    const size_t n_in = (size_t)B * e->cfg.vae_out_ch * H * W, n_lat = (size_t)B * z * h * w;
    // (noise NULL with PD_VAE_SAMPLE: the posterior kernel draws at (PD_RNG_VAE, draw 0) itself)
    const size_t n_noise = (what == PD_VAE_SAMPLE && noise) ? n_lat : 0, n_out = what == PD_VAE_MOMENTS ? 2 * n_lat : n_lat;
    return e->in_side_workspace("VAE", (n_in + n_noise + n_out) * sizeof(float),
                                [&] { return e->vae_encoder_forward(nullptr, B, H, W, what, nullptr, nullptr); }, [&] {
        int r = 0;
        float* din = reinterpret_cast<float*>(e->arena.alloc(n_in * sizeof(float)));
        float* dnoise = n_noise ? reinterpret_cast<float*>(e->arena.alloc(n_noise * sizeof(float))) : nullptr;
        float* dout = reinterpret_cast<float*>(e->arena.alloc(n_out * sizeof(float)));
        const float* src = images;
        const float* nz = noise;
        if (mem != PD_MEM_DEVICE) {
            if (hipMemcpyAsync(din, images, n_in * sizeof(float), hipMemcpyHostToDevice, e->stream) != hipSuccess ||
                (dnoise && hipMemcpyAsync(dnoise, noise, n_noise * sizeof(float), hipMemcpyHostToDevice, e->stream) != hipSuccess) ||
                hipStreamSynchronize(e->stream) != hipSuccess) { pd_set_error("image upload failed"); r = 1; }
            src = din;
            nz = dnoise;
        }
        if (!r) r = e->vae_encoder_forward(src, B, H, W, what, what == PD_VAE_SAMPLE ? nz : nullptr, dout);
        if (!r) {
            if (hipMemcpyAsync(out, dout, n_out * sizeof(float), mem == PD_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                               e->stream) != hipSuccess ||
                hipStreamSynchronize(e->stream) != hipSuccess) { pd_set_error("latent read-back failed"); r = 1; }
        }
        return r;
    });
}
