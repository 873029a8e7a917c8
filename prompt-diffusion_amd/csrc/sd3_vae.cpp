// pdengine: SD3's VAE -- what the reference's SD3 pipeline calls around its denoising loop.
//   vae.encode(control_image).latent_dist.sample(), (z - shift) * scaling   promptdiffusioncontrolnetpipeline_sd3.py:1132-1133
//   the same on the down-projected example pair (encode_support_pair)        promptdiffusioncontrolnetpipeline_sd3.py:1112-1115
//   vae.decode(latents / scaling + shift)                                    promptdiffusioncontrolnetpipeline_sd3.py:1271-1273
// diffusers' AutoencoderKL is the ldm Encoder / Decoder of vae.cpp (ldm/modules/diffusionmodules/model.py) under other parameter
// names, here with 16 latent channels, no quant convs and a shift next to the scaling factor; the layers, their order and their
// kernels are vae.cpp's, driven by a VaeDesc of its own.
#include <cstddef>

#include "engine.h"

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

extern "C" int pd_sd3_vae_config_layout(int32_t* size, int32_t* off_scaling, int32_t* off_shift) {
    if (size) *size = (int32_t)sizeof(pd_sd3_vae_config);
    if (off_scaling) *off_scaling = (int32_t)offsetof(pd_sd3_vae_config, scaling_factor);
    if (off_shift) *off_shift = (int32_t)offsetof(pd_sd3_vae_config, shift_factor);
    return 0;
}

extern "C" int pd_sd3_vae_configure(pd_engine* e, const pd_sd3_vae_config* c) {
    if (!e || !c) { pd_set_error("bad argument"); return 1; }
    if (e->sd3_vae.built) { pd_set_error("pd_sd3_vae_configure: already configured"); return 1; }
    auto check = [&]() -> int {
        bool ok = c->ch >= 32 && c->ch % 32 == 0 && c->num_levels >= 1 && c->num_levels <= PD_MAX_LEVELS && c->num_res_blocks >= 1 && c->z_channels >= 1 &&
                  c->out_ch >= 1 && c->out_ch <= 4 && c->scaling_factor > 0.0;
        for (int i = 0; ok && i < c->num_levels; ++i) ok = c->ch_mult[i] >= 1;
        if (!ok) {
            pd_set_error("pd_sd3_vae_configure: need ch a multiple of 32 (GroupNorm groups), 1 <= num_levels <= %d, ch_mult >= 1, num_res_blocks >= 1, "
                         "z_channels >= 1, 1 <= out_ch <= 4, scaling_factor > 0", PD_MAX_LEVELS);
            return 1;
        }
        return 0;
    };
    // (the builders register under the groups of their VaeDesc)
    return e->configure("pd_sd3_vae_configure", GROUP_SD3_VAE, check, [&] {
        VaeDesc d;
        d.z = c->z_channels;
        d.zpad = round_up(d.z, 8);
        d.ch = c->ch;
        d.num_levels = c->num_levels;
        for (int i = 0; i < c->num_levels; ++i) d.ch_mult[i] = c->ch_mult[i];
        d.num_res_blocks = c->num_res_blocks;
        d.out_ch = c->out_ch;
        d.scaling = c->scaling_factor;
        d.shift = c->shift_factor;
        d.flash_auto = true;
        d.diffusers = true;
        d.group = GROUP_SD3_VAE;
        d.enc_group = GROUP_SD3_VAE_ENCODER;
        d.quant = c->post_quant_conv != 0;
        e->sd3_vae.d = d;
        e->build_vae_decoder(e->sd3_vae, "vae.");
        if (c->encoder) {
            d.quant = c->quant_conv != 0;
            e->sd3_vae_enc.d = d;
            e->build_vae_encoder(e->sd3_vae_enc, "vae.");
        }
    });
}

extern "C" int pd_sd3_vae_weights_missing(pd_engine* e) {
    return e ? e->missing(GROUP_SD3_VAE) + e->missing(GROUP_SD3_VAE_ENCODER) : 0;
}

extern "C" int pd_sd3_vae_decode(pd_engine* e, const float* latents, int32_t B, int32_t h, int32_t w, int32_t mem, int32_t raw, float* images) {
    if (!e || !latents || !images || B < 1 || h < 1 || w < 1) { pd_set_error("bad argument"); return 1; }
    VaeW& v = e->sd3_vae;
    if (!v.built) { pd_set_error("pd_sd3_vae_decode: no SD3 VAE on this engine (pd_sd3_vae_configure)"); return 1; }
    if (e->ses.active) { pd_set_error("pd_sd3_vae_decode: end the sampling session first"); return 1; }
    if (!e->vae_plan_for(PD_VAE_SD3, h, w, 1 << (v.d.num_levels - 1), false).tiled && !e->vae_flash_on(v.d, v.attn.C, (long long)h * w) && (h * w) % 8) {
        pd_set_error("pd_sd3_vae_decode: h * w must be a multiple of 8 where the mid-block attention materialises its scores (got %d x %d)", h, w);
        return 1;
    }
    PD_TRY(e->require_loaded(GROUP_SD3_VAE, "SD3 VAE"));
    return e->vae_decode_call(v, PD_VAE_SD3, latents, B, h, w, mem, raw ? 1.f : (float)(1.0 / v.d.scaling), raw ? 0.f : (float)v.d.shift, images);
}

extern "C" int pd_sd3_vae_encode(pd_engine* e, const float* images, int32_t B, int32_t H, int32_t W, int32_t mem, int32_t what, const float* noise,
                                 int32_t raw, float* out) {
    if (!e || !images || !out || B < 1 || H < 1 || W < 1) { pd_set_error("bad argument"); return 1; }
    VaeEncW& v = e->sd3_vae_enc;
    if (!v.built) { pd_set_error("pd_sd3_vae_encode: no SD3 VAE encoder on this engine (pd_sd3_vae_configure with encoder = 1)"); return 1; }
    PD_TRY(e->require_loaded(GROUP_SD3_VAE_ENCODER, "SD3 VAE encoder"));
    if (e->ses.active) { pd_set_error("pd_sd3_vae_encode: end the sampling session first"); return 1; }
    const int dn = 1 << (v.d.num_levels - 1);
    if (H % dn || W % dn) { pd_set_error("pd_sd3_vae_encode: H and W must be multiples of %d (got %d x %d)", dn, H, W); return 1; }
    if (!e->vae_plan_for(PD_VAE_SD3, H, W, dn, true).tiled && !e->vae_flash_on(v.d, v.attn.C, (long long)(H / dn) * (W / dn)) && ((H / dn) * (W / dn)) % 8) {
        pd_set_error("pd_sd3_vae_encode: (H/%d)*(W/%d) must be a multiple of 8 where the mid-block attention materialises its scores (got %d x %d)", dn, dn, H, W);
        return 1;
    }
    if (what != PD_VAE_MEAN && what != PD_VAE_SAMPLE && what != PD_VAE_MOMENTS) {
        pd_set_error("pd_sd3_vae_encode: unknown `what` %d (PD_VAE_MEAN / PD_VAE_SAMPLE / PD_VAE_MOMENTS)", what);
        return 1;
    }
    return e->vae_encode_call(v, PD_VAE_SD3, images, B, H, W, mem, what, noise, raw ? 1.f : (float)v.d.scaling, raw ? 0.f : (float)v.d.shift, out);
}
