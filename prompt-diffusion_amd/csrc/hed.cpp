// pdengine: the HED edge detector (holistically-nested edge detection), the annotator behind the reference's apply_hed.
//   HEDdetector.__call__   annotator/hed/__init__.py:105-114   (RGB -> BGR, / 255; the uint8 ends stay in Python: annotators.py)
//   Network.forward        annotator/hed/__init__.py:71-93     (x * 255 - mean, VGG-16 trunk, five score heads, bilinear upsample to
//                                                               the input size, netCombine, sigmoid)
// The 13 conv3x3 + ReLU run on the engine's conv path (ACT_RELU: the ReLU instantiations of the shared epilogue); each stage ends in one hed_stage_tail launch
// (score head + 2x2 max-pool from one read of the feature map) and the whole tail of forward() is one hed_fuse launch (hed.hip).
#include "engine.h"

namespace {
const char* const kStage[5] = {"One", "Two", "Thr", "Fou", "Fiv"};
const int kConvs[5] = {2, 2, 3, 3, 3};
const int kWidth[5] = {64, 128, 256, 512, 512};
}  // namespace

// Registered in the order Network.__init__ creates the modules (= state_dict order): netVggOne .. netVggFiv, netScoreOne .. netScoreFiv,
// netCombine; "hed." + Network's own names (the checkpoint's "module" prefix is "net", :69)
void pd_engine::build_hed() {
    RegGroup rg(*this, GROUP_HED);
    HedW& v = hed;
    int ci = 0, cin = 3;
    for (int s = 0; s < 5; ++s) {
        const std::string p = std::string("hed.netVgg") + kStage[s] + ".";
        for (int j = 0; j < kConvs[s]; ++j) {
            // Sequential indices: stage one is conv, ReLU, conv, ReLU (0, 2); the others start with the MaxPool2d (1, 3, 5)
            const int idx = 2 * j + (s ? 1 : 0);
            build_conv(p + std::to_string(idx) + ".", v.conv[ci++], cin, kWidth[s], 3, 1);
            cin = kWidth[s];
        }
    }
    for (int s = 0; s < 5; ++s) {
        const std::string p = std::string("hed.netScore") + kStage[s] + ".";
        reg_vec(p + "weight", kWidth[s], &v.score_w[s], 'w');
        params.back().shape = {1, kWidth[s], 1, 1};
        reg_vec(p + "bias", 1, &v.score_b[s], 'b');
    }
    reg_vec("hed.netCombine.0.weight", 5, &v.comb_w, 'w');
    params.back().shape = {1, 5, 1, 1};
    reg_vec("hed.netCombine.0.bias", 1, &v.comb_b, 'b');
    v.built = true;
}

extern "C" int pd_hed_configure(pd_engine* e) {
    if (!e) { pd_set_error("bad argument"); return 1; }
    if (e->hed.built) return 0;
    return e->configure("pd_hed_configure", GROUP_HED, [&] { e->build_hed(); });
}

extern "C" int pd_hed_weights_missing(pd_engine* e) { return e ? e->missing(GROUP_HED) : 0; }

// Network.forward on [B, 3, H, W] RGB in [0, 1] (fp32, device) -> out [B, 1, H, W] (PD_HED_EDGE) or [B, 5, H, W] (PD_HED_SIDES)
int pd_engine::hed_forward(const float* images_dev, int B, int H, int W, int what, float* out_dev) {
    HedW& v = hed;
    // the feature maps alternate between two buffers of the largest layer's size: 64 channels at full resolution (every later layer
    // has twice the channels on a quarter of the pixels, or less)
    const size_t big = (size_t)B * H * W * kWidth[0] * dt_size(T);
    void* buf[2] = {arena.alloc(big), arena.alloc(big)};
    Act cur = new_act(B, H, W, v.conv[0].m.cin_pad, T);
    float* score[5];
    for (int s = 0; s < 5; ++s) score[s] = reinterpret_cast<float*>(arena.alloc((size_t)B * (H >> s) * (W >> s) * sizeof(float)));
    PD_LAUNCH(this, launch_hed_upload(images_dev, cur.p, T, B, H, W, cur.C, stream), "HED image upload launch failed");
    int which = 0, ci = 0, h = H, w = W;
    for (int s = 0; s < 5; ++s) {
        for (int j = 0; j < kConvs[s]; ++j) {
            const ConvW& c = v.conv[ci++];
            Act y;
            y.p = buf[which]; y.B = B; y.H = h; y.W = w; y.C = c.cout; y.dt = T;
            PD_TRY(conv(c, cur, y, {.act = ACT_RELU}));
            cur = y;
            which ^= 1;
        }
        const bool pool = s < 4;
        Act pooled = cur;
        pooled.p = buf[which]; pooled.H = h / 2; pooled.W = w / 2;
        PD_LAUNCH(this, launch_hed_stage_tail(cur.p, T, v.score_w[s], v.score_b[s], score[s], pool ? pooled.p : nullptr, B, h, w, cur.C, stream),
                  "HED stage-tail launch failed (stage %d, %d x %d x %d)", s + 1, h, w, cur.C);
        if (pool) {
            cur = pooled;
            which ^= 1;
            h /= 2; w /= 2;
        }
    }
    PD_LAUNCH(this, launch_hed_fuse(score, v.comb_w, v.comb_b, out_dev, B, H, W, what, stream), "HED fuse launch failed");
    return 0;
}

extern "C" int pd_hed_detect(pd_engine* e, const float* images, int32_t B, int32_t H, int32_t W, int32_t mem, int32_t what, float* out) {
    if (!e || !images || !out || B < 1 || H < 1 || W < 1) { pd_set_error("bad argument"); return 1; }
    if (!e->hed.built) { pd_set_error("this engine has no HED edge detector (pd_hed_configure)"); return 1; }
    PD_TRY(e->require_loaded(GROUP_HED, "HED"));
    if (e->ses.active) { pd_set_error("pd_hed_detect: end the sampling session first"); return 1; }
    if (H % 16 || W % 16) {
        pd_set_error("pd_hed_detect: H and W must be multiples of 16, the four 2x2 max-pools (got %d x %d; resize_image gives multiples of 64)", H, W);
        return 1;
    }
    if (what != PD_HED_EDGE && what != PD_HED_SIDES) {
        pd_set_error("pd_hed_detect: unknown `what` %d (PD_HED_EDGE / PD_HED_SIDES)", what);
        return 1;
    }
    if ((long long)B * H * W * 5 >= (1ll << 31)) { pd_set_error("pd_hed_detect: B * H * W too large (%d x %d x %d); split the batch", B, H, W); return 1; }
    HIP_OK(hipSetDevice(e->device));
    const size_t n_in = (size_t)B * 3 * H * W, n_out = (size_t)B * (what == PD_HED_SIDES ? 5 : 1) * H * W;
    return e->side_call("HED", [&](SideCall& f) {
        const float* src;
        PD_TRY(f.src(&src, images, n_in, mem));
        return e->hed_forward(src, B, H, W, what, f.dst(out, n_out, mem));
    });
}
