// pdengine: the M-LSD line detector, the annotator behind the reference's "mlsd" task (the straight-line / "hough" condition map).
//   MLSDdetector.__call__            annotator/mlsd/__init__.py:27-39      (pred_lines, then cv2.line per segment)
//   pred_lines / deccode_output...   annotator/mlsd/utils.py:19-86         (x / 127.5 - 1 with a constant-one plane, the network, 3x3 NMS, top 200, thresholds)
//   MobileV2_MLSD_Large.forward      annotator/mlsd/models/mbv2_mlsd_large.py:275-292
// The 1x1 and 3x3 convolutions run on the engine's contraction path with every BatchNorm folded into them by the loader
// (Engine.load_mlsd_state_dict; a C host folds for itself).  ReLU6 = min(ReLU, 6): the contractions apply their ReLU epilogue and the only
// consumer of a ReLU6 output, a depthwise conv, clamps at 6 while loading (min of a stored value and 6 is exact, so the bits equal a ReLU6
// epilogue's).  BlockTypeB's conv1(x) + x is activation, then residual: the order the shared epilogue already has (pd_mma.h).  The
// depthwise convs, the align_corners upsample into the concat buffer, the peak decode and the rasteriser are mlsd.hip.
#include <cmath>

#include "engine.h"

namespace {

// profiling classes of the launches (Bracket): 8 depthwise conv, 9 the detector's other element-wise kernels, 10 decode + raster

// inverted_residual_setting of MobileNetV2.__init__ (:173-182): expansion t, width c, repeats n, first stride s
const int kSetting[5][4] = {{1, 16, 1, 1}, {6, 24, 2, 2}, {6, 32, 3, 2}, {6, 64, 4, 2}, {6, 96, 3, 1}};
const int kSkipC[4] = {64, 32, 24, 16};   // in_c1 of blocks 15, 17, 19, 21 (c4, c3, c2, c1)

}  // namespace

// conv + BatchNorm as the loader leaves them: the conv's weight under its own key, the folded bias under the BatchNorm's bias key
void pd_engine::build_conv_bn(const std::string& conv, const std::string& bn, ConvW& c, int cin, int cout, int k, int stride) {
    c.cin = cin; c.cout = cout; c.k = k; c.stride = stride;
    make_mat(c.m, cout, cin * k * k, k * k, cin, true);
    reg_mat(conv + "weight", {cout, cin, k, k}, &c.m, 0, true);
    reg_bias(bn + "bias", &c.m, 0, cout);
}

void pd_engine::build_dw_bn(const std::string& conv, const std::string& bn, MlsdDw& d, int C, int stride) {
    d.C = C; d.stride = stride;
    reg_vec(conv + "weight", C * 9, &d.w, 'w');
    params.back().shape = {C, 1, 3, 3};
    reg_vec(bn + "bias", C, &d.b, 'b');
}

// Registered in state_dict() order: per conv its weight, then the bias of the BatchNorm behind it (block23.conv3: its own bias)
void pd_engine::build_mlsd() {
    RegGroup rg(*this, GROUP_MLSD);
    MlsdW& v = mlsd;
    const std::string f = "mlsd.backbone.features.";
    build_conv_bn(f + "0.0.", f + "0.1.", v.conv0, 4, 32, 3, 2);
    v.conv0.pad_shift = 1;   // ConvBNReLU.forward: F.pad(x, (0, 1, 0, 1)) + padding 0 at stride 2
    int cin = 32, idx = 0;
    for (const auto& st : kSetting)
        for (int i = 0; i < st[2]; ++i) {
            MlsdIR& r = v.ir[idx];
            const std::string p = f + std::to_string(idx + 1) + ".conv.";
            const int stride = i == 0 ? st[3] : 1, hidden = cin * st[0], cout = st[1];
            r.expand = st[0] != 1;
            r.res = stride == 1 && cin == cout;
            int j = 0;
            if (r.expand) { build_conv_bn(p + "0.0.", p + "0.1.", r.pw1, cin, hidden, 1, 1); j = 1; }
            build_dw_bn(p + std::to_string(j) + ".0.", p + std::to_string(j) + ".1.", r.dw, hidden, stride);
            build_conv_bn(p + std::to_string(j + 1) + ".", p + std::to_string(j + 2) + ".", r.pw2, hidden, cout, 1, 1);
            cin = cout;
            ++idx;
        }
    for (int j = 0; j < 4; ++j) {
        const std::string a = "mlsd.block" + std::to_string(15 + 2 * j) + ".", b = "mlsd.block" + std::to_string(16 + 2 * j) + ".";
        build_conv_bn(a + "conv1.0.", a + "conv1.1.", v.a1[j], j == 0 ? 96 : 64, 64, 1, 1);
        build_conv_bn(a + "conv2.0.", a + "conv2.1.", v.a2[j], kSkipC[j], 64, 1, 1);
        build_conv_bn(b + "conv1.0.", b + "conv1.1.", v.b1[j], 128, 128, 3, 1);
        build_conv_bn(b + "conv2.0.", b + "conv2.1.", v.b2[j], 128, 64, 3, 1);
    }
    build_conv_bn("mlsd.block23.conv1.0.", "mlsd.block23.conv1.1.", v.c1, 64, 64, 3, 1);
    v.c1.dilation = 5;
    build_conv_bn("mlsd.block23.conv2.0.", "mlsd.block23.conv2.1.", v.c2, 64, 64, 3, 1);
    build_conv("mlsd.block23.conv3.", v.c3, 64, 16, 1, 1);
    v.built = true;
}

extern "C" int pd_mlsd_configure(pd_engine* e) {
    if (!e) { pd_set_error("bad argument"); return 1; }
    if (e->mlsd.built) return 0;
    return e->configure("pd_mlsd_configure", GROUP_MLSD, [&] { e->build_mlsd(); });
}

extern "C" int pd_mlsd_weights_missing(pd_engine* e) { return e ? e->missing(GROUP_MLSD) : 0; }

int pd_engine::mlsd_dwconv(const MlsdDw& d, const Act& x, Act& y) {
    if (x.C != d.C || y.C != d.C || x.dt != T || y.dt != T) { pd_set_error("internal: M-LSD depthwise conv over %d / %d channels, layer has %d", x.C, y.C, d.C); return 1; }
    if (arena.dry) return 0;
    PD_TRY(check_arena());
    Bracket br(this, 8);
    br.rec.M = (int)y.rows(); br.rec.N = d.C; br.rec.K = 9; br.rec.taps = 90 + d.stride;   // (pd_profile_dump: output pixels, channels, stride)
    ++launches;
    if (launch_mlsd_dwconv(x.p, y.p, T, d.w, d.b, x.B, x.H, x.W, d.C, d.stride, 1, stream)) {
        pd_set_error("M-LSD depthwise conv launch failed (%d x %d x %d, stride %d)", x.H, x.W, d.C, d.stride);
        return 1;
    }
    return 0;
}

// MobileV2_MLSD_Large.forward on uint8 RGB pictures [B][H][W][3] (device) -> tp [B][9][H/2][W/2] fp32 (device)
int pd_engine::mlsd_forward(const uint8_t* images_dev, int B, int H, int W, float* tp_dev) {
    MlsdW& v = mlsd;
    const size_t es = dt_size(T);
    Act x0 = new_act(B, H, W, 8, T);
    PD_LAUNCH_K(this, 1, 9, launch_mlsd_upload(images_dev, x0.p, T, B, H, W, stream), "M-LSD image upload launch failed");
    Act cur = new_act(B, H / 2, W / 2, 32, T);
    PD_TRY(conv(v.conv0, x0, cur, {.act = ACT_RELU}));
    Act tap[5];
    int ntap = 0;
    for (int i = 0; i < 13; ++i) {
        const MlsdIR& r = v.ir[i];
        const int s = r.dw.stride;
        Act out = new_act(B, cur.H / s, cur.W / s, r.pw2.cout, T);
        const size_t mk = arena.mark();   // the block's hidden tensors die with it (stream-ordered)
        Act hid = cur;
        if (r.expand) {
            hid = new_act(B, cur.H, cur.W, r.pw1.cout, T);
            PD_TRY(conv(r.pw1, cur, hid, {.act = ACT_RELU}));
        }
        Act d = new_act(B, cur.H / s, cur.W / s, r.dw.C, T);
        PD_TRY(mlsd_dwconv(r.dw, hid, d));
        PD_TRY(conv(r.pw2, d, out, {.R = r.res ? &cur : nullptr}));
        arena.release(mk);
        cur = out;
        const int fi = i + 1;   // fpn_selected = [1, 3, 6, 10, 13]
        if (fi == 1 || fi == 3 || fi == 6 || fi == 10 || fi == 13) tap[ntap++] = cur;
    }
    Act x = tap[4];
    for (int j = 0; j < 4; ++j) {
        const Act& skip = tap[3 - j];
        Act y2 = new_act(B, skip.H, skip.W, 64, T);
        const size_t mk = arena.mark();
        // BlockTypeA: cat(conv2(skip), up(conv1(x))) -- both halves are written in place, the concatenated tensor is never copied
        Act cat = new_act(B, skip.H, skip.W, 128, T);
        Act lo = cat, hi = cat;
        lo.C = hi.C = 64;
        hi.p = reinterpret_cast<char*>(cat.p) + 64 * es;
        PD_TRY(conv(v.a2[j], skip, lo, {.act = ACT_RELU, .ldc = 128}));
        if (j == 0) {   // block15: upscale = False
            PD_TRY(conv(v.a1[j], x, hi, {.act = ACT_RELU, .ldc = 128}));
        } else {
            Act t = new_act(B, x.H, x.W, 64, T);
            PD_TRY(conv(v.a1[j], x, t, {.act = ACT_RELU}));
            PD_LAUNCH_K(this, 1, 9, launch_mlsd_upcat(t.p, 64, hi.p, 128, T, B, x.H, x.W, 64, stream), "M-LSD upsample launch failed (block %d)", 15 + 2 * j);
        }
        // BlockTypeB: conv2(conv1(x) + x), ReLU inside both convs
        Act y1 = new_act(B, skip.H, skip.W, 128, T);
        PD_TRY(conv(v.b1[j], cat, y1, {.act = ACT_RELU, .R = &cat}));
        PD_TRY(conv(v.b2[j], y1, y2, {.act = ACT_RELU}));
        arena.release(mk);
        x = y2;
    }
    Act z1 = new_act(B, x.H, x.W, 64, T), z2 = new_act(B, x.H, x.W, 64, T), z3 = new_act(B, x.H, x.W, 16, DT_F32);
    PD_TRY(conv(v.c1, x, z1, {.act = ACT_RELU}));
    PD_TRY(conv(v.c2, z1, z2, {.act = ACT_RELU}));
    PD_TRY(conv(v.c3, z2, z3));
    PD_LAUNCH_K(this, 1, 9, launch_mlsd_tpmap(reinterpret_cast<const float*>(z3.p), tp_dev, B, x.H, x.W, stream), "M-LSD output launch failed");
    return 0;
}

int pd_engine::mlsd_decode(const float* tp_dev, int B, int h, int w, float thr_v, float thr_d, int* segs_dev, int* count_dev) {
    unsigned long long* cand = reinterpret_cast<unsigned long long*>(arena.alloc((size_t)B * h * w * sizeof(unsigned long long)));
    int* ncand = reinterpret_cast<int*>(arena.alloc((size_t)B * sizeof(int)));
    PD_LAUNCH_K(this, 2, 10, launch_mlsd_decode(tp_dev, cand, ncand, segs_dev, count_dev, B, h, w, thr_v, thr_d, stream), "M-LSD decode launch failed");
    return 0;
}

extern "C" int pd_mlsd_detect_ex(pd_engine* e, const pd_mlsd_args* a) {
    if (!e || !a || !a->images) { pd_set_error("pd_mlsd_detect: null argument"); return 1; }
    const int B = a->B, H = a->H, W = a->W, what = a->what;
    if (B < 1 || H < 1 || W < 1) { pd_set_error("pd_mlsd_detect: [%d, %d, %d]: sizes must be >= 1", B, H, W); return 1; }
    if (!e->mlsd.built) { pd_set_error("this engine has no M-LSD line detector (pd_mlsd_configure)"); return 1; }
    PD_TRY(e->require_loaded(GROUP_MLSD, "M-LSD"));
    if (e->ses.active) { pd_set_error("pd_mlsd_detect: end the sampling session first"); return 1; }
    if (H % 32 || W % 32) {
        pd_set_error("pd_mlsd_detect: H and W must be multiples of 32, the five stride-2 layers (got %d x %d; resize_image gives multiples of 64)", H, W);
        return 1;
    }
    if (what != PD_MLSD_TPMAP && what != PD_MLSD_SEGMENTS && what != PD_MLSD_LINES) {
        pd_set_error("pd_mlsd_detect: unknown `what` %d (PD_MLSD_TPMAP / PD_MLSD_SEGMENTS / PD_MLSD_LINES)", what);
        return 1;
    }
    const bool lines = what == PD_MLSD_LINES;
    if (!a->out && !(lines && a->dst_f)) { pd_set_error("pd_mlsd_detect: no destination"); return 1; }
    if (a->dst_f && !lines) { pd_set_error("pd_mlsd_detect: dst_f goes with PD_MLSD_LINES"); return 1; }
    if (a->dst_f && (a->c_off < 0 || a->c_off + 3 > a->Cf)) { pd_set_error("pd_mlsd_detect: channels %d .. %d do not fit Cf = %d", a->c_off, a->c_off + 2, a->Cf); return 1; }
    if (what != PD_MLSD_TPMAP) {
        // a score of exactly 0 is what the reference's top-k gives the non-peaks it pads with: below zero they would all pass
        if (!std::isfinite(a->thr_v) || !std::isfinite(a->thr_d) || a->thr_v < 0.f) { pd_set_error("pd_mlsd_detect: thresholds must be finite and thr_v >= 0"); return 1; }
    }
    if ((long long)B * H * W * 96 >= (1ll << 31)) { pd_set_error("pd_mlsd_detect: B * H * W too large (%d x %d x %d); split the batch", B, H, W); return 1; }
    HIP_OK(hipSetDevice(e->device));
    const int h = H / 2, w = W / 2;
    const size_t n_px = (size_t)B * H * W, n_tp = (size_t)B * 9 * h * w, n_seg = (size_t)B * MLSD_TOPK * 4;
    const bool dev = a->mem == PD_MEM_DEVICE;
    const bool f_host = a->dst_f && a->mem_f != PD_MEM_DEVICE;
    return e->side_call("M-LSD", [&](SideCall& f) {
        const uint8_t* src;
        PD_TRY(f.src(&src, a->images, n_px * 3, a->mem));
        // a device destination is written by the kernels themselves (tp-map, byte map); everything else is staged
        float* tp = what != PD_MLSD_TPMAP ? f.scratch<float>(n_tp) : dev ? reinterpret_cast<float*>(a->out) : f.dst(reinterpret_cast<float*>(a->out), n_tp, a->mem);
        PD_TRY(e->mlsd_forward(src, B, H, W, tp));
        if (what == PD_MLSD_TPMAP) return 0;
        // [B][200][4], then the B counts
        int* segs = what == PD_MLSD_SEGMENTS ? f.dst(reinterpret_cast<int*>(a->out), n_seg + B, a->mem) : f.scratch<int>(n_seg + B);
        int* count = segs + n_seg;
        PD_TRY(e->mlsd_decode(tp, B, h, w, a->thr_v, a->thr_d, segs, count));
        if (what == PD_MLSD_SEGMENTS) return 0;
        uint8_t* map = f.scratch<uint8_t>(n_px);
        uint8_t* o8 = reinterpret_cast<uint8_t*>(a->out);
        if (o8 && !dev) o8 = f.dst(o8, n_px, a->mem);
        float* df = a->dst_f;
        int Cf = a->Cf, c_off = a->c_off;
        if (f_host) {   // the three channels as a [B, 3, H, W] tensor, copied into channels c_off .. of the caller's Cf
            df = f.dst(a->dst_f + (size_t)a->c_off * H * W, (size_t)3 * H * W, a->mem_f, (size_t)B, (size_t)a->Cf * H * W);
            Cf = 3; c_off = 0;
        }
        if (!e->arena.dry) {   // both launches under one bracket
            PD_TRY(e->check_arena());
            Bracket br(e, 10);
            e->launches += 2;
            if (launch_mlsd_draw(segs, count, MLSD_TOPK, map, B, H, W, e->stream)) { pd_set_error("pd_mlsd_detect: raster launch failed"); return 1; }
            if (launch_canny_emit(map, o8, df, B, H, W, Cf, c_off, a->mul, a->add, e->stream)) { pd_set_error("pd_mlsd_detect: emit launch failed"); return 1; }
        }
        return 0;
    });
}

extern "C" int pd_mlsd_detect(pd_engine* e, const uint8_t* images, int32_t B, int32_t H, int32_t W, int32_t mem, int32_t what, float thr_v,
                              float thr_d, void* out) {
    pd_mlsd_args a{};
    a.images = images; a.B = B; a.H = H; a.W = W; a.mem = mem; a.what = what; a.thr_v = thr_v; a.thr_d = thr_d; a.out = out;
    a.mul = 1.f;
    return pd_mlsd_detect_ex(e, &a);
}
