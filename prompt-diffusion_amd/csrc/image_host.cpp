// pdengine: the image ends of a call -- pd_resample_coefficients (Pillow's 8-bit resampling tables, host only), pd_image_load
// (uint8 NHWC pictures -> the engine's fp32 NCHW layout, resampled as Image.resize does it) and pd_image_store (fp32 NCHW -> uint8
// NHWC).  The kernels are in image_io.hip; the contract is in include/pdengine.h ("Image ends").
#include <cmath>

#include "engine.h"

namespace {

double sinc_filter(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return std::sin(x) / x;
}
double lanczos_filter(double x) { return (-3.0 <= x && x < 3.0) ? sinc_filter(x) * sinc_filter(x / 3) : 0.0; }
double box_filter(double x) { return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0; }
double bicubic_filter(double x) {   // Pillow's: a = -0.5
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// support of the filter, or 0 for an unknown one
double filter_support(int filter) {
    return filter == PD_RESAMPLE_LANCZOS ? 3.0 : filter == PD_RESAMPLE_BOX ? 0.5 : filter == PD_RESAMPLE_BICUBIC ? 2.0 : 0.0;
}

// bicubic: PD_RESAMPLE_BICUBIC is accepted too (pd_resample_coefficients_ex and the CLIP preprocessing; the older entries keep their two)
int check_axis(int in_size, int out_size, int filter, bool bicubic = false) {
    if (in_size < 1 || out_size < 1) { pd_set_error("resample: sizes must be >= 1 (got %d -> %d)", in_size, out_size); return 1; }
    if (filter_support(filter) == 0.0 || (filter == PD_RESAMPLE_BICUBIC && !bicubic)) {
        pd_set_error("resample: unknown filter %d (PD_RESAMPLE_LANCZOS / PD_RESAMPLE_BOX)", filter);
        return 1;
    }
    if ((long long)in_size > (long long)PD_RESAMPLE_MAX_SCALE * out_size) {
        pd_set_error("resample: %d -> %d reduces by more than PD_RESAMPLE_MAX_SCALE = %d", in_size, out_size, PD_RESAMPLE_MAX_SCALE);
        return 1;
    }
    return 0;
}

int axis_ksize(int in_size, int out_size, int filter) {
    double fs = (double)in_size / out_size;
    if (fs < 1.0) fs = 1.0;
    return (int)std::ceil(filter_support(filter) * fs) * 2 + 1;
}

// Resample.c: precompute_coeffs + normalize_coeffs_8bpc
void axis_tables(int in_size, int out_size, int filter, int ksize, int32_t* bounds, int32_t* kk) {
    double (*f)(double) = filter == PD_RESAMPLE_LANCZOS ? lanczos_filter : filter == PD_RESAMPLE_BICUBIC ? bicubic_filter : box_filter;
    const double scale = (double)in_size / out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = filter_support(filter) * fs;
    const double ss = 1.0 / fs;
    std::vector<double> w(ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = f((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int32_t* k = kk + (size_t)xx * ksize;
        for (int x = 0; x < ksize; ++x) {
            double v = x < xmax ? w[x] : 0.0;
            if (x < xmax && ww != 0.0) v /= ww;
            k[x] = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << 22)) : (int32_t)(0.5 + v * (double)(1 << 22));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

}  // namespace

extern "C" int pd_resample_coefficients(int32_t in_size, int32_t out_size, int32_t filter, int32_t* ksize, int32_t* bounds, int32_t* kk) {
    if (!ksize || (bounds == nullptr) != (kk == nullptr)) { pd_set_error("pd_resample_coefficients: bad argument"); return 1; }
    PD_TRY(check_axis(in_size, out_size, filter));
    *ksize = axis_ksize(in_size, out_size, filter);
    if (bounds) axis_tables(in_size, out_size, filter, *ksize, bounds, kk);
    return 0;
}

extern "C" int pd_resample_coefficients_ex(int32_t in_size, int32_t out_size, int32_t filter, int32_t* ksize, int32_t* bounds, int32_t* kk) {
    if (!ksize || (bounds == nullptr) != (kk == nullptr)) { pd_set_error("pd_resample_coefficients_ex: bad argument"); return 1; }
    PD_TRY(check_axis(in_size, out_size, filter, true));
    *ksize = axis_ksize(in_size, out_size, filter);
    if (bounds) axis_tables(in_size, out_size, filter, *ksize, bounds, kk);
    return 0;
}

int pd_resample_axis(int in_size, int out_size, int filter, int* ksize, std::vector<int32_t>& bounds, std::vector<int32_t>& kk) {
    PD_TRY(check_axis(in_size, out_size, filter, true));
    *ksize = axis_ksize(in_size, out_size, filter);
    bounds.assign((size_t)2 * out_size, 0);
    kk.assign((size_t)*ksize * out_size, 0);
    axis_tables(in_size, out_size, filter, *ksize, bounds.data(), kk.data());
    return 0;
}

int pd_engine::image_grow(ImageBuf& b, size_t bytes) {
    if (bytes <= b.cap) return 0;
    // (nothing of an earlier call is in flight: every image call synchronises the stream before it returns)
    if (b.p) { HIP_OK(hipStreamSynchronize(stream)); (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    HIP_OK(hipMalloc(&b.p, bytes));
    b.cap = bytes;
    ++image_allocs;
    return 0;
}

void pd_engine::image_release() {
    for (ImageBuf* b : {&img_u8, &img_tmp, &img_f32, &img_tab, &canny_states, &canny_flags, &clip_tmp, &clip_tab, &clip_out})
        if (b->p) { (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }
    if (canny_flags_host) { (void)hipHostFree(canny_flags_host); canny_flags_host = nullptr; }
}

extern "C" int pd_image_load(pd_engine* e, const pd_image_load_args* a) {
    if (!e || !a || !a->src || !a->dst) { pd_set_error("pd_image_load: null argument"); return 1; }
    const int Bs = a->Bs, Hs = a->Hs, Ws = a->Ws, B = a->B, C = a->C, H = a->H, W = a->W;
    if (Bs < 1 || B < 1 || C < 1 || B % Bs) { pd_set_error("pd_image_load: Bs = %d must divide B = %d (both >= 1), C = %d >= 1", Bs, B, C); return 1; }
    if (a->c_off < 0 || a->c_off + 3 > C) { pd_set_error("pd_image_load: channels %d .. %d do not fit C = %d", a->c_off, a->c_off + 2, C); return 1; }
    if (Bs != B && a->batch_mode != PD_IMAGE_REPEAT && a->batch_mode != PD_IMAGE_TILE) {
        pd_set_error("pd_image_load: unknown batch_mode %d (PD_IMAGE_REPEAT / PD_IMAGE_TILE)", a->batch_mode);
        return 1;
    }
    if (Hs < 1 || Ws < 1 || H < 1 || W < 1) { pd_set_error("pd_image_load: sizes must be >= 1 (%d x %d -> %d x %d)", Hs, Ws, H, W); return 1; }
    const bool need_h = Ws != W, need_v = Hs != H;
    if (need_h) PD_TRY(check_axis(Ws, W, a->filter));
    if (need_v) PD_TRY(check_axis(Hs, H, a->filter));
    HIP_OK(hipSetDevice(e->device));
    const size_t n_src = (size_t)Bs * Hs * Ws * 3, n_dst3 = (size_t)B * 3 * H * W;
    // tables: [bounds_h | kk_h | bounds_v | kk_v], rebuilt only when the shapes or the filter change
    const int ks_h = need_h ? axis_ksize(Ws, W, a->filter) : 0, ks_v = need_v ? axis_ksize(Hs, H, a->filter) : 0;
    const size_t off_kh = need_h ? (size_t)2 * W : 0, off_bv = off_kh + (size_t)ks_h * (need_h ? W : 0);
    const size_t off_kv = off_bv + (need_v ? (size_t)2 * H : 0), n_tab = off_kv + (size_t)ks_v * (need_v ? H : 0);
    if (n_tab) {
        const int32_t key[5] = {need_h ? Ws : 0, need_h ? W : 0, need_v ? Hs : 0, need_v ? H : 0, a->filter};
        bool same = e->img_tab.p != nullptr;
        for (int i = 0; i < 5; ++i) same = same && key[i] == e->img_tab_key[i];
        if (!same) {
            e->img_tab_host.assign(n_tab, 0);
            int32_t* t = e->img_tab_host.data();
            if (need_h) axis_tables(Ws, W, a->filter, ks_h, t, t + off_kh);
            if (need_v) axis_tables(Hs, H, a->filter, ks_v, t + off_bv, t + off_kv);
            for (int i = 0; i < 5; ++i) e->img_tab_key[i] = 0;
            PD_TRY(e->image_grow(e->img_tab, n_tab * sizeof(int32_t)));
            HIP_OK(hipMemcpyAsync(e->img_tab.p, t, n_tab * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
            for (int i = 0; i < 5; ++i) e->img_tab_key[i] = key[i];
        }
    }
    const int32_t* tab = reinterpret_cast<const int32_t*>(e->img_tab.p);
    const uint8_t* src = a->src;
    if (a->mem_src != PD_MEM_DEVICE) {
        PD_TRY(e->image_grow(e->img_u8, n_src));
        HIP_OK(hipMemcpyAsync(e->img_u8.p, a->src, n_src, hipMemcpyHostToDevice, e->stream));
        src = reinterpret_cast<const uint8_t*>(e->img_u8.p);
    }
    // a host destination: the three channels are made as a [B, 3, H, W] tensor on the device and copied into place
    float* dst = a->dst;
    int Cd = C, c_off = a->c_off;
    if (a->mem_dst != PD_MEM_DEVICE) {
        PD_TRY(e->image_grow(e->img_f32, n_dst3 * sizeof(float)));
        dst = reinterpret_cast<float*>(e->img_f32.p);
        Cd = 3;
        c_off = 0;
    }
    if (need_h) {
        PD_TRY(e->image_grow(e->img_tmp, (size_t)Bs * Hs * W * 3));
        ++e->launches;
        if (launch_image_hpass(src, reinterpret_cast<uint8_t*>(e->img_tmp.p), tab, tab + off_kh, ks_h, (long long)Bs * Hs, Ws, W, e->stream)) {
            pd_set_error("pd_image_load: horizontal pass launch failed");
            return 1;
        }
        src = reinterpret_cast<const uint8_t*>(e->img_tmp.p);
    }
    ++e->launches;
    if (launch_image_vpass(src, dst, need_v ? tab + off_bv : nullptr, need_v ? tab + off_kv : nullptr, ks_v, Bs, Hs, H, W, B, Cd, c_off,
                           Bs != B && a->batch_mode == PD_IMAGE_TILE, a->mul, a->add, e->stream)) {
        pd_set_error("pd_image_load: vertical pass / pack launch failed");
        return 1;
    }
    if (a->mem_dst != PD_MEM_DEVICE) {
        const size_t row = (size_t)3 * H * W * sizeof(float);
        HIP_OK(hipMemcpy2DAsync(a->dst + (size_t)a->c_off * H * W, (size_t)C * H * W * sizeof(float), dst, row, row, (size_t)B,
                                hipMemcpyDeviceToHost, e->stream));
    }
    HIP_OK(hipStreamSynchronize(e->stream));
    return 0;
}

extern "C" int pd_image_store(pd_engine* e, const float* src, int32_t B, int32_t C, int32_t H, int32_t W, int32_t mem_src, float mul,
                              float add, int32_t rounding, uint8_t* dst, int32_t mem_dst) {
    if (!e || !src || !dst) { pd_set_error("pd_image_store: null argument"); return 1; }
    if (B < 1 || H < 1 || W < 1 || (C != 1 && C != 3)) { pd_set_error("pd_image_store: [%d, %d, %d, %d]: sizes must be >= 1, C 1 or 3", B, C, H, W); return 1; }
    if (rounding != PD_ROUND_NEAREST_EVEN && rounding != PD_ROUND_TRUNC) {
        pd_set_error("pd_image_store: unknown rounding %d (PD_ROUND_NEAREST_EVEN / PD_ROUND_TRUNC)", rounding);
        return 1;
    }
    HIP_OK(hipSetDevice(e->device));
    const size_t n = (size_t)B * C * H * W;
    const float* s = src;
    if (mem_src != PD_MEM_DEVICE) {
        PD_TRY(e->image_grow(e->img_f32, n * sizeof(float)));
        HIP_OK(hipMemcpyAsync(e->img_f32.p, src, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
        s = reinterpret_cast<const float*>(e->img_f32.p);
    }
    uint8_t* d = dst;
    if (mem_dst != PD_MEM_DEVICE) {
        PD_TRY(e->image_grow(e->img_u8, n));
        d = reinterpret_cast<uint8_t*>(e->img_u8.p);
    }
    ++e->launches;
    if (launch_image_store(s, d, B, C, H, W, mul, add, rounding == PD_ROUND_TRUNC, e->stream)) { pd_set_error("pd_image_store: launch failed"); return 1; }
    if (mem_dst != PD_MEM_DEVICE) HIP_OK(hipMemcpyAsync(dst, d, n, hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    return 0;
}
