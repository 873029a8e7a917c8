// pdengine: the Canny edge detector, host side -- pd_canny (uint8 pictures -> the edge map as bytes and / or in the engine's fp32 NCHW
// layout) and the sweep loop of its hysteresis.  The kernels and the arithmetic are in canny.hip; the contract is in include/pdengine.h
// ("Canny edge detector").
#include <cmath>

#include "engine.h"

static_assert(CANNY_NONE == PD_CANNY_NONE && CANNY_WEAK == PD_CANNY_WEAK && CANNY_STRONG == PD_CANNY_STRONG, "pdengine.h");

// profiling classes of the launches (Bracket): 5 nms, 6 hysteresis sweep, 7 emit

// Sweeps are enqueued kCannyBatch at a time, sweep i of a batch raising flag i, and the flags are read from pinned memory after the
// batch.  A sweep that raised no flag found the fixed point (the sweeps behind it in the batch then change nothing either).  Every
// sweep before that one promoted at least one of the B * H * W pixels, which bounds the loop.
int pd_engine::canny_hysteresis(uint8_t* states_dev, int B, int H, int W) {
    canny_sweeps = 0;
    PD_TRY(image_grow(canny_flags, kCannyBatch * sizeof(int)));
    if (!canny_flags_host) {
        HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&canny_flags_host), kCannyBatch * sizeof(int), hipHostMallocDefault));
        ++image_allocs;
    }
    int* flags = reinterpret_cast<int*>(canny_flags.p);
    const long long bound = (long long)B * H * W + 1;
    while (canny_sweeps < bound) {
        HIP_OK(hipMemsetAsync(flags, 0, kCannyBatch * sizeof(int), stream));
        for (int i = 0; i < kCannyBatch; ++i) {
            Bracket br(this, 6);
            ++launches;
            ++canny_sweeps;
            if (launch_canny_hysteresis(states_dev, B, H, W, flags + i, stream)) { pd_set_error("canny: hysteresis launch failed"); return 1; }
        }
        HIP_OK(hipMemcpyAsync(canny_flags_host, flags, kCannyBatch * sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        for (int i = 0; i < kCannyBatch; ++i)
            if (!canny_flags_host[i]) return 0;
    }
    pd_set_error("canny: the hysteresis did not settle within %lld sweeps of a %d x %d x %d map (internal error)", canny_sweeps, B, H, W);
    return 1;
}

extern "C" int pd_canny(pd_engine* e, const pd_canny_args* a) {
    if (!e || !a || !a->src) { pd_set_error("pd_canny: null argument"); return 1; }
    if (!a->dst_u8 && !a->dst_f) { pd_set_error("pd_canny: no destination (dst_u8 and dst_f are both NULL)"); return 1; }
    const int B = a->B, H = a->H, W = a->W, C = a->C;
    if (B < 1 || H < 1 || W < 1 || (C != 1 && C != 3)) { pd_set_error("pd_canny: [%d, %d, %d, %d]: sizes must be >= 1, C 1 or 3", B, H, W, C); return 1; }
    if (a->dst_f && (a->c_off < 0 || a->c_off + 3 > a->Cf)) {
        pd_set_error("pd_canny: channels %d .. %d do not fit Cf = %d", a->c_off, a->c_off + 2, a->Cf);
        return 1;
    }
    if (!std::isfinite(a->low) || !std::isfinite(a->high)) { pd_set_error("pd_canny: thresholds must be finite"); return 1; }
    // floor, then clamp to what a magnitude can be compared with (m <= 2040: beyond either end the comparison no longer changes)
    auto threshold = [](float t) { const double f = std::floor((double)t); return (int)(f < -1.0 ? -1.0 : (f > 4096.0 ? 4096.0 : f)); };
    int lo = threshold(a->low), hi = threshold(a->high);
    if (lo > hi) std::swap(lo, hi);
    HIP_OK(hipSetDevice(e->device));
    const size_t n_px = (size_t)B * H * W;
    const uint8_t* src = a->src;
    if (a->mem_src != PD_MEM_DEVICE) {
        PD_TRY(e->image_grow(e->img_u8, n_px * C));
        HIP_OK(hipMemcpyAsync(e->img_u8.p, a->src, n_px * C, hipMemcpyHostToDevice, e->stream));
        src = reinterpret_cast<const uint8_t*>(e->img_u8.p);
    }
    PD_TRY(e->image_grow(e->canny_states, n_px));
    uint8_t* states = reinterpret_cast<uint8_t*>(e->canny_states.p);
    // host destinations: the bytes and the three channels (as a [B, 3, H, W] tensor) are made on the device and copied into place
    uint8_t* d8 = a->dst_u8;
    if (d8 && a->mem_u8 != PD_MEM_DEVICE) {
        PD_TRY(e->image_grow(e->img_tmp, n_px));
        d8 = reinterpret_cast<uint8_t*>(e->img_tmp.p);
    }
    float* df = a->dst_f;
    int Cf = a->Cf, c_off = a->c_off;
    if (df && a->mem_f != PD_MEM_DEVICE) {
        PD_TRY(e->image_grow(e->img_f32, n_px * 3 * sizeof(float)));
        df = reinterpret_cast<float*>(e->img_f32.p);
        Cf = 3;
        c_off = 0;
    }
    {
        Bracket br(e, 5);
        ++e->launches;
        if (launch_canny_nms(src, states, B, H, W, C, lo, hi, e->stream)) { pd_set_error("pd_canny: gradient / suppression launch failed"); return 1; }
    }
    PD_TRY(e->canny_hysteresis(states, B, H, W));
    {
        Bracket br(e, 7);
        ++e->launches;
        if (launch_canny_emit(states, d8, df, B, H, W, Cf, c_off, a->mul, a->add, e->stream)) { pd_set_error("pd_canny: emit launch failed"); return 1; }
    }
    if (d8 != a->dst_u8) HIP_OK(hipMemcpyAsync(a->dst_u8, d8, n_px, hipMemcpyDeviceToHost, e->stream));
    if (df != a->dst_f) {
        const size_t row = (size_t)3 * H * W * sizeof(float);
        HIP_OK(hipMemcpy2DAsync(a->dst_f + (size_t)a->c_off * H * W, (size_t)a->Cf * H * W * sizeof(float), df, row, row, (size_t)B,
                                hipMemcpyDeviceToHost, e->stream));
    }
    HIP_OK(hipStreamSynchronize(e->stream));
    return 0;
}
