// Per-operator parity hooks (declared in include/pdengine_ops.h): run ONE kernel of the hot path on
// host arrays in the reference's own layouts, so tests/ can compare each HIP kernel with the oracle.
// Not used by the sampling path.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pdengine_ops.h"
#include "engine.h"

namespace {
struct DevBuf {
    void* p = nullptr;
    explicit DevBuf(size_t bytes) { if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) p = nullptr; else { hipMemset(p, 0, bytes ? bytes : 16); hipDeviceSynchronize(); } }
    ~DevBuf() { if (p) hipFree(p); }
};
struct TempMat {
    pd_engine* e;
    size_t owned0;
    explicit TempMat(pd_engine* e_) : e(e_), owned0(e_->owned.size()) {}
    ~TempMat() {
        while (e->owned.size() > owned0) { hipFree(e->owned.back()); e->owned.pop_back(); }
    }
};
int to_dev_nhwc(pd_engine* e, const float* host, void* dst, int dt, int B, int C, int H, int W, int Cpad) {
    DevBuf tmp((size_t)B * C * H * W * 4);
    if (!tmp.p) return 1;
    HIP_OK(hipMemcpy(tmp.p, host, (size_t)B * C * H * W * 4, hipMemcpyHostToDevice));
    if (launch_nchw_to_nhwc(reinterpret_cast<const float*>(tmp.p), dst, dt, B, C, H, W, Cpad, e->stream)) return 1;
    HIP_OK(hipStreamSynchronize(e->stream));
    return 0;
}
int from_dev_nhwc(pd_engine* e, const void* src, int dt, float* host, int B, int C, int H, int W, int Cpad) {
    DevBuf tmp((size_t)B * C * H * W * 4);
    if (!tmp.p) return 1;
    if (launch_nhwc_to_nchw(src, dt, reinterpret_cast<float*>(tmp.p), B, C, H, W, Cpad, 1.f, e->stream)) return 1;
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(host, tmp.p, (size_t)B * C * H * W * 4, hipMemcpyDeviceToHost));
    return 0;
}
int round_up(int x, int m) { return (x + m - 1) / m * m; }
}  // namespace

extern "C" {

// y = conv2d(x, w, b, stride, padding = k/2) [+ SiLU] [* scale] [+ residual]; x NCHW fp32, w OIHW.
int pd_op_conv2d(pd_engine* e, const float* x, const float* w, const float* bias, const float* residual, int B, int Cin, int H,
                 int W, int Cout, int k, int stride, int upsample, int act_silu, float scale, int stream_out, float* y) {
    return pd_op_conv2d_ex(e, x, w, bias, residual, nullptr, B, Cin, H, W, Cout, k, stride, upsample, act_silu ? ACT_SILU : ACT_NONE, scale, stream_out, y);
}

// ... with the per-sample row of a ResBlock's time embedding (rowvec [B][Cout]) and act 0 / 1 / 5 (none / SiLU / ReLU)
int pd_op_conv2d_ex(pd_engine* e, const float* x, const float* w, const float* bias, const float* residual, const float* rowvec, int B, int Cin,
                    int H, int W, int Cout, int k, int stride, int upsample, int act, float scale, int stream_out, float* y) {
    if (!e || !x || !w || !y) { pd_set_error("null argument"); return 1; }
    if (act != ACT_NONE && act != ACT_SILU && act != ACT_RELU) { pd_set_error("pd_op_conv2d_ex: act %d (a conv takes 0 none, 1 SiLU, 5 ReLU)", act); return 1; }
    HIP_OK(hipSetDevice(e->device));
    TempMat guard(e);
    ConvW c;
    c.cin = Cin; c.cout = Cout; c.k = k; c.stride = stride;
    e->make_mat(c.m, Cout, Cin * k * k, k * k, Cin, true);
    if (!c.m.w) { pd_set_error("allocation failed"); return 1; }
    PD_TRY(e->upload_rows(c.m, 0, w, Cout, true));
    if (bias) PD_TRY(e->upload_vec(c.m.bias, bias, Cout, false, 0));
    const int Hv = H << upsample, Wv = W << upsample;
    const int Ho = stride == 2 ? (Hv + 1) / 2 : Hv, Wo = stride == 2 ? (Wv + 1) / 2 : Wv;
    const int cpad = c.m.cin_pad, odt = stream_out ? e->S : e->T, copad = round_up(Cout, 4);
    DevBuf in((size_t)B * H * W * cpad * dt_size(e->T)), out((size_t)B * Ho * Wo * copad * dt_size(odt)),
        res((size_t)B * Ho * Wo * copad * dt_size(e->S));
    if (!in.p || !out.p || !res.p) { pd_set_error("allocation failed"); return 1; }
    PD_TRY(to_dev_nhwc(e, x, in.p, e->T, B, Cin, H, W, cpad));
    Act a, o, r;
    a.p = in.p; a.B = B; a.H = H; a.W = W; a.C = cpad; a.dt = e->T;
    o.p = out.p; o.B = B; o.H = Ho; o.W = Wo; o.C = copad; o.dt = odt;
    r = o; r.p = res.p; r.dt = e->S;
    if (residual) PD_TRY(to_dev_nhwc(e, residual, res.p, e->S, B, Cout, Ho, Wo, copad));
    DevBuf rv((size_t)B * copad * 4);   // (DevBuf zero-fills: the pad columns of the row)
    if (!rv.p) { pd_set_error("allocation failed"); return 1; }
    if (rowvec) HIP_OK(hipMemcpy2D(rv.p, (size_t)copad * 4, rowvec, (size_t)Cout * 4, (size_t)Cout * 4, B, hipMemcpyHostToDevice));
    PD_TRY(e->conv(c, a, o, {.ups = upsample, .act = (Activation)act, .scale = scale, .R = residual ? &r : nullptr,
                             .rowvec = rowvec ? reinterpret_cast<const float*>(rv.p) : nullptr, .rowvec_stride = rowvec ? copad : 0}));
    return from_dev_nhwc(e, out.p, odt, y, B, Cout, Ho, Wo, copad);
}

// y = conv3x3(nearest_x2(x)) + bias [+ residual] through fold_upconv and the dispatch; an error unless the plan is the four-phase kernel
int pd_op_conv2d_upfold(pd_engine* e, const float* x, const float* w, const float* bias, const float* residual, int B, int Cin, int H,
                        int W, int Cout, float* y) {
    if (!e || !x || !w || !y) { pd_set_error("null argument"); return 1; }
    if (B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1) { pd_set_error("pd_op_conv2d_upfold: need B, Cin, Cout, H, W >= 1"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    TempMat guard(e);
    ConvW c;
    c.cin = Cin; c.cout = Cout; c.k = 3; c.stride = 1;
    e->make_mat(c.m, Cout, Cin * 9, 9, Cin, true);
    if (!c.m.w) { pd_set_error("allocation failed"); return 1; }
    PD_TRY(e->upload_rows(c.m, 0, w, Cout, true));
    if (bias) PD_TRY(e->upload_vec(c.m.bias, bias, Cout, false, 0));
    PD_TRY(e->fold_upconv(c.m));
    const int Ho = 2 * H, Wo = 2 * W;
    const int cpad = c.m.cin_pad, copad = round_up(Cout, 4);
    DevBuf in((size_t)B * H * W * cpad * dt_size(e->T)), out((size_t)B * Ho * Wo * copad * dt_size(e->T)),
        res((size_t)B * Ho * Wo * copad * dt_size(e->S));
    if (!in.p || !out.p || !res.p) { pd_set_error("allocation failed"); return 1; }
    PD_TRY(to_dev_nhwc(e, x, in.p, e->T, B, Cin, H, W, cpad));
    Act a, o, r;
    a.p = in.p; a.B = B; a.H = H; a.W = W; a.C = cpad; a.dt = e->T;
    o.p = out.p; o.B = B; o.H = Ho; o.W = Wo; o.C = copad; o.dt = e->T;
    r = o; r.p = res.p; r.dt = e->S;
    if (residual) PD_TRY(to_dev_nhwc(e, residual, res.p, e->S, B, Cout, Ho, Wo, copad));
    GemmCall call{.ups = 1, .R = residual ? &r : nullptr};
    PD_TRY(e->check_gemm(c.m, a, o, call));
    if (e->plan_gemm(e->fill_gemm(c.m, a, o, call), c.m, call).family != GEMM_UPFOLD) {
        pd_set_error("pd_op_conv2d_upfold: B %d Cin %d %dx%d Cout %d%s is not eligible for the four-phase upsample conv (mode, options, shape or epilogue)", B, Cin,
                     H, W, Cout, residual ? " + residual" : "");
        return 1;
    }
    PD_TRY(e->conv(c, a, o, call));
    return from_dev_nhwc(e, out.p, e->T, y, B, Cout, Ho, Wo, copad);
}

// y = Downsample(x) of the KL-VAE encoder: zero row / column appended at the bottom / right, then conv3x3 stride 2 padding 0
int pd_op_vae_downsample(pd_engine* e, const float* x, const float* w, const float* bias, int B, int C, int H, int W, float* y) {
    if (!e || !x || !w || !y) { pd_set_error("null argument"); return 1; }
    if (B < 1 || C < 1 || H < 2 || W < 2) { pd_set_error("pd_op_vae_downsample: need B, C >= 1 and H, W >= 2"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    TempMat guard(e);
    ConvW c;
    c.cin = C; c.cout = C; c.k = 3; c.stride = 2; c.pad_shift = 1;
    e->make_mat(c.m, C, C * 9, 9, C, true);
    if (!c.m.w) { pd_set_error("allocation failed"); return 1; }
    PD_TRY(e->upload_rows(c.m, 0, w, C, true));
    if (bias) PD_TRY(e->upload_vec(c.m.bias, bias, C, false, 0));
    const int Ho = H / 2, Wo = W / 2;   // (H + 1 - 3) / 2 + 1
    const int cpad = c.m.cin_pad, copad = round_up(C, 4);
    DevBuf in((size_t)B * H * W * cpad * dt_size(e->T)), out((size_t)B * Ho * Wo * copad * dt_size(e->T));
    if (!in.p || !out.p) { pd_set_error("allocation failed"); return 1; }
    PD_TRY(to_dev_nhwc(e, x, in.p, e->T, B, C, H, W, cpad));
    Act a, o;
    a.p = in.p; a.B = B; a.H = H; a.W = W; a.C = cpad; a.dt = e->T;
    o.p = out.p; o.B = B; o.H = Ho; o.W = Wo; o.C = copad; o.dt = e->T;
    PD_TRY(e->conv(c, a, o));
    return from_dev_nhwc(e, out.p, e->T, y, B, C, Ho, Wo, copad);
}

// The FreeU skip concat of a decoder block (launch_freeu_concat) in the residual-stream type: NCHW fp32 in and out
int pd_op_freeu_concat(pd_engine* e, const float* h, const float* h_add, const float* skip, const float* skip_add, int B, int C_h,
                       int C_skip, int H, int W, int skip_B, int skip_add_B, float s, float b, float* y) {
    if (!e || !h || !skip || !y) { pd_set_error("null argument"); return 1; }
    if (B < 1 || H < 1 || W < 1 || C_h < 4 || C_skip < 4 || C_h % 4 || C_skip % 4) {
        pd_set_error("pd_op_freeu_concat: need B, H, W >= 1 and C_h, C_skip positive multiples of 4");
        return 1;
    }
    if ((skip_B != B && 2 * skip_B != B) || (skip_add && skip_add_B != B && 2 * skip_add_B != B)) {
        pd_set_error("pd_op_freeu_concat: skip_B / skip_add_B must be B or B / 2");
        return 1;
    }
    HIP_OK(hipSetDevice(e->device));
    const int dt = e->S;
    const size_t px = (size_t)H * W, es = dt_size(dt);
    DevBuf dh((size_t)B * px * C_h * es), dha((size_t)B * px * C_h * es), ds((size_t)skip_B * px * C_skip * es),
        dsa((size_t)(skip_add ? skip_add_B : 1) * px * C_skip * es), dy((size_t)B * px * (C_h + C_skip) * es);
    if (!dh.p || !dha.p || !ds.p || !dsa.p || !dy.p) { pd_set_error("allocation failed"); return 1; }
    PD_TRY(to_dev_nhwc(e, h, dh.p, dt, B, C_h, H, W, C_h));
    if (h_add) PD_TRY(to_dev_nhwc(e, h_add, dha.p, dt, B, C_h, H, W, C_h));
    PD_TRY(to_dev_nhwc(e, skip, ds.p, dt, skip_B, C_skip, H, W, C_skip));
    if (skip_add) PD_TRY(to_dev_nhwc(e, skip_add, dsa.p, dt, skip_add_B, C_skip, H, W, C_skip));
    if (launch_freeu_concat(dh.p, h_add ? dha.p : nullptr, ds.p, skip_add ? dsa.p : nullptr, dy.p, dt, B, H, W, C_h, C_skip, s, b,
                            e->stream, (long long)skip_B * px, skip_add ? (long long)skip_add_B * px : 0)) {
        pd_set_error("pd_op_freeu_concat: launch failed");
        return 1;
    }
    return from_dev_nhwc(e, dy.p, dt, y, B, C_h + C_skip, H, W, C_h + C_skip);
}

// y[M,N] = act(x[M,K] @ w[N,K]^T + b) ; geglu: w [2*N, K] -> y[M,N] = (x w_a + b_a) * gelu(x w_g + b_g)
int pd_op_linear(pd_engine* e, const float* x, const float* w, const float* bias, int M, int K, int N, int geglu, int a_silu,
                 float* y) {
    pd_gemm_ex_args a{};
    a.x = x; a.w = w; a.bias = bias; a.M = M; a.K = K; a.N = N; a.act = geglu ? ACT_GEGLU : ACT_NONE; a.a_silu = a_silu; a.y = y;
    return pd_op_linear_ex(e, &a);
}

namespace {
int ex_dt(const pd_engine* e, int code) { return code == 1 ? e->T : code == 2 ? e->S : DT_F32; }
// host fp32 -> a device buffer of n elements in dt, and back
int put_flat(pd_engine* e, const std::vector<float>& host, void* dst, int dt) {
    DevBuf tmp(host.size() * 4);
    if (!tmp.p) { pd_set_error("allocation failed"); return 1; }
    HIP_OK(hipMemcpy(tmp.p, host.data(), host.size() * 4, hipMemcpyHostToDevice));
    if (launch_cast_rows(reinterpret_cast<const float*>(tmp.p), dst, dt, 1, (int)host.size(), (int)host.size(), e->stream)) { pd_set_error("cast launch failed"); return 1; }
    HIP_OK(hipStreamSynchronize(e->stream));
    return 0;
}
int get_flat(pd_engine* e, const void* src, int dt, std::vector<float>& host) {
    DevBuf tmp(host.size() * 4);
    if (!tmp.p) { pd_set_error("allocation failed"); return 1; }
    if (launch_nhwc_to_nchw(src, dt, reinterpret_cast<float*>(tmp.p), 1, 1, 1, (int)host.size(), 1, 1.f, e->stream)) { pd_set_error("cast launch failed"); return 1; }
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(host.data(), tmp.p, host.size() * 4, hipMemcpyDeviceToHost));
    return 0;
}
}  // namespace

// pd_engine::gemm on a linear layer with everything its callers pass (see pdengine_ops.h): activation, scale, residual in any of its types,
// 2-byte output, per-sample row / gate, the V^T side output, joint-buffer row remaps of C and A, an output row stride, and a NaN fill of
// every output element the launch must leave alone
int pd_op_linear_ex(pd_engine* e, pd_gemm_ex_args* g) {
    if (!e || !g || !g->x || !g->w || !g->y) { pd_set_error("null argument"); return 1; }
    const int M = g->M, K = g->K, N = g->N, act = g->act;
    if (M < 1 || K < 1 || N < 1) { pd_set_error("pd_op_linear_ex: need M, K, N >= 1"); return 1; }
    if (K % 8) { pd_set_error("K must be a multiple of 8"); return 1; }
    if (act < 0 || act > ACT_GATED_TANH_GELU) { pd_set_error("pd_op_linear_ex: act %d out of range", act); return 1; }
    const bool packed = act == ACT_GEGLU || act == ACT_GATED_TANH_GELU;
    const int tokens = g->rows_per_sample > 0 ? g->rows_per_sample : M;
    if (M % tokens) { pd_set_error("pd_op_linear_ex: M %d is no multiple of rows_per_sample %d", M, tokens); return 1; }
    const int B = M / tokens;
    const float scale = g->scale == 0.f ? 1.f : g->scale;
    const bool remap = g->c_sample_rows || g->a_sample_rows;
    const bool side = g->residual || g->rowvec || g->gate || g->vt_begin || remap || g->ldc_extra || g->out_dt;
    if (N % 4 && side) { pd_set_error("pd_op_linear_ex: N %d must be a multiple of 4 with anything beyond bias / activation", N); return 1; }
    if ((unsigned)g->res_dt > 2u || (unsigned)g->out_dt > 2u) { pd_set_error("pd_op_linear_ex: dtype codes are 0 fp32, 1 compute type, 2 stream type"); return 1; }
    if (g->vt_begin) {
        if (g->vt_begin < 0 || g->vt_begin % 4 || g->vt_begin >= N) { pd_set_error("pd_op_linear_ex: vt_begin %d must be a multiple of 4 in (0, N)", g->vt_begin); return 1; }
        if (!g->vt || g->vt_extra < 0 || g->vt_extra % 8 || g->vt_tok_off < 0) { pd_set_error("pd_op_linear_ex: V^T needs an output array, vt_extra a multiple of 8, vt_tok_off >= 0"); return 1; }
    } else if (g->vt_extra || g->vt_tok_off) { pd_set_error("pd_op_linear_ex: vt_extra / vt_tok_off without vt_begin"); return 1; }
    if (g->ldc_extra < 0 || g->ldc_extra % 4) { pd_set_error("pd_op_linear_ex: ldc_extra %d must be a non-negative multiple of 4", g->ldc_extra); return 1; }
    if (g->c_sample_rows ? (g->c_row_off < 0 || g->c_row_off + tokens > g->c_sample_rows) : g->c_row_off != 0) { pd_set_error("pd_op_linear_ex: c_row_off + tokens must fit c_sample_rows"); return 1; }
    if (g->a_sample_rows ? (g->a_row_off < 0 || g->a_row_off + tokens > g->a_sample_rows) : g->a_row_off != 0) { pd_set_error("pd_op_linear_ex: a_row_off + tokens must fit a_sample_rows"); return 1; }
    // what an instantiation would leave out without saying so (pd_mma.h: the extras are compile-time; gemm.hip: the GEGLU tiles add the bias only)
    const bool mm = g->gate || remap || act == ACT_TANH_GELU || act == ACT_ERF_GELU;
    if (packed && (g->residual || g->rowvec || g->gate || g->vt_begin || remap || scale != 1.f || g->a_silu || g->ln_gamma)) {
        pd_set_error("pd_op_linear_ex: a GEGLU / gated tanh-GELU layer takes a bias and nothing else");
        return 1;
    }
    if (act == ACT_RELU && mm) { pd_set_error("pd_op_linear_ex: the ReLU instantiations carry no gate / row remap"); return 1; }
    if (g->vt_tok_off && !mm) { pd_set_error("pd_op_linear_ex: vt_tok_off exists in the instantiations with the gate / row remaps only"); return 1; }
    if (g->ln_gamma && (!g->ln_beta || K > 2048 || g->a_silu)) { pd_set_error("pd_op_linear_ex: the LayerNorm fold needs gamma and beta, K <= 2048, no a_silu"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    TempMat guard(e);
    WMat m;
    const int wrows = packed ? 2 * N : N;
    e->make_mat(m, wrows, K, 1, K, true, packed);
    if (!m.w) { pd_set_error("allocation failed"); return 1; }
    PD_TRY(e->upload_rows(m, 0, g->w, wrows, false));
    if (g->bias) PD_TRY(e->upload_vec(m.bias, g->bias, wrows, packed, N));
    const int adt = g->a_silu ? DT_F32 : g->ln_gamma ? e->S : e->T, odt = ex_dt(e, g->out_dt), rdt = ex_dt(e, g->res_dt);
    const int Np = round_up(N, 4), ldc = Np + g->ldc_extra, ncol = g->vt_begin ? g->vt_begin : Np;   // ncol: the columns of C this call owns
    const int arows = g->a_sample_rows ? B * g->a_sample_rows : M, crows = g->c_sample_rows ? B * g->c_sample_rows : M;
    const int nvt = g->vt_begin ? N - g->vt_begin : 0, vt_ld = round_up(g->vt_tok_off + tokens, 8) + g->vt_extra;
    const float nan = std::nanf("");
    auto arow = [&](int i) { return g->a_sample_rows ? (i / tokens) * g->a_sample_rows + g->a_row_off + i % tokens : i; };
    auto crow = [&](int i) { return g->c_sample_rows ? (i / tokens) * g->c_sample_rows + g->c_row_off + i % tokens : i; };
    const size_t ob = dt_size(odt), nc = (size_t)crows * ldc, nv = (size_t)B * nvt * vt_ld;
    DevBuf in((size_t)arows * K * dt_size(adt)), out(nc * ob), vt(nv * ob), res((size_t)M * Np * dt_size(rdt)), rv((size_t)B * Np * 4), gt((size_t)B * Np * 4);
    if (!in.p || !out.p || !vt.p || !res.p || !rv.p || !gt.p) { pd_set_error("allocation failed"); return 1; }
    {
        std::vector<float> h((size_t)arows * K, g->a_sample_rows ? nan : 0.f);
        for (int i = 0; i < M; ++i) memcpy(&h[(size_t)arow(i) * K], g->x + (size_t)i * K, (size_t)K * 4);
        PD_TRY(put_flat(e, h, in.p, adt));
    }
    auto pad_cols = [&](const float* src, int rows, void* dst, int dt) -> int {   // [rows][N] -> [rows][Np]
        std::vector<float> h((size_t)rows * Np, 0.f);
        for (int i = 0; i < rows; ++i) memcpy(&h[(size_t)i * Np], src + (size_t)i * N, (size_t)N * 4);
        return put_flat(e, h, dst, dt);
    };
    if (g->residual) PD_TRY(pad_cols(g->residual, M, res.p, rdt));
    if (g->rowvec) PD_TRY(pad_cols(g->rowvec, B, rv.p, DT_F32));
    if (g->gate) PD_TRY(pad_cols(g->gate, B, gt.p, DT_F32));
    PD_TRY(put_flat(e, std::vector<float>(nc, nan), out.p, odt));
    if (nv) PD_TRY(put_flat(e, std::vector<float>(nv, nan), vt.p, odt));
    std::vector<unsigned char> c0(nc * ob), c1(nc * ob), v0(nv * ob), v1(nv * ob);   // the output buffers as the launch finds and leaves them
    HIP_OK(hipMemcpy(c0.data(), out.p, nc * ob, hipMemcpyDeviceToHost));
    if (nv) HIP_OK(hipMemcpy(v0.data(), vt.p, nv * ob, hipMemcpyDeviceToHost));
    Act a, o, r;
    a.p = in.p; a.B = B; a.H = tokens; a.W = 1; a.C = K; a.dt = adt;
    o.p = out.p; o.B = B; o.H = tokens; o.W = 1; o.C = Np; o.dt = odt;
    r = o; r.p = res.p; r.dt = rdt;
    GemmCall call;
    call.act = act == ACT_GEGLU ? ACT_NONE : (Activation)act;   // (a GEGLU weight matrix implies ACT_GEGLU)
    call.scale = scale;
    call.a_silu = g->a_silu != 0;
    if (g->residual) call.R = &r;
    if (g->rowvec) { call.rowvec = reinterpret_cast<const float*>(rv.p); call.rowvec_stride = Np; }
    if (g->gate) { call.gate = reinterpret_cast<const float*>(gt.p); call.gate_stride = Np; }
    if (nvt) { call.VT = vt.p; call.vt_begin = g->vt_begin; call.vt_ld = vt_ld; call.vt_tok_off = g->vt_tok_off; }
    if (g->ldc_extra) call.ldc = ldc;
    call.c_sample_rows = g->c_sample_rows; call.c_row_off = g->c_row_off;
    call.a_sample_rows = g->a_sample_rows; call.a_row_off = g->a_row_off;
    LnStats st;
    DevBuf stats((size_t)arows * 2 * 4), lg((size_t)K * 4 + 16), lb((size_t)K * 4 + 16);
    if (g->ln_gamma) {   // LayerNorm of x folded into the layer, statistics from row_stats_kernel (pd_op_ln_linear mode 1)
        if (!stats.p || !lg.p || !lb.p) { pd_set_error("allocation failed"); return 1; }
        HIP_OK(hipMemcpy(lg.p, g->ln_gamma, (size_t)K * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(lb.p, g->ln_beta, (size_t)K * 4, hipMemcpyHostToDevice));
        m.w_ln = e->dmalloc((size_t)m.N * m.Kpad * dt_size(e->T));
        m.colsum = reinterpret_cast<float*>(e->dmalloc((size_t)(m.N + 4) * sizeof(float)));
        m.bias_ln = reinterpret_cast<float*>(e->dmalloc((size_t)(m.N + 4) * sizeof(float)));
        if (!m.w_ln || !m.colsum || !m.bias_ln) { pd_set_error("allocation failed"); return 1; }
        if (launch_ln_fold(m.w, m.w_ln, e->T, m.N, m.K, m.Kpad, reinterpret_cast<float*>(lg.p), reinterpret_cast<float*>(lb.p), m.bias, m.colsum, m.bias_ln, e->stream) ||
            launch_row_stats(in.p, adt, reinterpret_cast<float*>(stats.p), arows, K, e->stream)) {
            pd_set_error("LayerNorm fold launch failed");
            return 1;
        }
        st.stats = reinterpret_cast<float*>(stats.p); st.parts = 1; st.C = K;
        call.ln_in = &st;
    }
    PD_TRY(e->gemm(m, a, o, call));
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(c1.data(), out.p, nc * ob, hipMemcpyDeviceToHost));
    if (nv) HIP_OK(hipMemcpy(v1.data(), vt.p, nv * ob, hipMemcpyDeviceToHost));
    std::vector<float> hc(nc), hv(nv);
    PD_TRY(get_flat(e, out.p, odt, hc));
    if (nv) PD_TRY(get_flat(e, vt.p, odt, hv));
    for (int i = 0; i < M; ++i) memcpy(g->y + (size_t)i * N, &hc[(size_t)crow(i) * ldc], (size_t)N * 4);
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < nvt; ++c)
            memcpy(g->vt + ((size_t)b * nvt + c) * tokens, &hv[((size_t)b * nvt + c) * vt_ld + g->vt_tok_off], (size_t)tokens * 4);
    // elements outside the call's own rows / columns / tokens whose bytes changed
    std::vector<char> own((size_t)crows, 0);
    for (int i = 0; i < M; ++i) own[crow(i)] = 1;
    int64_t changed = 0;
    for (int rr = 0; rr < crows; ++rr)
        for (int c = 0; c < ldc; ++c)
            if (!(own[rr] && c < ncol) && memcmp(&c0[((size_t)rr * ldc + c) * ob], &c1[((size_t)rr * ldc + c) * ob], ob)) ++changed;
    for (size_t i = 0; i < nv; ++i) {
        const int t = (int)(i % vt_ld);
        if (!(t >= g->vt_tok_off && t < g->vt_tok_off + tokens) && memcmp(&v0[i * ob], &v1[i * ob], ob)) ++changed;
    }
    g->touched = changed;
    return 0;
}

// y[M,N] = (e4m3(x / sx) @ e4m3(w / sw)^T) * sx * sw + b with per-row scales (max |row| / 448): the PREC_FP8 linear layer of
// the SD3 path (option sd3_fp8) on host fp32 arrays; act 4: tanh-GELU epilogue.  2-byte engine modes only.
int pd_op_linear_fp8(pd_engine* e, const float* x, const float* w, const float* bias, int M, int K, int N, int act, float* y) {
    if (!e || !x || !w || !y) { pd_set_error("null argument"); return 1; }
    if (e->f32) { pd_set_error("pd_op_linear_fp8: 2-byte engine modes only"); return 1; }
    if (K % 8 || (act != 0 && act != 4)) { pd_set_error("pd_op_linear_fp8: K must be a multiple of 8, act 0 or 4"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    TempMat guard(e);
    WMat m;
    e->make_mat(m, N, K, 1, K, true);
    if (!m.w) { pd_set_error("allocation failed"); return 1; }
    if (bias) PD_TRY(e->upload_vec(m.bias, bias, N, false, 0));
    m.Kpad8 = round_up(K, 128);
    DevBuf w32((size_t)N * K * 4), w8((size_t)m.N * m.Kpad8), ws((size_t)(m.N + 4) * 4), x32((size_t)M * K * 4), x8((size_t)M * m.Kpad8),
        xs((size_t)M * 4 + 16), out((size_t)M * round_up(N, 4) * 4);
    if (!w32.p || !w8.p || !ws.p || !x32.p || !x8.p || !xs.p || !out.p) { pd_set_error("allocation failed"); return 1; }
    HIP_OK(hipMemset(w8.p, 0, (size_t)m.N * m.Kpad8));
    HIP_OK(hipMemcpy(w32.p, w, (size_t)N * K * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(x32.p, x, (size_t)M * K * 4, hipMemcpyHostToDevice));
    HIP_OK(hipDeviceSynchronize());
    if (launch_quant_rows(w32.p, DT_F32, K, w8.p, m.Kpad8, reinterpret_cast<float*>(ws.p), N, K, e->stream) ||
        launch_quant_rows(x32.p, DT_F32, K, x8.p, m.Kpad8, reinterpret_cast<float*>(xs.p), M, K, e->stream)) {
        pd_set_error("quantisation launch failed");
        return 1;
    }
    m.w8 = w8.p; m.wscale = reinterpret_cast<float*>(ws.p);
    m.cin_pad = m.Kpad8;   // the activation rows are padded to the fp8 K step
    Act a, o;
    a.p = x8.p; a.B = M; a.H = 1; a.W = 1; a.C = m.Kpad8; a.dt = DT_FP8;
    o.p = out.p; o.B = M; o.H = 1; o.W = 1; o.C = round_up(N, 4); o.dt = DT_F32;
    PD_TRY(e->gemm(m, a, o, {.act = (Activation)act, .a_scale = reinterpret_cast<float*>(xs.p)}));
    HIP_OK(hipStreamSynchronize(e->stream));
    std::vector<float> host((size_t)M * o.C);
    HIP_OK(hipMemcpy(host.data(), out.p, host.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < M; ++i) memcpy(y + (size_t)i * N, host.data() + (size_t)i * o.C, (size_t)N * 4);
    return 0;
}

int pd_op_groupnorm(pd_engine* e, const float* x, const float* gamma, const float* beta, int B, int C, int H, int W, float eps,
                    int silu, float* y) {
    if (!e || !x || !gamma || !beta || !y) { pd_set_error("null argument"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    DevBuf in((size_t)B * H * W * C * dt_size(e->S)), out((size_t)B * H * W * C * dt_size(e->T)), g((size_t)C * 4 + 16), b((size_t)C * 4 + 16);
    if (!in.p || !out.p || !g.p || !b.p) { pd_set_error("allocation failed"); return 1; }
    HIP_OK(hipMemcpy(g.p, gamma, (size_t)C * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b.p, beta, (size_t)C * 4, hipMemcpyHostToDevice));
    PD_TRY(to_dev_nhwc(e, x, in.p, e->S, B, C, H, W, C));
    Act a, o;
    a.p = in.p; a.B = B; a.H = H; a.W = W; a.C = C; a.dt = e->S;
    o = a; o.p = out.p; o.dt = e->T;
    PD_TRY(e->groupnorm(a, o, reinterpret_cast<float*>(g.p), reinterpret_cast<float*>(b.p), eps, silu != 0));
    return from_dev_nhwc(e, out.p, e->T, y, B, C, H, W, C);
}

// GroupNorm (32 groups) of a tensor that exists only as a split-K GEMM's fp32 slabs: launch_gn_fused_slabs on host arrays
int pd_op_groupnorm_slabs(pd_engine* e, const float* slabs, int nslab, const float* bias, const float* row, const float* gamma,
                          const float* beta, int B, int C, int H, int W, float eps, int silu, float* y) {
    if (!e || !slabs || !gamma || !beta || !y) { pd_set_error("null argument"); return 1; }
    if (nslab < 1 || B < 1 || C < 32 || C % 32 || H < 1 || W < 1) { pd_set_error("pd_op_groupnorm_slabs: need nslab, B, H, W >= 1 and C a positive multiple of 32"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    const int HW = H * W;
    if (!gn_fused_bundle(e->S, HW, C, 32, e->opt.gn_reg)) { pd_set_error("pd_op_groupnorm_slabs: no single-kernel GroupNorm for C=%d HW=%d in this mode", C, HW); return 1; }
    const size_t n = (size_t)B * HW * C;
    DevBuf sl((size_t)nslab * n * 4), bi((size_t)C * 4 + 16), ro((size_t)B * C * 4 + 16), out(n * dt_size(e->T)), g((size_t)C * 4 + 16), b((size_t)C * 4 + 16);
    if (!sl.p || !bi.p || !ro.p || !out.p || !g.p || !b.p) { pd_set_error("allocation failed"); return 1; }
    HIP_OK(hipMemcpy(sl.p, slabs, (size_t)nslab * n * 4, hipMemcpyHostToDevice));
    if (bias) HIP_OK(hipMemcpy(bi.p, bias, (size_t)C * 4, hipMemcpyHostToDevice));
    if (row) HIP_OK(hipMemcpy(ro.p, row, (size_t)B * C * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(g.p, gamma, (size_t)C * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b.p, beta, (size_t)C * 4, hipMemcpyHostToDevice));
    if (launch_gn_fused_slabs(reinterpret_cast<const float*>(sl.p), nslab, bias ? reinterpret_cast<const float*>(bi.p) : nullptr,
                              row ? reinterpret_cast<const float*>(ro.p) : nullptr, C, e->S, out.p, e->T, reinterpret_cast<const float*>(g.p),
                              reinterpret_cast<const float*>(b.p), B, HW, C, 32, eps, silu ? 1 : 0, e->opt.gn_reg, e->stream, &e->gn_kernel)) {
        pd_set_error("pd_op_groupnorm_slabs: launch failed");
        return 1;
    }
    return from_dev_nhwc(e, out.p, e->T, y, B, C, H, W, C);
}

// gn_stats + gn_coef_kernel: the per-(sample, channel) {a, b} of y = x * a + b that the GroupNorm-fused convs and st_front_kernel apply
int pd_op_groupnorm_coef(pd_engine* e, const float* x, const float* gamma, const float* beta, int B, int C, int H, int W, float eps,
                         float* coef) {
    if (!e || !x || !gamma || !beta || !coef) { pd_set_error("null argument"); return 1; }
    if (B < 1 || C < 32 || C % 32 || H < 1 || W < 1) { pd_set_error("pd_op_groupnorm_coef: need B, H, W >= 1 and C a positive multiple of 32"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    DevBuf in((size_t)B * H * W * C * dt_size(e->S)), co((size_t)B * C * 2 * 4), g((size_t)C * 4 + 16), b((size_t)C * 4 + 16);
    if (!in.p || !co.p || !g.p || !b.p) { pd_set_error("allocation failed"); return 1; }
    HIP_OK(hipMemcpy(g.p, gamma, (size_t)C * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b.p, beta, (size_t)C * 4, hipMemcpyHostToDevice));
    PD_TRY(to_dev_nhwc(e, x, in.p, e->S, B, C, H, W, C));
    Act a;
    a.p = in.p; a.B = B; a.H = H; a.W = W; a.C = C; a.dt = e->S;
    int nchunk = 1;
    PD_TRY(e->gn_stats(a, nchunk));
    if (launch_gn_coef(e->gn_partial, reinterpret_cast<const float*>(g.p), reinterpret_cast<const float*>(b.p), reinterpret_cast<float*>(co.p), B,
                       H * W, C, 32, nchunk, eps, e->stream)) {
        pd_set_error("pd_op_groupnorm_coef: launch failed");
        return 1;
    }
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(coef, co.p, (size_t)B * C * 2 * 4, hipMemcpyDeviceToHost));
    return 0;
}

// y = Linear(LayerNorm(h)) the three ways a transformer block computes it (pd_engine::transformer): h in the residual-stream type,
// y in the compute type, both through pd_engine::gemm
int pd_op_ln_linear(pd_engine* e, int mode, const float* h, const float* x, const float* w1, const float* b1, const float* residual,
                    const float* gamma, const float* beta, const float* w, const float* bias, int M, int K, int N, float* h_out, float* y,
                    int* stats_parts, float* row_stats) {
    if (!e || !gamma || !beta || !w || !y) { pd_set_error("null argument"); return 1; }
    if (mode < 0 || mode > 2 || (mode < 2 ? !h : (!x || !w1))) { pd_set_error("pd_op_ln_linear: mode 0 / 1 take h, mode 2 takes x and w1"); return 1; }
    if (M < 1 || N < 1 || K < 8 || K % 8 || K > 2048) { pd_set_error("pd_op_ln_linear: need M, N >= 1 and K a multiple of 8, at most 2048"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    TempMat guard(e);
    const int Np = round_up(N, 4);
    const size_t sb = dt_size(e->S), tb = dt_size(e->T);
    WMat m, m1;
    e->make_mat(m, N, K, 1, K, true);
    if (!m.w) { pd_set_error("allocation failed"); return 1; }
    PD_TRY(e->upload_rows(m, 0, w, N, false));
    if (bias) PD_TRY(e->upload_vec(m.bias, bias, N, false, 0));
    DevBuf tmp((size_t)M * K * 4), hs((size_t)M * K * sb), a1((size_t)M * K * tb), rs((size_t)M * K * sb), ln((size_t)M * K * tb), out((size_t)M * Np * tb),
        g((size_t)K * 4 + 16), b((size_t)K * 4 + 16), f32out((size_t)M * (Np > K ? Np : K) * 4);
    const int cap_parts = ((K + 159) / 160) * 2;   // pd_engine::transformer's sizing of the statistics rows
    DevBuf stats((size_t)M * cap_parts * 2 * 4);
    if (!tmp.p || !hs.p || !a1.p || !rs.p || !ln.p || !out.p || !g.p || !b.p || !f32out.p || !stats.p) { pd_set_error("allocation failed"); return 1; }
    HIP_OK(hipMemcpy(g.p, gamma, (size_t)K * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b.p, beta, (size_t)K * 4, hipMemcpyHostToDevice));
    auto put = [&](const float* src, void* dst, int dt) -> int {   // host fp32 [M][K] -> device rows in dt
        HIP_OK(hipMemcpy(tmp.p, src, (size_t)M * K * 4, hipMemcpyHostToDevice));
        if (launch_cast_rows(reinterpret_cast<const float*>(tmp.p), dst, dt, M, K, K, e->stream)) { pd_set_error("cast launch failed"); return 1; }
        HIP_OK(hipStreamSynchronize(e->stream));
        return 0;
    };
    auto get = [&](const void* src, int dt, int ld, int cols, float* dst) -> int {   // device rows in dt -> host fp32 [M][cols]
        if (launch_nhwc_to_nchw(src, dt, reinterpret_cast<float*>(f32out.p), 1, 1, 1, M * ld, 1, 1.f, e->stream)) { pd_set_error("cast launch failed"); return 1; }
        HIP_OK(hipStreamSynchronize(e->stream));
        std::vector<float> host((size_t)M * ld);
        HIP_OK(hipMemcpy(host.data(), f32out.p, host.size() * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < M; ++i) memcpy(dst + (size_t)i * cols, host.data() + (size_t)i * ld, (size_t)cols * 4);
        return 0;
    };
    Act hA, o;
    hA.p = hs.p; hA.B = M; hA.H = 1; hA.W = 1; hA.C = K; hA.dt = e->S;
    o.p = out.p; o.B = M; o.H = 1; o.W = 1; o.C = Np; o.dt = e->T;
    LnStats st;
    st.stats = reinterpret_cast<float*>(stats.p);
    st.cap_parts = cap_parts;
    if (mode == 2) {   // the producer writes h and leaves the row statistics (proj_in / attn1.to_out with its residual)
        e->make_mat(m1, K, K, 1, K, true);
        if (!m1.w) { pd_set_error("allocation failed"); return 1; }
        PD_TRY(e->upload_rows(m1, 0, w1, K, false));
        if (b1) PD_TRY(e->upload_vec(m1.bias, b1, K, false, 0));
        PD_TRY(put(x, a1.p, e->T));
        Act a, r;
        a = hA; a.p = a1.p; a.dt = e->T;
        r = hA; r.p = rs.p;
        if (residual) PD_TRY(put(residual, rs.p, e->S));
        PD_TRY(e->gemm(m1, a, hA, {.R = residual ? &r : nullptr, .ln_out = &st}));
    } else {
        PD_TRY(put(h, hs.p, e->S));
    }
    if (mode == 0) {
        Act l = hA;
        l.p = ln.p; l.dt = e->T;
        PD_TRY(e->layernorm(hA, l, reinterpret_cast<float*>(g.p), reinterpret_cast<float*>(b.p)));
        PD_TRY(e->gemm(m, l, o));
    } else {
        m.w_ln = e->dmalloc((size_t)m.N * m.Kpad * tb);
        m.colsum = reinterpret_cast<float*>(e->dmalloc((size_t)(m.N + 4) * sizeof(float)));
        m.bias_ln = reinterpret_cast<float*>(e->dmalloc((size_t)(m.N + 4) * sizeof(float)));
        if (!m.w_ln || !m.colsum || !m.bias_ln) { pd_set_error("allocation failed"); return 1; }
        if (launch_ln_fold(m.w, m.w_ln, e->T, m.N, m.K, m.Kpad, reinterpret_cast<float*>(g.p), reinterpret_cast<float*>(b.p), m.bias, m.colsum,
                           m.bias_ln, e->stream)) {
            pd_set_error("LayerNorm fold launch failed");
            return 1;
        }
        if (mode == 1) {
            st.parts = 1; st.C = K;
            if (launch_row_stats(hs.p, e->S, st.stats, M, K, e->stream)) { pd_set_error("row statistics launch failed"); return 1; }
        }
        PD_TRY(e->gemm(m, hA, o, {.ln_in = &st}));
    }
    HIP_OK(hipStreamSynchronize(e->stream));
    if (stats_parts) *stats_parts = mode ? st.parts : 0;
    if (row_stats && mode) {   // what the consumer's ln_row_stats folds: the partials of every row, summed here in their order
        if (st.parts < 1 || st.parts > cap_parts) { pd_set_error("pd_op_ln_linear: %d statistics partials per row", st.parts); return 1; }
        std::vector<float> hp((size_t)M * st.parts * 2);
        HIP_OK(hipMemcpy(hp.data(), stats.p, hp.size() * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < M; ++i) {
            float sum = 0.f, sq = 0.f;
            for (int k = 0; k < st.parts; ++k) { sum += hp[((size_t)i * st.parts + k) * 2]; sq += hp[((size_t)i * st.parts + k) * 2 + 1]; }
            row_stats[2 * i] = sum; row_stats[2 * i + 1] = sq;
        }
    }
    if (h_out) PD_TRY(get(hs.p, e->S, K, K, h_out));
    return get(out.p, e->T, Np, N, y);
}

int pd_op_layernorm(pd_engine* e, const float* x, const float* gamma, const float* beta, int rows, int C, float* y) {
    if (!e || !x || !gamma || !beta || !y) { pd_set_error("null argument"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    DevBuf tmp((size_t)rows * C * 4), in((size_t)rows * C * dt_size(e->S)), out((size_t)rows * C * 4), g((size_t)C * 4 + 16), b((size_t)C * 4 + 16);
    if (!tmp.p || !in.p || !out.p || !g.p || !b.p) { pd_set_error("allocation failed"); return 1; }
    HIP_OK(hipMemcpy(g.p, gamma, (size_t)C * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b.p, beta, (size_t)C * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(tmp.p, x, (size_t)rows * C * 4, hipMemcpyHostToDevice));
    if (launch_cast_rows(reinterpret_cast<const float*>(tmp.p), in.p, e->S, rows, C, C, e->stream)) return 1;
    Act a, o;
    a.p = in.p; a.B = rows; a.H = 1; a.W = 1; a.C = C; a.dt = e->S;
    o = a; o.p = out.p; o.dt = DT_F32;
    PD_TRY(e->layernorm(a, o, reinterpret_cast<float*>(g.p), reinterpret_cast<float*>(b.p)));
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(y, out.p, (size_t)rows * C * 4, hipMemcpyDeviceToHost));
    return 0;
}

// softmax(q k^T dh^-0.5) v per head; q [B,Nq,C], k/v [B,Nk,C] fp32, C = heads*dh (heads from the engine config)
int pd_op_attention(pd_engine* e, const float* q, const float* k, const float* v, int B, int Nq, int Nk, int C, float* o) {
    return pd_op_attention_ex(e, q, k, v, B, Nq, Nk, C, 0, 0, 0.f, nullptr, 0, 0, 0.f, o, nullptr);
}

// pd_engine::attention with everything its callers pass (see pdengine_ops.h): heads, causal mask, scale, Toeplitz bias rows, the strided
// q | k arrangement of a fused projection, extra V^T row padding, and a fill value for every byte the kernel must not let through
int pd_op_attention_ex(pd_engine* e, const float* q, const float* k, const float* v, int B, int Nq, int Nk, int C, int heads, int causal,
                       float scale, const float* relbias, int layout, int vt_extra, float pad_fill, float* o, int64_t* touched) {
    if (!e || !q || !k || !v || !o) { pd_set_error("null argument"); return 1; }
    if (heads <= 0) heads = e->cfg.num_heads;
    if (B < 1 || Nq < 1 || Nk < 1 || C < 1 || heads < 1 || C % heads) { pd_set_error("pd_op_attention_ex: need B, Nq, Nk >= 1 and C a multiple of heads"); return 1; }
    const int dh = C / heads;
    if (layout != 0 && layout != 1) { pd_set_error("pd_op_attention_ex: layout %d (0 contiguous, 1 q | k rows of one buffer)", layout); return 1; }
    if (layout == 1 && Nq > Nk) { pd_set_error("pd_op_attention_ex: layout 1 takes the queries from the first Nq <= Nk rows (Nq %d, Nk %d)", Nq, Nk); return 1; }
    if (vt_extra < 0 || vt_extra % 8) { pd_set_error("pd_op_attention_ex: vt_extra %d must be a non-negative multiple of 8", vt_extra); return 1; }
    if (!(scale >= 0.f)) { pd_set_error("pd_op_attention_ex: scale must be positive (0: dh^-0.5)"); return 1; }
    if (causal && Nq != Nk) { pd_set_error("pd_op_attention_ex: the causal mask needs Nq == Nk (got %d, %d)", Nq, Nk); return 1; }
    if (relbias && (dh != 64 || Nq != Nk || causal)) {
        pd_set_error("pd_op_attention_ex: the bias kernel takes dh 64, Nq == Nk, no causal mask (got dh %d, Nq %d, Nk %d, causal %d)", dh, Nq, Nk, causal);
        return 1;
    }
    HIP_OK(hipSetDevice(e->device));
    const int lpad = round_up(Nk, 8) + vt_extra;
    const size_t eb = dt_size(e->T);
    const int ld = layout ? 2 * C : C;          // row stride of q and of k
    const int qrows = layout ? Nk : Nq;         // rows per sample of the query and of the output buffer
    std::vector<float> vt((size_t)B * C * lpad, pad_fill);
    for (int b = 0; b < B; ++b)
        for (int n = 0; n < Nk; ++n)
            for (int c = 0; c < C; ++c) vt[((size_t)b * C + c) * lpad + n] = v[((size_t)b * Nk + n) * C + c];
    // layout 0: hq = q, hk = k as they came; layout 1: hq [B][Nk][2C] holds q | k, the q half of rows >= Nq filled
    std::vector<float> hqk;
    if (layout) {
        hqk.assign((size_t)B * Nk * 2 * C, pad_fill);
        for (int b = 0; b < B; ++b)
            for (int n = 0; n < Nk; ++n) {
                float* row = &hqk[((size_t)b * Nk + n) * 2 * C];
                if (n < Nq) memcpy(row, q + ((size_t)b * Nq + n) * C, (size_t)C * 4);
                memcpy(row + C, k + ((size_t)b * Nk + n) * C, (size_t)C * 4);
            }
    }
    const size_t nq = (size_t)B * qrows * ld, nk = layout ? 0 : (size_t)B * Nk * C, no = (size_t)B * qrows * C;
    std::vector<float> fill(no, pad_fill);
    DevBuf tq(nq * 4), tk(nk * 4), tv(vt.size() * 4), fo(no * 4);
    DevBuf dq(nq * eb), dk(nk * eb), dv(vt.size() * eb), dout(no * eb);
    if (!tq.p || !tk.p || !tv.p || !dq.p || !dk.p || !dv.p || !dout.p || !fo.p) { pd_set_error("allocation failed"); return 1; }
    HIP_OK(hipMemcpy(tq.p, layout ? hqk.data() : q, nq * 4, hipMemcpyHostToDevice));
    if (!layout) HIP_OK(hipMemcpy(tk.p, k, nk * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(tv.p, vt.data(), vt.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(fo.p, fill.data(), no * 4, hipMemcpyHostToDevice));
    if (launch_cast_rows(reinterpret_cast<const float*>(tq.p), dq.p, e->T, (long long)B * qrows, ld, ld, e->stream)) return 1;
    if (!layout && launch_cast_rows(reinterpret_cast<const float*>(tk.p), dk.p, e->T, (long long)B * Nk, C, C, e->stream)) return 1;
    if (launch_cast_rows(reinterpret_cast<const float*>(tv.p), dv.p, e->T, (long long)B * C, lpad, lpad, e->stream)) return 1;
    if (layout && launch_cast_rows(reinterpret_cast<const float*>(fo.p), dout.p, e->T, (long long)B * qrows, C, C, e->stream)) return 1;
    std::vector<unsigned char> before, after;
    if (layout) {   // the output buffer as the launch finds it
        before.resize(no * eb); after.resize(no * eb);
        HIP_OK(hipStreamSynchronize(e->stream));
        HIP_OK(hipMemcpy(before.data(), dout.p, no * eb, hipMemcpyDeviceToHost));
    }
    // Toeplitz bias rows: natural-log units in, exp2 units to the kernel through T5's own conversion (launch_t5_relbias with the identity
    // bucket map over a [2 Nk - 1][heads] fp32 table)
    const int nrel = 2 * Nk - 1;
    DevBuf btab(relbias ? (size_t)nrel * heads * 4 : 0), bidx(relbias ? (size_t)nrel * 4 : 0), brel(relbias ? (size_t)nrel * heads * 4 : 0);
    if (relbias) {
        if (!btab.p || !bidx.p || !brel.p) { pd_set_error("allocation failed"); return 1; }
        std::vector<float> tab((size_t)nrel * heads);
        std::vector<int> idx(nrel);
        for (int i = 0; i < nrel; ++i) {
            idx[i] = i;
            for (int h = 0; h < heads; ++h) tab[(size_t)i * heads + h] = relbias[(size_t)h * nrel + i];
        }
        HIP_OK(hipMemcpy(btab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(bidx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
        if (launch_t5_relbias(reinterpret_cast<const int*>(bidx.p), btab.p, heads, DT_F32, reinterpret_cast<float*>(brel.p), heads, nrel, e->stream)) {
            pd_set_error("pd_op_attention_ex: bias conversion launch failed");
            return 1;
        }
    }
    const void* kp = layout ? reinterpret_cast<const char*>(dq.p) + (size_t)C * eb : dk.p;
    const long long in_bs = layout ? (long long)Nk * 2 * C : 0, out_bs = layout ? (long long)Nk * C : 0;
    PD_TRY(e->attention(dq.p, ld, kp, ld, dv.p, lpad, dout.p, C, B, Nq, Nk, C, heads, causal != 0, in_bs, in_bs, out_bs,
                        relbias ? reinterpret_cast<const float*>(brel.p) : nullptr, scale));
    if (launch_nhwc_to_nchw(dout.p, e->T, reinterpret_cast<float*>(fo.p), 1, 1, 1, (int)no, 1, 1.f, e->stream)) return 1;
    HIP_OK(hipStreamSynchronize(e->stream));
    if (!layout) {
        HIP_OK(hipMemcpy(o, fo.p, no * 4, hipMemcpyDeviceToHost));
        if (touched) *touched = 0;
        return 0;
    }
    for (int b = 0; b < B; ++b)
        HIP_OK(hipMemcpy(o + (size_t)b * Nq * C, reinterpret_cast<const float*>(fo.p) + (size_t)b * Nk * C, (size_t)Nq * C * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(after.data(), dout.p, no * eb, hipMemcpyDeviceToHost));
    int64_t changed = 0;   // elements of the rows >= Nq whose bytes differ from what the launch found
    for (int b = 0; b < B; ++b)
        for (size_t i = ((size_t)b * Nk + Nq) * C; i < ((size_t)b * Nk + Nk) * C; ++i)
            if (memcmp(&before[i * eb], &after[i * eb], eb)) ++changed;
    if (touched) *touched = changed;
    return 0;
}

// softmax(q k^T C^-0.5) v with ONE head over all C channels (the first stage's AttnBlock); q, k, v, o [B, N, C] fp32.  Runs what
// pd_engine::vae_attention runs between its two projections: vae_attention.hip where option "vae_flash" is 1 (2-byte modes, C 128 / 512:
// anything else is an error, not a fall-back), the three-launch materialised path where it is 0 or -1 (N a multiple of 8)
int pd_op_vae_attention(pd_engine* e, const float* q, const float* k, const float* v, int B, int N, int C, float* o) {
    if (!e || !q || !k || !v || !o) { pd_set_error("null argument"); return 1; }
    if (B < 1 || N < 1 || C < 8 || C % 8) { pd_set_error("pd_op_vae_attention: need B, N >= 1 and C a multiple of 8"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    const bool flash = e->opt.vae_flash > 0;
    if (flash && (e->f32 || !vae_attention_eligible(e->T, C))) {
        pd_set_error("pd_op_vae_attention: the flash kernel takes the 2-byte modes at C = 128 or 512 (got C = %d)", C);
        return 1;
    }
    if (!flash && N % 8) { pd_set_error("pd_op_vae_attention: the materialised path needs N a multiple of 8 (got %d)", N); return 1; }
    const int npad = flash ? round_up(N, 8) : round_up(N, 64);
    const size_t eb = dt_size(e->T);
    // q | k interleaved per token like the fused projection's output [B][N][2C]; V transposed and zero-padded [B][C][npad]
    std::vector<float> qk((size_t)B * N * 2 * C), vt((size_t)B * C * npad, 0.f);
    for (size_t r = 0; r < (size_t)B * N; ++r) {
        memcpy(&qk[r * 2 * C], q + r * C, (size_t)C * 4);
        memcpy(&qk[r * 2 * C + C], k + r * C, (size_t)C * 4);
    }
    for (int b = 0; b < B; ++b)
        for (int n = 0; n < N; ++n)
            for (int c = 0; c < C; ++c) vt[((size_t)b * C + c) * npad + n] = v[((size_t)b * N + n) * C + c];
    DevBuf tqk(qk.size() * 4), tv(vt.size() * 4), dqk(qk.size() * eb), dv(vt.size() * eb), dout((size_t)B * N * C * eb), fo((size_t)B * N * C * 4);
    DevBuf sc(flash ? 0 : (size_t)N * N * 4), pr(flash ? 0 : (size_t)N * npad * eb);   // (DevBuf zero-fills: the pad columns of pr)
    if (!tqk.p || !tv.p || !dqk.p || !dv.p || !dout.p || !fo.p || !sc.p || !pr.p) { pd_set_error("allocation failed"); return 1; }
    HIP_OK(hipMemcpy(tqk.p, qk.data(), qk.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(tv.p, vt.data(), vt.size() * 4, hipMemcpyHostToDevice));
    if (launch_cast_rows(reinterpret_cast<const float*>(tqk.p), dqk.p, e->T, (long long)B * N, 2 * C, 2 * C, e->stream)) return 1;
    if (launch_cast_rows(reinterpret_cast<const float*>(tv.p), dv.p, e->T, (long long)B * C, npad, npad, e->stream)) return 1;
    PD_TRY(e->vae_attn_product(dqk.p, 2 * C, dv.p, npad, dout.p, B, N, C, flash, reinterpret_cast<float*>(sc.p), pr.p));
    if (launch_nhwc_to_nchw(dout.p, e->T, reinterpret_cast<float*>(fo.p), 1, 1, 1, B * N * C, 1, 1.f, e->stream)) return 1;
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(o, fo.p, (size_t)B * N * C * 4, hipMemcpyDeviceToHost));
    return 0;
}

// IP-Adapter's image term alone (launch_ip_attention_add): out = round_T(att + s * softmax(q2 k_ip^T scale) v_ip) per head, every operand
// rounded to the compute type first; q2, att, out [B, N, C]; k_ip, v_ip [Bk, T, C], Bk = B or 1 (one set for every sample); scale 0: dh^-0.5
int pd_op_ip_attention_add(pd_engine* e, const float* q2, const float* att, const float* k_ip, const float* v_ip, int B, int N, int C, int heads, int T,
                           int Bk, float scale, float s, float* out) {
    if (!e || !q2 || !att || !k_ip || !v_ip || !out) { pd_set_error("null argument"); return 1; }
    if (heads <= 0) heads = e->cfg.num_heads;
    if (B < 1 || N < 1 || C < 8 || C % 8 || C % heads || T < 1 || T > 64 || (Bk != 1 && Bk != B)) {
        pd_set_error("pd_op_ip_attention_add: need B, N >= 1, C a multiple of 8 and of heads, 1 <= T <= 64, Bk = 1 or B (got B %d N %d C %d heads %d T %d Bk %d)", B,
                     N, C, heads, T, Bk);
        return 1;
    }
    if ((long long)B * N * C > INT32_MAX) { pd_set_error("pd_op_ip_attention_add: more than 2^31 elements"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    const size_t eb = dt_size(e->T), no = (size_t)B * N * C, nk = (size_t)Bk * T * C;
    DevBuf fq(no * 4), fa(no * 4), fk(nk * 4), fv(nk * 4), dq(no * eb), da(no * eb), dk(nk * eb), dv(nk * eb);
    if (!fq.p || !fa.p || !fk.p || !fv.p || !dq.p || !da.p || !dk.p || !dv.p) { pd_set_error("allocation failed"); return 1; }
    HIP_OK(hipMemcpy(fq.p, q2, no * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(fa.p, att, no * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(fk.p, k_ip, nk * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(fv.p, v_ip, nk * 4, hipMemcpyHostToDevice));
    if (launch_cast_rows(reinterpret_cast<const float*>(fq.p), dq.p, e->T, (long long)B * N, C, C, e->stream)) return 1;
    if (launch_cast_rows(reinterpret_cast<const float*>(fa.p), da.p, e->T, (long long)B * N, C, C, e->stream)) return 1;
    if (launch_cast_rows(reinterpret_cast<const float*>(fk.p), dk.p, e->T, (long long)Bk * T, C, C, e->stream)) return 1;
    if (launch_cast_rows(reinterpret_cast<const float*>(fv.p), dv.p, e->T, (long long)Bk * T, C, C, e->stream)) return 1;
    if (scale == 0.f) scale = (float)(1.0 / std::sqrt((double)(C / heads)));
    ++e->launches;
    const int r = launch_ip_attention_add(dq.p, da.p, dk.p, dv.p, Bk == 1 ? 0 : (long long)T * C, B, N, C, heads, T, scale, s, e->T, e->stream);
    if (r) { pd_set_error(r == 2 ? "pd_op_ip_attention_add: unsupported head dim %d" : "pd_op_ip_attention_add: launch failed (dh %d)", C / heads); return 1; }
    if (launch_nhwc_to_nchw(da.p, e->T, reinterpret_cast<float*>(fa.p), 1, 1, 1, (int)no, 1, 1.f, e->stream)) return 1;
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(out, fa.p, no * 4, hipMemcpyDeviceToHost));
    return 0;
}

// launch_pag_identity on host data: vt [Bs, C, N] -> out [count, N, C] = samples [src, src + count) transposed, through the engine's
// storage type and the V^T layout of the QKV GEMM (row stride round_up(N, 8)); the pad columns hold 1.0, which a correct kernel never copies
int pd_op_pag_identity(pd_engine* e, const float* vt, int Bs, int C, int N, int src, int count, float* out) {
    if (!e || !vt || !out) { pd_set_error("null argument"); return 1; }
    if (Bs < 1 || C < 1 || N < 1 || src < 0 || count < 1 || src + count > Bs) {
        pd_set_error("pd_op_pag_identity: need Bs, C, N >= 1 and 0 <= src, src + count <= Bs (got Bs %d C %d N %d src %d count %d)", Bs, C, N, src, count);
        return 1;
    }
    HIP_OK(hipSetDevice(e->device));
    const int npad = round_up(N, 8);
    const size_t eb = dt_size(e->T), nin = (size_t)Bs * C * npad, nout = (size_t)count * N * C;
    std::vector<float> host(nin, 1.0f);
    for (size_t r = 0; r < (size_t)Bs * C; ++r) std::memcpy(&host[r * npad], vt + r * N, (size_t)N * sizeof(float));
    DevBuf fin(nin * 4), din(nin * eb), dout(nout * eb), fout(nout * 4);
    if (!fin.p || !din.p || !dout.p || !fout.p) { pd_set_error("allocation failed"); return 1; }
    HIP_OK(hipMemcpy(fin.p, host.data(), nin * 4, hipMemcpyHostToDevice));
    if (launch_cast_rows(reinterpret_cast<const float*>(fin.p), din.p, e->T, (long long)Bs * C, npad, npad, e->stream)) return 1;
    ++e->launches;
    ++e->pag_launches;
    if (launch_pag_identity(din.p, dout.p, (int)eb, src, count, N, C, npad, e->stream)) { pd_set_error("pd_op_pag_identity: launch failed (N %d, C %d)", N, C); return 1; }
    if (launch_nhwc_to_nchw(dout.p, e->T, reinterpret_cast<float*>(fout.p), 1, 1, 1, (int)nout, 1, 1.f, e->stream)) return 1;
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(out, fout.p, nout * 4, hipMemcpyDeviceToHost));
    return 0;
}

int pd_bench_pag_identity(pd_engine* e, int32_t B, int32_t N, int32_t C, int32_t iters, float* ms_kernel, float* ms_copy) {
    if (!e || !ms_kernel || !ms_copy || iters < 1 || B < 1 || N < 1 || C < 1) { pd_set_error("pd_bench_pag_identity: bad argument"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    const int npad = round_up(N, 8);
    const size_t eb = dt_size(e->T), nin = (size_t)B * C * npad, nout = (size_t)B * N * C;
    DevBuf vt(nin * eb), att(nout * eb), src(nout * eb), dst(nout * eb);
    if (!vt.p || !att.p || !src.p || !dst.p) { pd_set_error("pd_bench_pag_identity: allocation failed"); return 1; }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    int rc = 0;
    float t = 0.f;
    for (int i = 0; i < 3 && !rc; ++i) rc = launch_pag_identity(vt.p, att.p, (int)eb, 0, B, N, C, npad, e->stream);
    hipEventRecord(e0, e->stream);
    for (int i = 0; i < iters && !rc; ++i) rc = launch_pag_identity(vt.p, att.p, (int)eb, 0, B, N, C, npad, e->stream);
    hipEventRecord(e1, e->stream);
    hipEventSynchronize(e1);
    hipEventElapsedTime(&t, e0, e1);
    *ms_kernel = t / (float)iters;
    for (int i = 0; i < 3; ++i) hipMemcpyAsync(dst.p, src.p, nout * eb, hipMemcpyDeviceToDevice, e->stream);
    hipEventRecord(e0, e->stream);
    for (int i = 0; i < iters; ++i) hipMemcpyAsync(dst.p, src.p, nout * eb, hipMemcpyDeviceToDevice, e->stream);
    hipEventRecord(e1, e->stream);
    hipEventSynchronize(e1);
    hipEventElapsedTime(&t, e0, e1);
    *ms_copy = t / (float)iters;
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    if (rc) { pd_set_error("pd_bench_pag_identity: launch failed (N %d, C %d)", N, C); return 1; }
    return 0;
}

// The guidance of cfg_update_kernel alone (do_update 0) as an evaluation with perturbed-attention guidance on runs it (UpdateState::pag;
// pag_scale 0 is then a step at the adaptive scale's clamp): eps [Bt, HW, C] in eps_dtype -> out [B, HW, C] fp32
int pd_op_cfg_combine(pd_engine* e, const float* eps, int B, int HW, int C, int eps_dtype, int use_cfg, float cfg_scale, float pag_scale,
                      float* out) {
    if (!e || !eps || !out) { pd_set_error("null argument"); return 1; }
    if (B < 1 || HW < 1 || C < 1 || (eps_dtype != PD_DT_F32 && eps_dtype != PD_DT_F16 && eps_dtype != PD_DT_BF16)) {
        pd_set_error("pd_op_cfg_combine: need B, HW, C >= 1 and eps_dtype one of PD_DT_F32 / F16 / BF16 (got %d, %d, %d, %d)", B, HW, C, eps_dtype);
        return 1;
    }
    HIP_OK(hipSetDevice(e->device));
    const int Bf = use_cfg ? 2 * B : B, Bt = Bf + (pag_scale != 0.f ? B : 0);
    const int dt = eps_dtype == PD_DT_F32 ? DT_F32 : eps_dtype == PD_DT_F16 ? DT_F16 : DT_BF16;
    const size_t nin = (size_t)Bt * HW * C, nout = (size_t)B * HW * C;
    DevBuf fin(nin * 4), din(nin * dt_size(dt)), dout(nout * 4);
    if (!fin.p || !din.p || !dout.p) { pd_set_error("allocation failed"); return 1; }
    HIP_OK(hipMemcpy(fin.p, eps, nin * 4, hipMemcpyHostToDevice));
    if (launch_cast_rows(reinterpret_cast<const float*>(fin.p), din.p, dt, (long long)Bt * HW, C, C, e->stream)) return 1;
    UpdateState u{din.p, dt, C, nullptr, nullptr, reinterpret_cast<float*>(dout.p), nullptr, B, HW, C, C, use_cfg ? 1 : 0};
    u.pag = 1;      // the guidance of an evaluation with the state on, whatever the step's scale
    u.pag_scale = pag_scale;
    u.pag_off = Bf;
    DdimCoef k{};
    k.cfg_scale = cfg_scale;
    ++e->launches;
    if (launch_cfg_ddim(u, k, nullptr, 1.f, 0, nullptr, e->stream)) { pd_set_error("pd_op_cfg_combine: launch failed"); return 1; }
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(out, dout.p, nout * 4, hipMemcpyDeviceToHost));
    return 0;
}

// One whole SpatialTransformer block of the engine's own networks (GroupNorm eps 1e-6, proj_in, BasicTransformerBlock, proj_out, + x;
// attention.py:321-340 and :271-275) with the weights loaded under `prefix` (e.g. "model.diffusion_model.input_blocks.1.1.") on
// x [B, C, H, W] and context [B, context_len, context_dim], through exactly the code path a sampling step takes -- including the fused
// tail kernel (st_tail.hip) where it is eligible.
int pd_op_spatial_transformer(pd_engine* e, const char* prefix, const float* x, const float* ctx, int B, int H, int W, float* y) {
    if (!e) { pd_set_error("null argument"); return 1; }
    return pd_op_spatial_transformer_ctx(e, prefix, x, ctx, B, H, W, e->cfg.context_len, y);
}

// ... on a context of any length: [B, L, context_dim], 1 <= L <= PD_MAX_CONTEXT_LEN
static int spatial_transformer_hook(pd_engine* e, const char* prefix, const float* x, const float* ctx, const float* tokens, int B, int H, int W, int L,
                                    int T, float* y, int n_perturbed = 0);
// ... with the last n_perturbed samples perturbed (perturbed-attention guidance, PagTerm): identity self-attention from their own V
int pd_op_spatial_transformer_pag(pd_engine* e, const char* prefix, const float* x, const float* ctx, int B, int H, int W, int L, int n_perturbed,
                                  float* y) {
    if (n_perturbed < 1 || n_perturbed >= B) { pd_set_error("pd_op_spatial_transformer_pag: n_perturbed %d outside 1 .. B - 1 = %d", n_perturbed, B - 1); return 1; }
    return spatial_transformer_hook(e, prefix, x, ctx, nullptr, B, H, W, L, 0, y, n_perturbed);
}
int pd_op_spatial_transformer_ctx(pd_engine* e, const char* prefix, const float* x, const float* ctx, int B, int H, int W, int L, float* y) {
    return spatial_transformer_hook(e, prefix, x, ctx, nullptr, B, H, W, L, 0, y);
}

// ... with IP-Adapter's image term: tokens [B, T, context_dim] go through the block's loaded to_k_ip / to_v_ip (the engine's own GEMMs),
// then the block runs with the term at the block's current scale, as in a sampling step.  Scale 0: exactly the call above.
int pd_op_spatial_transformer_ip(pd_engine* e, const char* prefix, const float* x, const float* ctx, const float* tokens, int B, int H, int W, int L,
                                 int T, float* y) {
    if (!tokens) { pd_set_error("null argument"); return 1; }
    return spatial_transformer_hook(e, prefix, x, ctx, tokens, B, H, W, L, T, y);
}

static int spatial_transformer_hook(pd_engine* e, const char* prefix, const float* x, const float* ctx, const float* tokens, int B, int H, int W, int L,
                                    int T, float* y, int n_perturbed) {
    if (!e || !prefix || !x || !ctx || !y) { pd_set_error("null argument"); return 1; }
    if (L < 1 || L > PD_MAX_CONTEXT_LEN) { pd_set_error("context length %d out of range 1 .. %d", L, PD_MAX_CONTEXT_LEN); return 1; }
    HIP_OK(hipSetDevice(e->device));
    const std::string pre(prefix);
    auto it = e->index.find(pre + "norm.weight");
    if (it == e->index.end()) { pd_set_error("no SpatialTransformer under '%s'", prefix); return 1; }
    const float* gn_g = e->params[it->second].vdst;
    STW* st = nullptr;
    for (NetW* net : {&e->unet, &e->cnet})
        for (STW* s : net->st_list)
            if (s->gn_g == gn_g) st = s;
    if (!st) { pd_set_error("no SpatialTransformer under '%s'", prefix); return 1; }
    for (const Param& p : e->params)
        if (!p.loaded && p.name.compare(0, pre.size(), pre) == 0) { pd_set_error("weights not loaded: '%s'", p.name.c_str()); return 1; }
    const int ipj = st->ip_slot;
    if (tokens) {
        if (ipj < 0 || !e->ip.built || e->ip.broken) { pd_set_error("no IP-Adapter weights for the block under '%s' (pd_ip_adapter_configure; UNet blocks only)", prefix); return 1; }
        if (T < 1 || T > 64) { pd_set_error("pd_op_spatial_transformer_ip: T %d outside 1 .. 64", T); return 1; }
        for (const char* w : {"to_k_ip", "to_v_ip"}) {   // (this block's pair is all the call reads)
            const std::string n = "ip_adapter." + std::to_string(2 * ipj + 1) + "." + w + ".weight";
            auto pi = e->index.find(n);
            if (pi == e->index.end() || !e->params[pi->second].loaded) { pd_set_error("weights not loaded: '%s'", n.c_str()); return 1; }
        }
    }
    e->ln_dirty = true;
    PD_TRY(e->fold_layernorms());
    const int C = st->C, D = e->cfg.context_dim, Dp = round_up(D, 8), lpad = round_up(L, 8), N = H * W;
    const size_t eb = dt_size(e->T);
    // a private workspace for this call (op hooks run outside a session)
    const size_t ws = (size_t)64 << 20, act = (size_t)B * N * C * 4;
    DevBuf work(ws + 48 * act), cin((size_t)B * L * D * 4), cdev((size_t)B * L * Dp * eb), kbuf((size_t)B * L * C * eb), vtbuf((size_t)B * C * lpad * eb),
        kvp(e->st_tail_on(*st, H * W, L) ? st_tail_kv_bytes(B, L) : 256), xin((size_t)B * N * C * dt_size(e->S));
    const size_t ntok = tokens ? (size_t)B * T : 0;
    DevBuf tin(ntok * D * 4), tdev(ntok * Dp * eb), kip(ntok * C * eb), vip(ntok * C * eb);
    if (!work.p || !cin.p || !cdev.p || !kbuf.p || !vtbuf.p || !kvp.p || !xin.p || !tin.p || !tdev.p || !kip.p || !vip.p) { pd_set_error("allocation failed"); return 1; }
    const Arena saved = e->arena;
    e->arena = Arena{};
    e->arena.base = reinterpret_cast<char*>(work.p);
    e->arena.cap = ws + 48 * act;
    int rc = 0;
    do {
        if ((rc = to_dev_nhwc(e, x, xin.p, e->S, B, C, H, W, C))) break;
        if (hipMemcpy(cin.p, ctx, (size_t)B * L * D * 4, hipMemcpyHostToDevice) != hipSuccess) { rc = 1; break; }
        if ((rc = launch_cast_rows(reinterpret_cast<const float*>(cin.p), cdev.p, e->T, (long long)B * L, D, Dp, e->stream))) break;
        Act c, k;
        c.p = cdev.p; c.B = B; c.H = L; c.W = 1; c.C = Dp; c.dt = e->T;
        k.p = kbuf.p; k.B = B; k.H = L; k.W = 1; k.C = C; k.dt = e->T;
        if ((rc = e->gemm(st->kv2, c, k, {.VT = vtbuf.p, .vt_begin = C, .vt_ld = lpad}))) break;
        KVSlot kv;
        kv.K = kbuf.p; kv.VT = vtbuf.p; kv.L = L;
        if (e->st_tail_on(*st, N, L) && st->tail_w) {
            if ((rc = launch_st_tail_kv_pack(kbuf.p, vtbuf.p, kvp.p, B, L, lpad, e->stream))) break;
            kv.P = kvp.p;
        }
        IpTerm term;
        const bool with_term = tokens && e->ip.scale[ipj] != 0.f;
        if (with_term) {
            if (hipMemcpy(tin.p, tokens, ntok * D * 4, hipMemcpyHostToDevice) != hipSuccess) { rc = 1; break; }
            if ((rc = launch_cast_rows(reinterpret_cast<const float*>(tin.p), tdev.p, e->T, (long long)ntok, D, Dp, e->stream))) break;
            Act t, ko, vo;
            t.p = tdev.p; t.B = (int)ntok; t.H = 1; t.W = 1; t.C = Dp; t.dt = e->T;
            ko = t; ko.p = kip.p; ko.C = C;
            vo = ko; vo.p = vip.p;
            if ((rc = e->gemm(e->ip.to_k[ipj], t, ko))) break;
            if ((rc = e->gemm(e->ip.to_v[ipj], t, vo))) break;
            term.K[0] = kip.p; term.V[0] = vip.p; term.nseg = 1; term.T = T; term.kv_bs = (long long)T * C; term.s = e->ip.scale[ipj];
        }
        Act a, o;
        a.p = xin.p; a.B = B; a.H = H; a.W = W; a.C = C; a.dt = e->S;
        const PagTerm pt{n_perturbed, false, B - n_perturbed};
        if ((rc = e->transformer(*st, a, o, kv, 0, with_term ? &term : nullptr, n_perturbed ? &pt : nullptr))) break;
        rc = from_dev_nhwc(e, o.p, e->S, y, B, C, H, W, C);
    } while (0);
    (void)hipStreamSynchronize(e->stream);
    e->arena = saved;
    return rc;
}


// timestep_embedding + time_embed MLP of a loaded network: the first two stages of pd_engine::compute_emb
int pd_op_timestep_embedding_i(const int64_t* t, int n, int dim, float* out) {
    if (!t || !out || n < 1 || dim < 2) { pd_set_error("bad argument"); return 1; }
    std::vector<float> host;
    pd_host_timestep_embedding(t, n, dim, host);
    std::memcpy(out, host.data(), host.size() * sizeof(float));
    return 0;
}

int pd_op_timestep_embedding_f(const double* t, int n, int dim, float* out) {
    if (!t || !out || n < 1 || dim < 2) { pd_set_error("bad argument"); return 1; }
    std::vector<float> host;
    pd_host_timestep_embedding_f(t, n, dim, host);
    std::memcpy(out, host.data(), host.size() * sizeof(float));
    return 0;
}

int pd_op_time_embed(pd_engine* e, int net, const int64_t* t, int n, float* temb, float* emb) {
    if (!e || !t || n < 1 || (!temb && !emb)) { pd_set_error("null argument"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    NetW& nw = net ? e->cnet : e->unet;
    const int mc = e->cfg.model_channels, td = mc * 4;
    std::vector<float> host;
    pd_host_timestep_embedding(t, n, mc, host);
    if (temb) memcpy(temb, host.data(), host.size() * sizeof(float));
    if (!emb) return 0;
    DevBuf a((size_t)n * mc * 4), b((size_t)n * td * 4), c((size_t)n * td * 4);
    if (!a.p || !b.p || !c.p) { pd_set_error("allocation failed"); return 1; }
    HIP_OK(hipMemcpy(a.p, host.data(), host.size() * 4, hipMemcpyHostToDevice));
    Act te, e1, e2;
    te.p = a.p; te.B = n; te.H = te.W = 1; te.C = mc; te.dt = DT_F32;
    e1 = te; e1.p = b.p; e1.C = td;
    e2 = e1; e2.p = c.p;
    PD_TRY(e->gemm(nw.te0, te, e1, {.act = ACT_SILU}));
    PD_TRY(e->gemm(nw.te2, e1, e2));
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(emb, c.p, (size_t)n * td * 4, hipMemcpyDeviceToHost));
    return 0;
}

// HED stage tail (launch_hed_stage_tail) in the compute type: NCHW fp32 in, score [B, H, W] and pooled NCHW fp32 out
int pd_op_hed_stage_tail(pd_engine* e, const float* x, const float* w, const float* bias, int B, int C, int H, int W, float* score,
                         float* pooled) {
    if (!e || !x || !w || !bias || !score) { pd_set_error("null argument"); return 1; }
    if (B < 1 || C < 8 || C % 8 || H < 1 || W < 1 || (pooled && ((H | W) & 1))) {
        pd_set_error("pd_op_hed_stage_tail: need B, H, W >= 1, C a positive multiple of 8, and even H, W with a pooled output");
        return 1;
    }
    HIP_OK(hipSetDevice(e->device));
    const int dt = e->T;
    const size_t px = (size_t)B * H * W;
    DevBuf dx(px * C * dt_size(dt)), dw((size_t)(C + 4) * 4), db(16), ds(px * 4), dp(px / 4 * C * dt_size(dt));
    if (!dx.p || !dw.p || !db.p || !ds.p || !dp.p) { pd_set_error("allocation failed"); return 1; }
    PD_TRY(to_dev_nhwc(e, x, dx.p, dt, B, C, H, W, C));
    HIP_OK(hipMemcpy(dw.p, w, (size_t)C * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(db.p, bias, 4, hipMemcpyHostToDevice));
    if (launch_hed_stage_tail(dx.p, dt, reinterpret_cast<const float*>(dw.p), reinterpret_cast<const float*>(db.p), reinterpret_cast<float*>(ds.p),
                              pooled ? dp.p : nullptr, B, H, W, C, e->stream)) {
        pd_set_error("pd_op_hed_stage_tail: launch failed");
        return 1;
    }
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(score, ds.p, px * 4, hipMemcpyDeviceToHost));
    return pooled ? from_dev_nhwc(e, dp.p, dt, pooled, B, C, H / 2, W / 2, C) : 0;
}

// HED fuse (launch_hed_fuse): fp32 score maps in, fp32 NCHW out
int pd_op_hed_fuse(pd_engine* e, const float* scores, const float* cw, const float* cb, int B, int H, int W, int what, float* out) {
    if (!e || !scores || !cw || !cb || !out) { pd_set_error("null argument"); return 1; }
    if (B < 1 || H < 16 || W < 16 || H % 16 || W % 16 || (what != PD_HED_EDGE && what != PD_HED_SIDES)) {
        pd_set_error("pd_op_hed_fuse: need B >= 1, H and W positive multiples of 16, what PD_HED_EDGE / PD_HED_SIDES");
        return 1;
    }
    HIP_OK(hipSetDevice(e->device));
    size_t off[6] = {0};
    for (int i = 0; i < 5; ++i) off[i + 1] = off[i] + (size_t)B * (H >> i) * (W >> i);
    const size_t n_out = (size_t)B * (what == PD_HED_SIDES ? 5 : 1) * H * W;
    DevBuf ds(off[5] * 4), dc(32), dout(n_out * 4);
    if (!ds.p || !dc.p || !dout.p) { pd_set_error("allocation failed"); return 1; }
    HIP_OK(hipMemcpy(ds.p, scores, off[5] * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dc.p, cw, 5 * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(reinterpret_cast<float*>(dc.p) + 5, cb, 4, hipMemcpyHostToDevice));
    const float* maps[5];
    for (int i = 0; i < 5; ++i) maps[i] = reinterpret_cast<const float*>(ds.p) + off[i];
    if (launch_hed_fuse(maps, reinterpret_cast<const float*>(dc.p), reinterpret_cast<const float*>(dc.p) + 5, reinterpret_cast<float*>(dout.p), B, H,
                        W, what, e->stream)) {
        pd_set_error("pd_op_hed_fuse: launch failed");
        return 1;
    }
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(out, dout.p, n_out * 4, hipMemcpyDeviceToHost));
    return 0;
}

// M-LSD depthwise conv3x3 + bias + ReLU6 (launch_mlsd_dwconv) in the compute type: NCHW fp32 in and out
int pd_op_dwconv3x3(pd_engine* e, const float* x, const float* w, const float* bias, int B, int C, int H, int W, int stride, int in_relu6,
                    float* y) {
    if (!e || !x || !w || !bias || !y) { pd_set_error("null argument"); return 1; }
    if (B < 1 || C < 8 || C % 8 || H < 1 || W < 1 || (stride != 1 && stride != 2) || (stride == 2 && ((H | W) & 1))) {
        pd_set_error("pd_op_dwconv3x3: need B, H, W >= 1, C a positive multiple of 8, stride 1 or 2, and even H, W at stride 2");
        return 1;
    }
    HIP_OK(hipSetDevice(e->device));
    const int dt = e->T, Ho = stride == 1 ? H : H / 2, Wo = stride == 1 ? W : W / 2;
    DevBuf dx((size_t)B * H * W * C * dt_size(dt)), dy((size_t)B * Ho * Wo * C * dt_size(dt)), dw((size_t)C * 9 * 4), db((size_t)C * 4);
    if (!dx.p || !dy.p || !dw.p || !db.p) { pd_set_error("allocation failed"); return 1; }
    PD_TRY(to_dev_nhwc(e, x, dx.p, dt, B, C, H, W, C));
    HIP_OK(hipMemcpy(dw.p, w, (size_t)C * 9 * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(db.p, bias, (size_t)C * 4, hipMemcpyHostToDevice));
    if (launch_mlsd_dwconv(dx.p, dy.p, dt, reinterpret_cast<const float*>(dw.p), reinterpret_cast<const float*>(db.p), B, H, W, C, stride,
                           in_relu6, e->stream)) {
        pd_set_error("pd_op_dwconv3x3: launch failed");
        return 1;
    }
    return from_dev_nhwc(e, dy.p, dt, y, B, C, Ho, Wo, C);
}

// M-LSD upsample into a concat buffer (launch_mlsd_upcat): y goes to the device, the kernel writes its channel range, y comes back
int pd_op_upcat_bilinear(pd_engine* e, const float* x, int B, int C, int h, int w, int Cy, int c_off, float* y) {
    if (!e || !x || !y) { pd_set_error("null argument"); return 1; }
    if (B < 1 || h < 1 || w < 1 || C < 8 || C % 8 || Cy % 8 || c_off % 8 || c_off < 0 || c_off + C > Cy) {
        pd_set_error("pd_op_upcat_bilinear: need B, h, w >= 1, C, Cy and c_off multiples of 8, and c_off + C <= Cy");
        return 1;
    }
    HIP_OK(hipSetDevice(e->device));
    const int dt = e->T;
    DevBuf dx((size_t)B * h * w * C * dt_size(dt)), dy((size_t)B * 4 * h * w * Cy * dt_size(dt));
    if (!dx.p || !dy.p) { pd_set_error("allocation failed"); return 1; }
    PD_TRY(to_dev_nhwc(e, x, dx.p, dt, B, C, h, w, C));
    PD_TRY(to_dev_nhwc(e, y, dy.p, dt, B, Cy, 2 * h, 2 * w, Cy));
    if (launch_mlsd_upcat(dx.p, C, reinterpret_cast<char*>(dy.p) + (size_t)c_off * dt_size(dt), Cy, dt, B, h, w, C, e->stream)) {
        pd_set_error("pd_op_upcat_bilinear: launch failed");
        return 1;
    }
    return from_dev_nhwc(e, dy.p, dt, y, B, Cy, 2 * h, 2 * w, Cy);
}

// y = [relu](conv2d(x, w, b, padding = dilation, dilation)); x NCHW fp32, w OIHW
int pd_op_conv2d_dilated(pd_engine* e, const float* x, const float* w, const float* bias, int B, int Cin, int H, int W, int Cout, int dilation,
                         int relu, float* y) {
    if (!e || !x || !w || !y) { pd_set_error("null argument"); return 1; }
    if (B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1 || dilation < 1) { pd_set_error("pd_op_conv2d_dilated: need B, Cin, Cout, H, W, dilation >= 1"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    TempMat guard(e);
    ConvW c;
    c.cin = Cin; c.cout = Cout; c.k = 3; c.stride = 1; c.dilation = dilation;
    e->make_mat(c.m, Cout, Cin * 9, 9, Cin, true);
    if (!c.m.w) { pd_set_error("allocation failed"); return 1; }
    PD_TRY(e->upload_rows(c.m, 0, w, Cout, true));
    if (bias) PD_TRY(e->upload_vec(c.m.bias, bias, Cout, false, 0));
    const int cpad = c.m.cin_pad, copad = round_up(Cout, 4);
    DevBuf in((size_t)B * H * W * cpad * dt_size(e->T)), out((size_t)B * H * W * copad * dt_size(e->T));
    if (!in.p || !out.p) { pd_set_error("allocation failed"); return 1; }
    PD_TRY(to_dev_nhwc(e, x, in.p, e->T, B, Cin, H, W, cpad));
    Act a, o;
    a.p = in.p; a.B = B; a.H = H; a.W = W; a.C = cpad; a.dt = e->T;
    o.p = out.p; o.B = B; o.H = H; o.W = W; o.C = copad; o.dt = e->T;
    PD_TRY(e->conv(c, a, o, {.act = relu ? ACT_RELU : ACT_NONE}));
    return from_dev_nhwc(e, out.p, e->T, y, B, Cout, H, W, copad);
}

int pd_op_mlsd_decode(pd_engine* e, const float* tp, int B, int h, int w, float thr_v, float thr_d, int32_t* segs, int32_t* count) {
    if (!e || !tp || !segs || !count) { pd_set_error("null argument"); return 1; }
    if (B < 1 || h < 1 || w < 1 || !std::isfinite(thr_v) || !std::isfinite(thr_d) || thr_v < 0.f) {
        pd_set_error("pd_op_mlsd_decode: need B, h, w >= 1 and finite thresholds with thr_v >= 0");
        return 1;
    }
    HIP_OK(hipSetDevice(e->device));
    const size_t n_tp = (size_t)B * 9 * h * w, n_seg = (size_t)B * MLSD_TOPK * 4;
    DevBuf dtp(n_tp * 4), dc((size_t)B * h * w * 8), dn((size_t)B * 4), ds(n_seg * 4), dk((size_t)B * 4);
    if (!dtp.p || !dc.p || !dn.p || !ds.p || !dk.p) { pd_set_error("allocation failed"); return 1; }
    HIP_OK(hipMemcpy(dtp.p, tp, n_tp * 4, hipMemcpyHostToDevice));
    if (launch_mlsd_decode(reinterpret_cast<const float*>(dtp.p), reinterpret_cast<unsigned long long*>(dc.p), reinterpret_cast<int*>(dn.p),
                           reinterpret_cast<int*>(ds.p), reinterpret_cast<int*>(dk.p), B, h, w, thr_v, thr_d, e->stream)) {
        pd_set_error("pd_op_mlsd_decode: launch failed");
        return 1;
    }
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(segs, ds.p, n_seg * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(count, dk.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    return 0;
}

int pd_op_draw_lines(pd_engine* e, const int32_t* segs, const int32_t* count, int B, int n, int H, int W, uint8_t* out) {
    if (!e || !segs || !count || !out) { pd_set_error("null argument"); return 1; }
    if (B < 1 || n < 1 || H < 1 || W < 1) { pd_set_error("pd_op_draw_lines: need B, n, H, W >= 1"); return 1; }
    for (int b = 0; b < B; ++b)
        if (count[b] < 0 || count[b] > n) { pd_set_error("pd_op_draw_lines: count[%d] = %d outside 0 .. %d", b, count[b], n); return 1; }
    HIP_OK(hipSetDevice(e->device));
    const size_t n_px = (size_t)B * H * W;
    DevBuf ds((size_t)B * n * 16), dk((size_t)B * 4), dm(n_px), d8(n_px);
    if (!ds.p || !dk.p || !dm.p || !d8.p) { pd_set_error("allocation failed"); return 1; }
    HIP_OK(hipMemcpy(ds.p, segs, (size_t)B * n * 16, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dk.p, count, (size_t)B * 4, hipMemcpyHostToDevice));
    if (launch_mlsd_draw(reinterpret_cast<const int*>(ds.p), reinterpret_cast<const int*>(dk.p), n, reinterpret_cast<uint8_t*>(dm.p), B, H, W,
                         e->stream) ||
        launch_canny_emit(reinterpret_cast<const uint8_t*>(dm.p), reinterpret_cast<uint8_t*>(d8.p), nullptr, B, H, W, 0, 0, 1.f, 0.f, e->stream)) {
        pd_set_error("pd_op_draw_lines: launch failed");
        return 1;
    }
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(out, d8.p, n_px, hipMemcpyDeviceToHost));
    return 0;
}

int pd_op_canny_hysteresis(pd_engine* e, const uint8_t* states, int B, int H, int W, int mem, uint8_t* out) {
    if (!e || !states || !out) { pd_set_error("null argument"); return 1; }
    if (B < 1 || H < 1 || W < 1) { pd_set_error("pd_op_canny_hysteresis: [%d, %d, %d]: sizes must be >= 1", B, H, W); return 1; }
    HIP_OK(hipSetDevice(e->device));
    const size_t n = (size_t)B * H * W;
    const bool dev = mem == PD_MEM_DEVICE;
    PD_TRY(e->image_grow(e->canny_states, n));   // the sweeps run in place on the engine's own map
    uint8_t* map = reinterpret_cast<uint8_t*>(e->canny_states.p);
    HIP_OK(hipMemcpyAsync(map, states, n, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
    PD_TRY(e->canny_hysteresis(map, B, H, W));
    HIP_OK(hipMemcpyAsync(out, map, n, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    return 0;
}

// sd3_update_kernel alone (launch_sd3_update) on copies of the caller's tensors
int pd_op_sd3_update(pd_engine* e, const float* v, const float* x, const float* z0, const float* mask, const float* eps, int B, int C,
                     int H, int W, int use_cfg, float guidance, float dsigma, float sigma, int pure, int seeded, int mem, float* x_out,
                     float* x_in_out) {
    if (!e || !x_out) { pd_set_error("null argument"); return 1; }
    if (B < 1 || C < 1 || H < 1 || W < 1 || B > 32) { pd_set_error("pd_op_sd3_update: bad shape (batch %d, latent %dx%dx%d)", B, C, H, W); return 1; }
    const bool step = v != nullptr, need_eps = !step || mask;
    if (step && !x) { pd_set_error("pd_op_sd3_update: a step needs x"); return 1; }
    if (mask && (!step || !z0)) { pd_set_error("pd_op_sd3_update: a mask needs v and z0"); return 1; }
    if (!step && !pure && !z0) { pd_set_error("pd_op_sd3_update: the start state needs z0 unless pure"); return 1; }
    if (seeded && eps) { pd_set_error("pd_op_sd3_update: seeded draws and an eps tensor exclude each other"); return 1; }
    if (need_eps && !seeded && !eps) { pd_set_error("pd_op_sd3_update: eps is required (or seeded)"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    const size_t n = (size_t)B * C * H * W, nm = (size_t)B * H * W, nv = (use_cfg ? 2 : 1) * n;
    const hipMemcpyKind kin = mem == PD_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind kout = mem == PD_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    DevBuf dv(nv * 4), dx(n * 4), dz(n * 4), dm(nm * 4), de(n * 4), dxin(2 * n * 4);
    if (!dv.p || !dx.p || !dz.p || !dm.p || !de.p || !dxin.p) { pd_set_error("allocation failed"); return 1; }
    auto up = [&](void* dst, const float* src, size_t cnt) { return src ? hipMemcpyAsync(dst, src, cnt * 4, kin, e->stream) : hipSuccess; };
    HIP_OK(up(dv.p, v, nv));
    HIP_OK(up(dx.p, x, n));
    HIP_OK(up(dz.p, z0, n));
    HIP_OK(up(dm.p, mask, nm));
    HIP_OK(up(de.p, eps, n));
    auto fp = [](const DevBuf& b, const void* given) { return given ? reinterpret_cast<float*>(b.p) : nullptr; };
    Sd3Update u;
    u.v = fp(dv, v); u.x = reinterpret_cast<float*>(dx.p); u.x_in = fp(dxin, x_in_out); u.z0 = fp(dz, z0); u.mask = fp(dm, mask);
    u.eps = fp(de, eps); u.rng_state = seeded ? e->rng_dev : nullptr;
    u.B = B; u.HW = H * W; u.per = (long long)C * H * W;
    u.guidance = guidance; u.dsigma = dsigma; u.sigma = sigma; u.use_cfg = use_cfg ? 1 : 0; u.pure = pure ? 1 : 0;
    if (launch_sd3_update(u, e->stream)) { pd_set_error("pd_op_sd3_update: launch failed"); return 1; }
    HIP_OK(hipMemcpyAsync(x_out, dx.p, n * 4, kout, e->stream));
    if (x_in_out) HIP_OK(hipMemcpyAsync(x_in_out, dxin.p, 2 * n * 4, kout, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    return 0;
}
}  // extern "C"
