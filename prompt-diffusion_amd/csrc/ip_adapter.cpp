// IP-Adapter image prompts for the SD1.5 UNet (declared in include/pdengine.h): the adapter's weights in a registry group of their own,
// the per-image state (pd_ip_adapter_set_image: projection, LayerNorm and the K / V GEMMs of every block, once per image), the scales,
// and what pd_engine::transformer calls per block and network evaluation -- one launch of ip_attention.hip per guidance half.
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/pdengine_ops.h"
#include "engine.h"

namespace {
bool ip_head_dim(int dh) { return dh == 8 || dh == 16 || dh == 32 || dh == 40 || dh == 80 || dh == 160; }

// tok [rows * T][D] in the compute type = LayerNorm(reshape(proj(emb) + bias)) of emb [rows][E] fp32 on the device; workspace from the arena
int ip_tokens(pd_engine* e, const float* emb, int rows, Act& tok) {
    const IpAdapterW& w = e->ip;
    const int D = e->cfg.context_dim;
    Act a = e->new_act(rows, 1, 1, w.E, e->T);
    PD_LAUNCH(e, launch_cast_rows(emb, a.p, e->T, rows, w.E, w.E, e->stream), "ip adapter: embedding cast launch failed");
    Act p = e->new_act(rows, 1, 1, w.T * D, e->T);
    PD_TRY(e->gemm(w.proj, a, p));
    Act pv = p;   // the same memory as [rows * T][D]
    pv.B = rows * w.T; pv.C = D;
    tok = e->new_act(rows * w.T, 1, 1, D, e->T);
    return e->layernorm(pv, tok, w.norm_g, w.norm_b, 1e-5f);
}
}  // namespace

bool pd_engine::ip_term(const STW& s, int Bf, bool use_cfg, IpTerm& t) const {
    if (s.ip_slot < 0 || !ip.active()) return false;
    const int j = s.ip_slot;
    if (ip.scale[j] == 0.f) return false;
    const size_t half = (size_t)ip.Bi * ip.T * s.C * dt_size(T);
    const char* k = reinterpret_cast<const char*>(ip.kv) + ip.k_off[j];
    const char* v = reinterpret_cast<const char*>(ip.kv) + ip.v_off[j];
    t = IpTerm{};
    t.T = ip.T;
    t.s = ip.scale[j];
    t.kv_bs = ip.Bi == 1 ? 0 : (long long)ip.T * s.C;
    if (use_cfg && Bf % 2 == 0) {   // [unconditional ; conditional]
        t.nseg = 2;
        t.K[0] = k; t.V[0] = v;
        t.K[1] = k + half; t.V[1] = v + half;
    } else {
        t.nseg = 1;
        t.K[0] = k + half; t.V[0] = v + half;
    }
    return true;
}

int pd_engine::ip_check_batch(int B) const {
    if (!ip.active() || ip.Bi == 1 || ip.Bi == B) return 0;
    pd_set_error("IP-Adapter: %d image embeddings are set, the sampling batch is %d (set 1, for every sample, or one per sample)", ip.Bi, B);
    return 1;
}

// att [Bt][N][C] += s * softmax(q K_ip^T) V_ip, one launch per run of the term; q_shared > 1: q2 holds the Bt / q_shared samples every run shares
int pd_engine::ip_image_term(const void* q2, void* att, const IpTerm& t, int Bt, int N, int C, int q_shared) {
    if (Bt % t.nseg || (q_shared > 1 && q_shared != t.nseg)) {
        pd_set_error("internal: image term of %d runs on a batch of %d (%d shared)", t.nseg, Bt, q_shared);
        return 1;
    }
    const int seg = Bt / t.nseg, heads = cfg.num_heads;
    const size_t run = (size_t)seg * N * C * dt_size(T);
    const float scale = (float)(1.0 / std::sqrt((double)(C / heads)));
    for (int r = 0; r < t.nseg; ++r) {
        const char* q = reinterpret_cast<const char*>(q2) + (q_shared > 1 ? 0 : r * run);
        char* a = reinterpret_cast<char*>(att) + r * run;
        if (!arena.dry) ++ip_launches;
        PD_LAUNCH(this, launch_ip_attention_add(q, a, t.K[r], t.V[r], t.kv_bs, seg, N, C, heads, t.T, scale, t.s, T, stream),
                  "IP-Adapter attention launch failed (C %d, heads %d, T %d)", C, heads, t.T);
    }
    return 0;
}

extern "C" {

int pd_ip_adapter_configure(pd_engine* e, const pd_ip_adapter_config* c) {
    if (!e || !c) { pd_set_error("pd_ip_adapter_configure: null argument"); return 1; }
    IpAdapterW& w = e->ip;
    if (w.built) {
        if (w.broken) { pd_set_error("pd_ip_adapter_configure: the weight allocation failed earlier; create a new engine"); return 1; }
        return 0;
    }
    const int D = e->cfg.context_dim;
    return e->configure("pd_ip_adapter_configure", GROUP_IP_ADAPTER, [&] {
        if (c->num_tokens < 1 || c->num_tokens > 64) { pd_set_error("pd_ip_adapter_configure: num_tokens %d outside 1 .. 64", c->num_tokens); return 1; }
        if (c->embed_dim < 8 || c->embed_dim % 8) { pd_set_error("pd_ip_adapter_configure: embed_dim %d must be a positive multiple of 8", c->embed_dim); return 1; }
        for (int32_t r : c->reserved)
            if (r) { pd_set_error("pd_ip_adapter_configure: reserved fields must be zero"); return 1; }
        if (D % 8) { pd_set_error("pd_ip_adapter_configure: context_dim %d must be a multiple of 8", D); return 1; }
        for (STW* s : e->unet.st_list)
            if (s->C % e->cfg.num_heads || !ip_head_dim(s->C / e->cfg.num_heads)) {
                pd_set_error("pd_ip_adapter_configure: no image-attention kernel for head dim %d / %d", s->C, e->cfg.num_heads);
                return 1;
            }
        return 0;
    }, [&] {
        w.T = c->num_tokens;
        w.E = c->embed_dim;
        e->make_mat(w.proj, w.T * D, w.E, 1, w.E, true);
        e->reg_mat("image_proj.proj.weight", {w.T * D, w.E}, &w.proj, 0, false);
        e->reg_bias("image_proj.proj.bias", &w.proj, 0, w.T * D);
        e->reg_vec("image_proj.norm.weight", D, &w.norm_g, 'g');
        e->reg_vec("image_proj.norm.bias", D, &w.norm_b, 'e');
        // diffusers' processor order: down blocks, up blocks, mid block
        for (EncBlock& b : e->unet.enc)
            if (b.kind == 1 && b.attn) w.blocks.push_back(&b.st);
        for (DecBlock& b : e->unet.dec)
            if (b.attn) w.blocks.push_back(&b.st);
        w.blocks.push_back(&e->unet.mid1);
        const int nb = (int)w.blocks.size();
        w.to_k.resize(nb);   // (sized once: the registry points into them)
        w.to_v.resize(nb);
        for (int j = 0; j < nb; ++j) {
            STW* s = w.blocks[j];
            const std::string p = "ip_adapter." + std::to_string(2 * j + 1) + ".";
            e->make_mat(w.to_k[j], s->C, D, 1, D, false);
            e->reg_mat(p + "to_k_ip.weight", {s->C, D}, &w.to_k[j], 0, false);
            e->make_mat(w.to_v[j], s->C, D, 1, D, false);
            e->reg_mat(p + "to_v_ip.weight", {s->C, D}, &w.to_v[j], 0, false);
            s->ip_slot = j;
        }
        w.scale.assign(nb, 1.f);
        w.built = true;
        w.broken = e->alloc_failed;
    });
}

int pd_ip_adapter_weights_missing(pd_engine* e) { return e && e->ip.built ? e->missing(GROUP_IP_ADAPTER) : 0; }

int pd_ip_adapter_set_scale(pd_engine* e, const float* scales, int32_t n) {
    if (!e || !scales) { pd_set_error("pd_ip_adapter_set_scale: null argument"); return 1; }
    IpAdapterW& w = e->ip;
    if (!w.built || w.broken) { pd_set_error("this engine has no IP-Adapter (pd_ip_adapter_configure)"); return 1; }
    const int nb = (int)w.blocks.size();
    if (n != 1 && n != nb) { pd_set_error("pd_ip_adapter_set_scale: %d scales (1, or one per cross-attention block: %d)", n, nb); return 1; }
    std::vector<float> v(nb);
    for (int j = 0; j < nb; ++j) {
        v[j] = scales[n == 1 ? 0 : j];
        if (!std::isfinite(v[j])) { pd_set_error("pd_ip_adapter_set_scale: scale %d is not finite", j); return 1; }
    }
    if (!memcmp(v.data(), w.scale.data(), nb * sizeof(float))) return 0;
    HIP_OK(hipSetDevice(e->device));
    e->clear_graphs();   // the scales are kernel arguments, and a zero removes launches
    w.scale = v;
    return 0;
}

int pd_ip_adapter_get_scale(pd_engine* e, float* scales, int32_t n) {
    if (!e || !scales) { pd_set_error("pd_ip_adapter_get_scale: null argument"); return 1; }
    const IpAdapterW& w = e->ip;
    if (!w.built || w.broken) { pd_set_error("this engine has no IP-Adapter (pd_ip_adapter_configure)"); return 1; }
    if (n != (int)w.blocks.size()) { pd_set_error("pd_ip_adapter_get_scale: room for %d scales, the adapter has %d", n, (int)w.blocks.size()); return 1; }
    memcpy(scales, w.scale.data(), (size_t)n * sizeof(float));
    return 0;
}

int pd_ip_adapter_clear_image(pd_engine* e) {
    if (!e) { pd_set_error("null engine"); return 1; }
    IpAdapterW& w = e->ip;
    if (!w.Bi) return 0;
    HIP_OK(hipSetDevice(e->device));
    e->clear_graphs();
    w.Bi = 0;
    ++w.gen;
    return 0;
}

int pd_ip_adapter_set_image(pd_engine* e, const float* cond, const float* uncond, int32_t Bi, int32_t mem) {
    if (!e || !cond || Bi < 1) { pd_set_error("pd_ip_adapter_set_image: bad argument"); return 1; }
    IpAdapterW& w = e->ip;
    if (!w.built || w.broken) { pd_set_error("this engine has no IP-Adapter (pd_ip_adapter_configure)"); return 1; }
    PD_TRY(e->require_loaded(GROUP_IP_ADAPTER, "IP-Adapter"));
    if (e->ses.active) { pd_set_error("pd_ip_adapter_set_image: end the sampling session first"); return 1; }
    HIP_OK(hipSetDevice(e->device));
    e->clear_graphs();   // captured loops hold the buffers' addresses and were captured against the old state
    const int nb = (int)w.blocks.size(), rows = 2 * Bi;
    const size_t eb = dt_size(e->T);
    // the buffers: per block K then V, each [2][Bi][T][C_j], 256-byte aligned
    size_t total = 0;
    std::vector<size_t> k_off(nb), v_off(nb);
    for (int j = 0; j < nb; ++j) {
        const size_t one = ((size_t)rows * w.T * w.blocks[j]->C * eb + 255) & ~(size_t)255;
        k_off[j] = total; v_off[j] = total + one;
        total += 2 * one;
    }
    w.Bi = 0;   // (no state while the buffers are rewritten; restored below on success)
    ++w.gen;
    if (total > w.kv_cap) {
        HIP_OK(hipStreamSynchronize(e->stream));
        if (e->stream2) HIP_OK(hipStreamSynchronize(e->stream2));
        if (w.kv) (void)hipFree(w.kv);
        w.kv = nullptr; w.kv_cap = 0;
        if (hipMalloc(&w.kv, total) != hipSuccess) { pd_set_error("pd_ip_adapter_set_image: allocation of %zu bytes failed", total); return 1; }
        w.kv_cap = total;
    }
    const int rc = e->side_call("IP-Adapter image", [&](SideCall& f) {
        // rows [0, Bi): the unconditional embeddings (zeros by default, as the reference's encode_image returns), [Bi, 2 Bi): the image's
        float* emb = f.scratch<float>((size_t)rows * w.E);
        if (!e->arena.dry) {
            PD_TRY(e->check_arena());
            const size_t half = (size_t)Bi * w.E * sizeof(float);
            const hipMemcpyKind kind = mem == PD_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
            if (uncond) HIP_OK(hipMemcpyAsync(emb, uncond, half, kind, e->stream));
            else HIP_OK(hipMemsetAsync(emb, 0, half, e->stream));
            HIP_OK(hipMemcpyAsync(emb + (size_t)Bi * w.E, cond, half, kind, e->stream));
        }
        Act tok;
        PD_TRY(ip_tokens(e, emb, rows, tok));
        for (int j = 0; j < nb; ++j) {
            Act k = tok, v = tok;
            k.C = v.C = w.blocks[j]->C;
            k.p = reinterpret_cast<char*>(w.kv) + k_off[j];
            v.p = reinterpret_cast<char*>(w.kv) + v_off[j];
            PD_TRY(e->gemm(w.to_k[j], tok, k));
            PD_TRY(e->gemm(w.to_v[j], tok, v));
        }
        return 0;
    });
    if (rc) return rc;
    w.k_off = k_off; w.v_off = v_off;
    w.Bi = Bi;
    return 0;
}

// The image term's kernel alone on random data in the compute type, and the yardstick next to it: `iters` back-to-back launches between
// two events, then `iters` device-to-device copies of the 3 B N C elements the kernel moves (q2 and att read, att written)
int pd_bench_ip_attention(pd_engine* e, int32_t B, int32_t N, int32_t C, int32_t T, int32_t iters, float* ms_kernel, float* ms_copy) {
    if (!e || !ms_kernel || !ms_copy || iters < 1 || B < 1 || N < 1 || T < 1 || T > 64 || C < 8 || C % 8 || C % e->cfg.num_heads) {
        pd_set_error("pd_bench_ip_attention: bad argument");
        return 1;
    }
    HIP_OK(hipSetDevice(e->device));
    const size_t eb = dt_size(e->T), n = (size_t)B * N * C, nk = (size_t)T * C;
    const int heads = e->cfg.num_heads;
    void *q = nullptr, *a = nullptr, *k = nullptr, *v = nullptr, *src = nullptr, *dst = nullptr;
    int rc = 0;
    if (hipMalloc(&q, n * eb) != hipSuccess || hipMalloc(&a, n * eb) != hipSuccess || hipMalloc(&k, nk * eb) != hipSuccess ||
        hipMalloc(&v, nk * eb) != hipSuccess || hipMalloc(&src, 3 * n * eb) != hipSuccess || hipMalloc(&dst, 3 * n * eb) != hipSuccess) {
        pd_set_error("pd_bench_ip_attention: allocation failed");
        rc = 1;
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!rc && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) { pd_set_error("hipEventCreate failed"); rc = 1; }
    if (!rc) {
        launch_fill_random(q, e->T, (long long)n, 1.f, 0.f, 1, e->stream);
        launch_fill_random(a, e->T, (long long)n, 1.f, 0.f, 2, e->stream);
        launch_fill_random(k, e->T, (long long)nk, 1.f, 0.f, 3, e->stream);
        launch_fill_random(v, e->T, (long long)nk, 1.f, 0.f, 4, e->stream);
        launch_fill_random(src, e->T, (long long)(3 * n), 1.f, 0.f, 5, e->stream);
        const float scale = (float)(1.0 / std::sqrt((double)(C / heads)));
        // (s = 0: att stays what it is however often the kernel runs on it; the arithmetic does not depend on s)
        auto run = [&] { return launch_ip_attention_add(q, a, k, v, 0, B, N, C, heads, T, scale, 0.f, e->T, e->stream); };
        for (int i = 0; i < 3 && !rc; ++i) rc = run();
        if (!rc) {
            hipEventRecord(e0, e->stream);
            for (int i = 0; i < iters && !rc; ++i) rc = run();
            hipEventRecord(e1, e->stream);
            hipEventSynchronize(e1);
            float t = 0.f;
            hipEventElapsedTime(&t, e0, e1);
            *ms_kernel = t / (float)iters;
        }
        if (rc) pd_set_error("pd_bench_ip_attention: launch failed or shape refused (C %d, heads %d, T %d)", C, heads, T);
    }
    if (!rc) {
        for (int i = 0; i < 3; ++i) hipMemcpyAsync(dst, src, 3 * n * eb, hipMemcpyDeviceToDevice, e->stream);
        hipEventRecord(e0, e->stream);
        for (int i = 0; i < iters; ++i) hipMemcpyAsync(dst, src, 3 * n * eb, hipMemcpyDeviceToDevice, e->stream);
        hipEventRecord(e1, e->stream);
        hipEventSynchronize(e1);
        float t = 0.f;
        hipEventElapsedTime(&t, e0, e1);
        *ms_copy = t / (float)iters;
    }
    hipStreamSynchronize(e->stream);
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    for (void* p : {q, a, k, v, src, dst})
        if (p) hipFree(p);
    return rc;
}
}
