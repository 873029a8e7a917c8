// LoRA adapters merged in place into the engine's matrix weights (pd_lora_*; DESIGN.md §7 "LoRA adapters").
//
// Every matrix parameter an adapter touches becomes a target: the first adapter saves the parameter's rows as the base copy
// W0 (in the storage type T, in the WMat's own row layout), and each adapter's factors are kept on the device as up^T
// [r][rows] and down [r][Kpad] (laid out like upload_rows lays out a row: k = tap * cin_pad + c, zero pad columns).  A merge
// rebuilds W from W0 with lora_merge_kernel (lora.hip), so the weights never depend on the order of earlier scale changes;
// adapters that are not a stack of rank-1 columns (pd_lora_add_ex: Hadamard and Kronecker products, a DoRA magnitude) are
// kept as LoraForm records and merged after the plain columns, in load order, by the form kernels of lora.hip.  A merge
// then marks the derived copies stale (folded LayerNorm weights, fused st_tail packs, SD3 e4m3 copies), drops captured
// graphs, refolds the LayerNorms and synchronises.  The sampling path itself is unchanged.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>

static bool all_finite(const float* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

static int dev_alloc(void** p, size_t bytes) {
    *p = nullptr;
    if (hipMalloc(p, bytes ? bytes : 16) != hipSuccess) {
        *p = nullptr;
        pd_set_error("LoRA: hipMalloc of %zu bytes failed", bytes);
        return 1;
    }
    return 0;
}

// rows of the WMat a target's base copy holds: the parameter's rows, or all m.N rows of a GEGLU matrix (row_off 0)
static int base_rows(const Param& p) { return p.mat->geglu ? p.mat->N : (int)p.shape[0]; }

int pd_engine::lora_add(int adapter, const char* name, const float* up, int up_rows, int rank, const float* down,
                        const int64_t* ds, int dn) {
    if (ses.active) { pd_set_error("pd_lora_add: end the sampling session first"); return 1; }
    if (adapter < 0) { pd_set_error("pd_lora_add: '%s': adapter id %d must be >= 0", name, adapter); return 1; }
    auto it = index.find(name);
    if (it == index.end()) { pd_set_error("pd_lora_add: unknown tensor '%s'", name); return 2; }
    const int pi = it->second;
    const Param& p = params[pi];
    if (p.kind != 1) { pd_set_error("pd_lora_add: '%s' is a vector parameter (bias / norm); adapters apply to matrices", name); return 3; }
    if (rank <= 0) { pd_set_error("pd_lora_add: '%s': rank %d must be positive", name, rank); return 3; }
    WMat& m = *p.mat;
    const int rows = (int)p.shape[0];
    if (up_rows != rows) { pd_set_error("pd_lora_add: '%s': up has %d rows, the parameter has %d", name, up_rows, rows); return 3; }
    const int kk = m.taps, cin = m.cin;
    bool ok = false;
    if (dn == 2) ok = ds[0] == rank && ds[1] == (int64_t)cin * kk;
    else if (dn == 4)
        ok = ds[0] == rank && ds[1] == cin && ds[2] * ds[3] == kk && (!p.conv || (ds[2] == p.shape[2] && ds[3] == p.shape[3]));
    if (!ok) {
        pd_set_error("pd_lora_add: '%s': down must be [%d, %d] or [%d, %d, kh, kw] with kh * kw = %d (got %d dims)", name, rank, cin * kk,
                     rank, cin, kk, dn);
        return 3;
    }
    if (!all_finite(up, (size_t)rows * rank) || !all_finite(down, (size_t)rank * cin * kk)) {
        pd_set_error("pd_lora_add: '%s': up / down hold non-finite values", name);
        return 3;
    }
    auto tit = lora.find(pi);
    if (tit != lora.end())
        for (const LoraEntry& en : tit->second.entries)
            if (en.adapter == adapter) { pd_set_error("pd_lora_add: '%s' already has adapter %d", name, adapter); return 3; }
    if (tit != lora.end())
        for (const LoraForm& fo : tit->second.forms)
            if (fo.adapter == adapter) { pd_set_error("pd_lora_add: '%s' already has adapter %d", name, adapter); return 3; }
    HIP_OK(hipSetDevice(device));
    // host layout of the new columns
    std::vector<float> ut((size_t)rank * rows), d((size_t)rank * m.Kpad, 0.f);
    for (int n = 0; n < rows; ++n)
        for (int j = 0; j < rank; ++j) ut[(size_t)j * rows + n] = up[(size_t)n * rank + j];
    for (int j = 0; j < rank; ++j)
        for (int c = 0; c < cin; ++c)
            for (int tp = 0; tp < kk; ++tp) d[(size_t)j * m.Kpad + (size_t)tp * m.cin_pad + c] = down[((size_t)j * cin + c) * kk + tp];
    PD_TRY(lora_target_base(pi));
    LoraTarget& t = lora[pi];
    void *nut = nullptr, *nd = nullptr;
    const int R = t.R + rank;
    PD_TRY(dev_alloc(&nut, (size_t)R * rows * 4));
    if (dev_alloc(&nd, (size_t)R * m.Kpad * 4)) { hipFree(nut); return 1; }
    if (t.R) {
        HIP_OK(hipMemcpyAsync(nut, t.ut, (size_t)t.R * rows * 4, hipMemcpyDeviceToDevice, stream));
        HIP_OK(hipMemcpyAsync(nd, t.d, (size_t)t.R * m.Kpad * 4, hipMemcpyDeviceToDevice, stream));
    }
    HIP_OK(hipMemcpyAsync(reinterpret_cast<float*>(nut) + (size_t)t.R * rows, ut.data(), ut.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_OK(hipMemcpyAsync(reinterpret_cast<float*>(nd) + (size_t)t.R * m.Kpad, d.data(), d.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_OK(hipStreamSynchronize(stream));   // (ut / d above are host temporaries; the old buffers are freed next)
    if (t.ut) hipFree(t.ut);
    if (t.d) hipFree(t.d);
    t.ut = reinterpret_cast<float*>(nut);
    t.d = reinterpret_cast<float*>(nd);
    t.R = R;
    t.entries.push_back({adapter, rank});
    if (!t.merged.empty() || !t.fmerged.empty()) t.merged.push_back(0.f);   // W does not hold the new columns yet
    lora_scale.emplace(adapter, 0.f);
    return lora_merge(pi, false);   // a no-op unless the adapter is already active
}

int pd_engine::lora_target_base(int pi) {
    const Param& p = params[pi];
    WMat& m = *p.mat;
    LoraTarget& t = lora[pi];
    if (t.w0) return 0;
    const size_t rowb = (size_t)m.Kpad * dt_size(T);
    t.w0_bytes = (size_t)base_rows(p) * rowb;   // first adapter on this parameter: W holds the base weights now
    if (dev_alloc(&t.w0, t.w0_bytes)) { lora.erase(pi); return 1; }
    HIP_OK(hipMemcpyAsync(t.w0, reinterpret_cast<char*>(m.w) + (size_t)(m.geglu ? 0 : p.row_off) * rowb, t.w0_bytes,
                          hipMemcpyDeviceToDevice, stream));
    return 0;
}

// up [rows][r] -> up^T [r][rows] times `scale`; down [r][cin][taps] -> [r][Kpad] in the WMat's column layout
static void lay_pair(const WMat& m, int rows, int r, float scale, const float* up, const float* down, float* ut, float* d) {
    for (int n = 0; n < rows; ++n)
        for (int j = 0; j < r; ++j) ut[(size_t)j * rows + n] = scale * up[(size_t)n * r + j];
    for (int j = 0; j < r; ++j)
        for (int c = 0; c < m.cin; ++c)
            for (int tp = 0; tp < m.taps; ++tp)
                d[(size_t)j * m.Kpad + (size_t)tp * m.cin_pad + c] = down[((size_t)j * m.cin + c) * m.taps + tp];
}

int pd_engine::lora_add_ex(int adapter, const char* name, const pd_lora_factors& f) {
    if (ses.active) { pd_set_error("pd_lora_add_ex: end the sampling session first"); return 1; }
    if (adapter < 0) { pd_set_error("pd_lora_add_ex: '%s': adapter id %d must be >= 0", name, adapter); return 1; }
    auto it = index.find(name);
    if (it == index.end()) { pd_set_error("pd_lora_add_ex: unknown tensor '%s'", name); return 2; }
    const int pi = it->second;
    const Param& p = params[pi];
    if (p.kind != 1) { pd_set_error("pd_lora_add_ex: '%s' is a vector parameter (bias / norm); adapters apply to matrices", name); return 3; }
    if (f.kind != PD_LORA_PAIR && f.kind != PD_LORA_HADA && f.kind != PD_LORA_KRON) {
        pd_set_error("pd_lora_add_ex: '%s': unknown kind %d", name, f.kind);
        return 3;
    }
    if (!f.up || !f.down || (f.kind == PD_LORA_HADA && (!f.up2 || !f.down2))) { pd_set_error("pd_lora_add_ex: '%s': null factor", name); return 3; }
    if (!std::isfinite(f.scale)) { pd_set_error("pd_lora_add_ex: '%s': non-finite scale", name); return 3; }
    WMat& m = *p.mat;
    const int rows = (int)p.shape[0], kk = m.taps, cin = m.cin;
    const size_t K = (size_t)cin * kk;
    const bool kron = f.kind == PD_LORA_KRON, hada = f.kind == PD_LORA_HADA;
    size_t n_u1, n_d1, n_u2 = 0, n_d2 = 0;   // floats of each host factor
    if (kron) {
        if (f.kron_a <= 0 || f.kron_b <= 0 || rows % f.kron_a != 0 || cin % f.kron_b != 0) {
            pd_set_error("pd_lora_add_ex: '%s': w1 [%d, %d] does not divide the parameter's [%d, %d] (a * c = N and b * d = cin)", name,
                         f.kron_a, f.kron_b, rows, cin);
            return 3;
        }
        n_u1 = (size_t)f.kron_a * f.kron_b;
        n_d1 = (size_t)(rows / f.kron_a) * (cin / f.kron_b) * kk;
    } else {
        if (f.rank <= 0 || (hada && f.rank2 <= 0)) { pd_set_error("pd_lora_add_ex: '%s': rank %d must be positive", name, hada && f.rank > 0 ? f.rank2 : f.rank); return 3; }
        n_u1 = (size_t)rows * f.rank;
        n_d1 = (size_t)f.rank * K;
        if (hada) { n_u2 = (size_t)rows * f.rank2; n_d2 = (size_t)f.rank2 * K; }
    }
    if (!all_finite(f.up, n_u1) || !all_finite(f.down, n_d1) || (hada && (!all_finite(f.up2, n_u2) || !all_finite(f.down2, n_d2))) ||
        (f.magnitude && !all_finite(f.magnitude, rows))) {
        pd_set_error("pd_lora_add_ex: '%s': factors hold non-finite values", name);
        return 3;
    }
    if (f.kind == PD_LORA_PAIR && !f.magnitude) {   // a plain pair: the stacked columns of pd_lora_add
        std::vector<float> up(n_u1);
        for (size_t i = 0; i < n_u1; ++i) up[i] = f.scale * f.up[i];
        const int64_t ds[2] = {f.rank, (int64_t)K};
        return lora_add(adapter, name, up.data(), rows, f.rank, f.down, ds, 2);
    }
    auto tit = lora.find(pi);
    if (tit != lora.end()) {
        bool dup = false;
        for (const LoraEntry& en : tit->second.entries) dup = dup || en.adapter == adapter;
        for (const LoraForm& fo : tit->second.forms) dup = dup || fo.adapter == adapter;
        if (dup) { pd_set_error("pd_lora_add_ex: '%s' already has adapter %d", name, adapter); return 3; }
    }
    HIP_OK(hipSetDevice(device));
    // device layout, every part a multiple of 4 floats
    auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
    const size_t o_u1 = 0, s_u1 = kron ? n_u1 : (size_t)f.rank * rows;
    const size_t o_d1 = o_u1 + up4(s_u1), s_d1 = kron ? n_d1 : (size_t)f.rank * m.Kpad;
    const size_t o_u2 = o_d1 + up4(s_d1), s_u2 = hada ? (size_t)f.rank2 * rows : 0;
    const size_t o_d2 = o_u2 + up4(s_u2), s_d2 = hada ? (size_t)f.rank2 * m.Kpad : 0;
    const size_t o_mg = o_d2 + up4(s_d2), total = o_mg + up4(f.magnitude ? rows : 0);
    std::vector<float> h(total, 0.f);
    if (kron) {
        const int c = rows / f.kron_a, d = cin / f.kron_b;
        for (size_t i = 0; i < n_u1; ++i) h[o_u1 + i] = f.scale * f.up[i];
        for (int pp = 0; pp < c; ++pp)
            for (int q = 0; q < d; ++q)
                for (int tp = 0; tp < kk; ++tp) h[o_d1 + ((size_t)pp * kk + tp) * d + q] = f.down[((size_t)pp * d + q) * kk + tp];
    } else {
        lay_pair(m, rows, f.rank, f.scale, f.up, f.down, &h[o_u1], &h[o_d1]);
        if (hada) lay_pair(m, rows, f.rank2, 1.f, f.up2, f.down2, &h[o_u2], &h[o_d2]);
    }
    if (f.magnitude) memcpy(&h[o_mg], f.magnitude, (size_t)rows * 4);
    PD_TRY(lora_target_base(pi));
    LoraTarget& t = lora[pi];
    void* q = nullptr;
    PD_TRY(dev_alloc(&q, total * 4));
    LoraForm fo;
    fo.adapter = adapter; fo.kind = f.kind; fo.r1 = kron ? 0 : f.rank; fo.r2 = hada ? f.rank2 : 0;
    fo.ka = kron ? f.kron_a : 0; fo.kb = kron ? f.kron_b : 0;
    fo.buf = reinterpret_cast<float*>(q);
    fo.bytes = total * 4;
    fo.ut1 = fo.buf + o_u1; fo.d1 = fo.buf + o_d1;
    if (hada) { fo.ut2 = fo.buf + o_u2; fo.d2 = fo.buf + o_d2; }
    if (f.magnitude) fo.mag = fo.buf + o_mg;
    if (hipMemcpyAsync(q, h.data(), total * 4, hipMemcpyHostToDevice, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
        hipFree(q);
        pd_set_error("pd_lora_add_ex: '%s': upload failed", name);
        return 1;
    }
    t.forms.push_back(fo);
    if (!t.merged.empty() || !t.fmerged.empty()) t.fmerged.push_back(0.f);   // W does not hold the new adapter yet
    lora_scale.emplace(adapter, 0.f);
    return lora_merge(pi, false);   // a no-op unless the adapter is already active
}

int pd_engine::lora_set_scales(const float* scales, int n) {
    if (ses.active) { pd_set_error("pd_lora_set_scales: end the sampling session first"); return 1; }
    if (n < 0 || (n > 0 && !scales)) { pd_set_error("pd_lora_set_scales: bad scale array (n = %d)", n); return 1; }
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(scales[i])) { pd_set_error("pd_lora_set_scales: non-finite scale %g for adapter %d", scales[i], i); return 1; }
        if (scales[i] != 0.f && !lora_scale.count(i)) { pd_set_error("pd_lora_set_scales: unknown adapter id %d", i); return 1; }
    }
    for (auto& kv : lora_scale) kv.second = kv.first < n ? scales[kv.first] : 0.f;
    return lora_merge(-1, false);
}

// restores / merges every target (or one) whose adapters' multipliers differ from what W holds
int pd_engine::lora_merge(int only, bool force) {
    struct Job { int pi; LoraTarget* t; size_t off; bool plain, forms; };
    std::vector<Job> jobs;
    std::vector<float> cols;
    bool changed = false;
    size_t scratch = 0;
    HIP_OK(hipSetDevice(device));
    for (auto& kv : lora) {
        if (only >= 0 && kv.first != only) continue;
        LoraTarget& t = kv.second;
        std::vector<float> want(t.entries.size()), fwant(t.forms.size());
        bool plain = false, forms = false;
        for (size_t i = 0; i < t.entries.size(); ++i) {
            want[i] = lora_scale[t.entries[i].adapter];
            plain = plain || want[i] != 0.f;
        }
        for (size_t i = 0; i < t.forms.size(); ++i) {
            fwant[i] = lora_scale[t.forms[i].adapter];
            forms = forms || fwant[i] != 0.f;
        }
        if (!plain && !forms) { want.clear(); fwant.clear(); }
        if (!force && want == t.merged && fwant == t.fmerged) continue;
        const Param& p = params[kv.first];
        WMat& m = *p.mat;
        const size_t rowb = (size_t)m.Kpad * dt_size(T);
        if (!plain && !forms) {   // no active adapter: W0 exactly
            HIP_OK(hipMemcpyAsync(reinterpret_cast<char*>(m.w) + (size_t)(m.geglu ? 0 : p.row_off) * rowb, t.w0, t.w0_bytes,
                                  hipMemcpyDeviceToDevice, stream));
        } else {
            jobs.push_back({kv.first, &t, cols.size(), plain, forms});
            for (size_t i = 0; i < t.entries.size(); ++i) cols.insert(cols.end(), (size_t)t.entries[i].r, want[i]);
            if (forms) scratch = std::max(scratch, (size_t)p.shape[0] * m.Kpad);
        }
        t.merged = want;
        t.fmerged = fwant;
        changed = true;
    }
    if (!changed) return 0;
    if (scratch > lora_tmp_cap) {
        HIP_OK(hipStreamSynchronize(stream));
        if (lora_tmp) hipFree(lora_tmp);
        if (lora_sum) hipFree(lora_sum);
        lora_tmp = lora_sum = nullptr;
        lora_tmp_cap = 0;
        void *q0 = nullptr, *q1 = nullptr;
        PD_TRY(dev_alloc(&q0, scratch * 4));
        if (dev_alloc(&q1, scratch * 4)) { hipFree(q0); return 1; }
        lora_tmp = reinterpret_cast<float*>(q0);
        lora_sum = reinterpret_cast<float*>(q1);
        lora_tmp_cap = scratch;
    }
    if (!jobs.empty()) {
        if (cols.size() > lora_scale_cap) {
            HIP_OK(hipStreamSynchronize(stream));
            if (lora_scale_dev) hipFree(lora_scale_dev);
            lora_scale_cap = 0;
            void* q = nullptr;
            PD_TRY(dev_alloc(&q, cols.size() * 4));
            lora_scale_dev = reinterpret_cast<float*>(q);
            lora_scale_cap = cols.size();
        }
        if (!cols.empty()) HIP_OK(hipMemcpyAsync(lora_scale_dev, cols.data(), cols.size() * 4, hipMemcpyHostToDevice, stream));
        for (const Job& j : jobs) {
            const Param& p = params[j.pi];
            WMat& m = *p.mat;
            const int rows = (int)p.shape[0], row_off = m.geglu ? 0 : p.row_off, half = m.geglu ? m.Nout : 0;
            int rc = 0;
            if (!j.forms) {   // plain adapters only: the one merge kernel
                rc = launch_lora_merge(T, m.w, j.t->w0, rows, row_off, half, m.Kpad, j.t->ut, j.t->d, lora_scale_dev + j.off, j.t->R, stream);
            } else {          // W0, then the plain columns, then each active form in load order, in fp32; rounded once by the last
                int left = j.plain ? 1 : 0, first = 1;
                for (float s : j.t->fmerged) left += s != 0.f;
                if (j.plain) {
                    rc = launch_lora_form_delta(lora_tmp, rows, m.Kpad, j.t->ut, j.t->d, lora_scale_dev + j.off, 0.f, j.t->R, nullptr, nullptr, 0,
                                                stream) ||
                         launch_lora_form_apply(T, m.w, j.t->w0, lora_sum, lora_tmp, nullptr, rows, row_off, half, m.Kpad, first, --left == 0,
                                                stream);
                    first = 0;
                }
                for (size_t i = 0; i < j.t->forms.size() && !rc; ++i) {
                    const LoraForm& fo = j.t->forms[i];
                    const float s = j.t->fmerged[i];
                    if (s == 0.f) continue;
                    if (fo.kind == PD_LORA_KRON)
                        rc = launch_lora_kron_delta(lora_tmp, rows, m.Kpad, m.cin, m.cin_pad, m.taps, fo.ut1, fo.d1, s, fo.ka, fo.kb, stream);
                    else
                        rc = launch_lora_form_delta(lora_tmp, rows, m.Kpad, fo.ut1, fo.d1, nullptr, s, fo.r1, fo.ut2, fo.d2, fo.r2, stream);
                    rc = rc || launch_lora_form_apply(T, m.w, j.t->w0, lora_sum, lora_tmp, fo.mag, rows, row_off, half, m.Kpad, first,
                                                      --left == 0, stream);
                    first = 0;
                }
            }
            if (rc) {
                pd_set_error("LoRA merge launch failed for '%s'", p.name.c_str());
                return 1;
            }
        }
    }
    ln_dirty = true;
    sd3_fp8_dirty = true;
    clear_graphs();
    PD_TRY(fold_layernorms());
    HIP_OK(hipStreamSynchronize(stream));   // (cols is a host temporary)
    return 0;
}

// the base weights of targets were just written into W (pd_load_weights / pd_init_random_weights): take them as W0, merge again
int pd_engine::lora_rebase(int only) {
    HIP_OK(hipSetDevice(device));
    bool any = false;
    for (auto& kv : lora) {
        if (only >= 0 && kv.first != only) continue;
        const Param& p = params[kv.first];
        const size_t rowb = (size_t)p.mat->Kpad * dt_size(T);
        HIP_OK(hipMemcpyAsync(kv.second.w0, reinterpret_cast<char*>(p.mat->w) + (size_t)(p.mat->geglu ? 0 : p.row_off) * rowb,
                              kv.second.w0_bytes, hipMemcpyDeviceToDevice, stream));
        any = true;
    }
    return any ? lora_merge(only, true) : 0;
}

int pd_engine::lora_remove(int adapter) {
    if (ses.active) { pd_set_error("pd_lora_remove: end the sampling session first"); return 1; }
    if (adapter != -1 && !lora_scale.count(adapter)) { pd_set_error("pd_lora_remove: unknown adapter id %d", adapter); return 1; }
    HIP_OK(hipSetDevice(device));
    std::vector<int> emptied, restack;
    for (auto& kv : lora) {
        LoraTarget& t = kv.second;
        bool hit = false;
        for (const LoraEntry& en : t.entries) hit = hit || adapter == -1 || en.adapter == adapter;
        for (const LoraForm& fo : t.forms) hit = hit || adapter == -1 || fo.adapter == adapter;
        if (!hit) continue;
        const Param& p = params[kv.first];
        WMat& m = *p.mat;
        std::vector<LoraEntry> keep;
        for (const LoraEntry& en : t.entries)
            if (adapter != -1 && en.adapter != adapter) keep.push_back(en);
        std::vector<LoraForm> fkeep;
        for (const LoraForm& fo : t.forms) {   // (every merge ends synchronised: nothing in flight reads a form's buffer)
            if (adapter != -1 && fo.adapter != adapter) fkeep.push_back(fo);
            else hipFree(fo.buf);
        }
        t.forms = fkeep;
        if (keep.empty() && fkeep.empty()) {
            const size_t rowb = (size_t)m.Kpad * dt_size(T);
            HIP_OK(hipMemcpyAsync(reinterpret_cast<char*>(m.w) + (size_t)(m.geglu ? 0 : p.row_off) * rowb, t.w0, t.w0_bytes,
                                  hipMemcpyDeviceToDevice, stream));
            emptied.push_back(kv.first);
            continue;
        }
        restack.push_back(kv.first);
        if (keep.size() == t.entries.size()) continue;   // only a form left
        if (keep.empty()) {
            hipFree(t.ut);
            hipFree(t.d);
            t.ut = t.d = nullptr;
            t.R = 0;
            t.entries.clear();
            continue;
        }
        // restack the kept adapters' columns, in their load order
        const int rows = (int)p.shape[0];
        int R = 0;
        for (const LoraEntry& en : keep) R += en.r;
        void *nut = nullptr, *nd = nullptr;
        PD_TRY(dev_alloc(&nut, (size_t)R * rows * 4));
        if (dev_alloc(&nd, (size_t)R * m.Kpad * 4)) { hipFree(nut); return 1; }
        int src = 0, dst = 0;
        for (const LoraEntry& en : t.entries) {
            if (adapter == -1 || en.adapter != adapter) {
                HIP_OK(hipMemcpyAsync(reinterpret_cast<float*>(nut) + (size_t)dst * rows, t.ut + (size_t)src * rows, (size_t)en.r * rows * 4,
                                      hipMemcpyDeviceToDevice, stream));
                HIP_OK(hipMemcpyAsync(reinterpret_cast<float*>(nd) + (size_t)dst * m.Kpad, t.d + (size_t)src * m.Kpad,
                                      (size_t)en.r * m.Kpad * 4, hipMemcpyDeviceToDevice, stream));
                dst += en.r;
            }
            src += en.r;
        }
        HIP_OK(hipStreamSynchronize(stream));
        hipFree(t.ut);
        hipFree(t.d);
        t.ut = reinterpret_cast<float*>(nut);
        t.d = reinterpret_cast<float*>(nd);
        t.R = R;
        t.entries = keep;
    }
    HIP_OK(hipStreamSynchronize(stream));
    for (int pi : emptied) {
        LoraTarget& t = lora[pi];
        hipFree(t.w0);
        if (t.ut) hipFree(t.ut);
        if (t.d) hipFree(t.d);
        lora.erase(pi);
    }
    if (adapter == -1) lora_scale.clear();
    else lora_scale.erase(adapter);
    for (int pi : restack) PD_TRY(lora_merge(pi, true));
    if (!emptied.empty() && restack.empty()) {   // (lora_merge did this otherwise)
        ln_dirty = true;
        sd3_fp8_dirty = true;
        clear_graphs();
        PD_TRY(fold_layernorms());
        HIP_OK(hipStreamSynchronize(stream));
    }
    return 0;
}

void pd_engine::lora_release() {
    for (auto& kv : lora) {
        if (kv.second.w0) hipFree(kv.second.w0);
        if (kv.second.ut) hipFree(kv.second.ut);
        if (kv.second.d) hipFree(kv.second.d);
        for (const LoraForm& fo : kv.second.forms) hipFree(fo.buf);
    }
    if (lora_tmp) hipFree(lora_tmp);
    if (lora_sum) hipFree(lora_sum);
    lora_tmp = lora_sum = nullptr;
    lora_tmp_cap = 0;
    lora.clear();
    lora_scale.clear();
    if (lora_scale_dev) hipFree(lora_scale_dev);
    lora_scale_dev = nullptr;
    lora_scale_cap = 0;
}

size_t pd_engine::lora_bytes(bool base_only) const {
    size_t b = 0;
    for (const auto& kv : lora) {
        b += kv.second.w0_bytes;
        if (!base_only) b += (size_t)kv.second.R * ((size_t)params[kv.first].shape[0] + params[kv.first].mat->Kpad) * 4;
        if (!base_only)
            for (const LoraForm& fo : kv.second.forms) b += fo.bytes;
    }
    return b;
}

// ------------------------------------------------------------------------------------ C ABI
int pd_lora_add(pd_engine* e, int32_t adapter, const char* name, const float* up, int32_t up_rows, int32_t rank, const float* down,
                const int64_t* down_shape, int32_t down_ndim) {
    if (!e || !name || !up || !down || !down_shape) { pd_set_error("null argument"); return 1; }
    return e->lora_add(adapter, name, up, up_rows, rank, down, down_shape, down_ndim);
}

int pd_lora_add_ex(pd_engine* e, int32_t adapter, const char* name, const pd_lora_factors* f) {
    if (!e || !name || !f) { pd_set_error("null argument"); return 1; }
    return e->lora_add_ex(adapter, name, *f);
}

int pd_lora_set_scales(pd_engine* e, const float* scales, int32_t n) {
    if (!e) { pd_set_error("null engine"); return 1; }
    return e->lora_set_scales(scales, n);
}

int pd_lora_remove(pd_engine* e, int32_t adapter) {
    if (!e) { pd_set_error("null engine"); return 1; }
    return e->lora_remove(adapter);
}

int pd_read_weights(pd_engine* e, const char* name, float* out) {
    if (!e || !name || !out) { pd_set_error("null argument"); return 1; }
    auto it = e->index.find(name);
    if (it == e->index.end()) { pd_set_error("pd_read_weights: unknown tensor '%s'", name); return 2; }
    return e->read_param(e->params[it->second], out);
}
