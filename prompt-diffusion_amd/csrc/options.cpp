// pdengine: options, stats and the per-launch profile behind the C ABI.  The options are the rows of kOptions (options.h); nothing
// here knows a key by name except "verbose" (which leaves the captured graphs alone) and "profile" (a command, not a stored knob).
#include <cstdio>
#include <cstring>

#include "engine.h"

static const OptionRow* find_option(const char* key) {
    for (const OptionRow& r : kOptions)
        if (!strcmp(key, r.key)) return &r;
    for (const OptionRow& r : kSwitches)
        if (!strcmp(key, r.key)) return &r;
    return nullptr;
}

// option "profile": brackets on or off, records dropped, and the event overhead calibrated
static void set_profiling(pd_engine* e, bool on) {
    (void)hipStreamSynchronize(e->stream);
    e->profiling = on;
    e->prof.clear();
    e->ev_used = 0;
    if (!e->profiling) return;
    // an event pair around a kernel reads the kernel PLUS the marker packets between them: calibrate that on back-to-back event
    // pairs with NOTHING between them and take it off every bracket.  (Round 3 calibrated on a pair around an empty launch and
    // thereby subtracted that launch's own latency too: the per-launch averages came out 8 % under the kernel trace.)
    const int n = 64;
    std::vector<hipEvent_t> ev(2 * n);
    for (auto& x : ev) x = e->next_event();
    for (int i = 0; i < n; ++i) {
        (void)hipEventRecord(ev[2 * i], e->stream);
        (void)hipEventRecord(ev[2 * i + 1], e->stream);
    }
    (void)hipStreamSynchronize(e->stream);
    double tot = 0.0;
    int cnt = 0;
    for (int i = n / 2; i < n; ++i) {   // second half: warmed up
        float t = 0.f;
        if (ev[2 * i] && ev[2 * i + 1] && hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]) == hipSuccess) { tot += t; ++cnt; }
    }
    e->prof_overhead_ms = cnt ? (float)(tot / cnt) : 0.f;
    e->ev_used = 0;
}

extern "C" {

int pd_set_option(pd_engine* e, const char* key, int64_t value) {
    if (!e || !key) { pd_set_error("null argument"); return 1; }
    if (!strcmp(key, "verbose")) { e->opt.verbose = (int)value; return 0; }
    e->clear_graphs();   // every other knob changes what a step launches
    const OptionRow* r = find_option(key);
    if (!r) { pd_set_error("unknown option '%s'", key); return 1; }
    for (const OptionRow& sw : kSwitches)      // (a session's workspace was sized for the evaluation its switches chose)
        if (r == &sw && e->ses.active) { pd_set_error("option '%s': end the sampling session first", key); return 1; }
    if (r->accepts && !r->accepts(value)) { pd_set_error("%s", r->range_error); return 1; }
    if (r->kind == OPT_COMMAND) { set_profiling(e, value != 0); return 0; }
    e->opt.*r->member = r->kind == OPT_BOOL ? value != 0 : r->kind == OPT_TRI ? (value < 0 ? -1 : value != 0) : (int)value;
    if (r->effect == OPT_FX_LN) e->ln_dirty = true;
    if (r->effect == OPT_FX_SD3_FP8) e->sd3_fp8_dirty = true;
    return 0;
}

int pd_get_option(pd_engine* e, const char* key, int64_t* value) {
    if (!e || !key || !value) { pd_set_error("null argument"); return 1; }
    const OptionRow* r = find_option(key);
    if (!r) { pd_set_error("unknown option '%s'", key); return 1; }
    *value = r->kind == OPT_COMMAND ? (e->profiling ? 1 : 0) : (int64_t)(e->opt.*r->member);
    return 0;
}

int pd_option_info(int32_t index, const char** key, int64_t* default_value) {
    if (index < 0 || index >= (int32_t)(sizeof(kOptions) / sizeof(kOptions[0]))) return 1;
    if (key) *key = kOptions[index].key;
    if (default_value) *default_value = kOptions[index].def;
    return 0;
}

int64_t pd_get_stat(pd_engine* e, const char* key) {
    if (!e || !key) return -1;
    if (!strcmp(key, "ncu")) return (int64_t)e->ncu;   // compute units the chip-fill rules are scaled to (ChipFill)
    if (!strcmp(key, "graph_captures")) return (int64_t)e->graph_captures;
    if (!strcmp(key, "graph_replays")) return (int64_t)e->graph_replays;
    if (!strcmp(key, "workspace_bytes")) return (int64_t)e->arena.cap;
    if (!strcmp(key, "side_workspace_bytes")) return (int64_t)e->arena2.cap;   // what the first stage / HED / text encoders run in (side_call)
    if (!strcmp(key, "weight_bytes")) return (int64_t)e->weight_bytes;
    if (!strcmp(key, "launches")) return (int64_t)e->launches;
    if (!strcmp(key, "ip_launches")) return (int64_t)e->ip_launches;   // of which: IP-Adapter's image term (ip_attention.hip)
    if (!strcmp(key, "pag_launches")) return (int64_t)e->pag_launches;   // of which: made for the perturbed branch of pd_set_pag (engine.h)
    if (!strcmp(key, "pag_fork_block")) return (int64_t)e->pag_fork_block;   // block where the last evaluation forked that branch off; -1: none
    if (!strcmp(key, "image_allocs")) return (int64_t)e->image_allocs;   // allocations of pd_image_load / pd_image_store / pd_canny so far
    if (!strcmp(key, "canny_sweeps")) return (int64_t)e->canny_sweeps;   // hysteresis launches of the last pd_canny / pd_op_canny_hysteresis
    if (!strcmp(key, "gn_from_slabs")) return (int64_t)e->gn_from_slabs;
    if (!strcmp(key, "vae_tiles")) return (int64_t)e->vae_tiles_run;   // tiles run by tiled VAE calls (pd_vae_set_tiling)
    if (!strcmp(key, "vae_flash_launches")) return (int64_t)e->vae_flash_launches;   // of which: vae_attention.hip
    if (!strcmp(key, "ups_fold_launches")) return (int64_t)e->ups_fold_launches;   // of which: conv_upfold.hip's four-phase upsample conv
    if (!strcmp(key, "ring_launches")) return (int64_t)e->ring_launches;   // of which: gemm_ring.hip's persistent ring kernel
    if (!strcmp(key, "gn_kernel")) {   // which kernel the last pd_engine::groupnorm launch took
        static_assert(GN_KIND_TWO_PASS == PD_GN_TWO_PASS && GN_KIND_LDS_SLAB == PD_GN_LDS_SLAB && GN_KIND_REGISTER == PD_GN_REGISTER, "pdengine.h");
        return (int64_t)e->gn_kernel;
    }
    if (!strcmp(key, "attn_kernel")) {   // which kernel family the last pd_engine::attention launch took
        static_assert(ATTN_KIND_GENERIC == PD_ATTN_GENERIC && ATTN_KIND_PIPELINED == PD_ATTN_PIPELINED, "pdengine.h");
        return (int64_t)e->attn_kernel;
    }
    if (!strcmp(key, "gemm_family")) {   // which kernel family the last pd_engine::gemm launch took
        static_assert(GEMM_GEMV == PD_GEMM_GEMV && GEMM_PATCH1 == PD_GEMM_PATCH1 && GEMM_PATCH2 == PD_GEMM_PATCH2 && GEMM_PATCH4 == PD_GEMM_PATCH4 &&
                      GEMM_RING == PD_GEMM_RING && GEMM_IGEMM == PD_GEMM_IGEMM && GEMM_UPFOLD == PD_GEMM_UPFOLD, "pdengine.h");
        return (int64_t)e->gemm_family;
    }
    if (!strcmp(key, "gemm_tile")) return (int64_t)e->gemm_tile;       // the tile of the instantiation that launch took
    if (!strcmp(key, "gemm_ring_tile")) return (int64_t)e->gemm_ring_tile;   // the ring kernel's tile (2 / 3: ping-pong), -1: not a ring launch
    if (!strcmp(key, "gemm_splitk")) return (int64_t)e->gemm_splitk;   // ... and its K / channel-chunk slices
    if (!strcmp(key, "steps")) return (int64_t)e->ses.S;
    if (!strcmp(key, "cfg_shared")) return (int64_t)((e->ses.share_u ? 1 : 0) | (e->ses.share_c ? 2 : 0) | (e->ses.cn_cond_only ? 4 : 0));
    if (!strcmp(key, "lora_base_bytes")) return (int64_t)e->lora_bytes(true);   // base copies W0 of the adapted parameters
    if (!strcmp(key, "lora_bytes")) return (int64_t)e->lora_bytes(false);        // ... plus the adapters' factors
    if (!strcmp(key, "lora_targets")) return (int64_t)e->lora.size();
    if (!strcmp(key, "event_overhead_ns")) return (int64_t)(e->prof_overhead_ms * 1e6f);
    return -1;
}

// Per-launch HIP-event timing collected while option "profile" is on.  klass: 0 igemm conv3x3,
// 1 igemm conv1x1 / linear, 2 attention, 3 conv3x3 LDS-patch kernel, 4 st_front / st_tail, 5 / 6 / 7 the Canny kernels, -1 all.
int pd_profile_read(pd_engine* e, int32_t klass, double* total_ms, int64_t* n_launches, double* flops) {
    if (!e) { pd_set_error("null engine"); return 1; }
    HIP_OK(hipStreamSynchronize(e->stream));
    if (e->stream2) HIP_OK(hipStreamSynchronize(e->stream2));
    double ms = 0.0, fl = 0.0;
    int64_t n = 0;
    for (auto& r : e->prof) {
        if (klass >= 0 && r.klass != klass) continue;
        float t = 0.f;
        if (r.a && r.b && hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) {
            t -= e->prof_overhead_ms;            // the empty-bracket time (see option "profile")
            ms += t > 0.f ? t : 0.f;
            fl += r.flops;
            ++n;
        }
    }
    if (total_ms) *total_ms = ms;
    if (n_launches) *n_launches = n;
    if (flops) *flops = fl;
    return 0;
}

// Debug aid: one CSV row per profiled launch (klass, M, N, K, taps-code, ms, flops).
int pd_profile_dump(pd_engine* e, const char* path) {
    if (!e || !path) { pd_set_error("null argument"); return 1; }
    HIP_OK(hipStreamSynchronize(e->stream));
    if (e->stream2) HIP_OK(hipStreamSynchronize(e->stream2));
    FILE* f = fopen(path, "w");
    if (!f) { pd_set_error("cannot open %s", path); return 1; }
    fprintf(f, "klass,M,N,K,taps,ms,flops\n");
    for (auto& r : e->prof) {
        float t = 0.f;
        if (r.a && r.b && hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) {
            t -= e->prof_overhead_ms;
            fprintf(f, "%d,%d,%d,%d,%d,%.6f,%.0f\n", r.klass, r.M, r.N, r.K, r.taps, t > 0.f ? t : 0.f, r.flops);
        }
    }
    fclose(f);
    return 0;
}

}  // extern "C"
