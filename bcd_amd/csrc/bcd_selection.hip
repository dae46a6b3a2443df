// bcd_selection.hip -- a frame's similar-patch selection kept beyond the call that decided it (bcd_hip_selection_*, bcd_hip_denoise_layers_keep;
// DESIGN.md section 12).  Similar sets, |S|, the marking, the processed / fallback lists and the count image depend only on the histograms, the sample
// counts and the visiting order; the estimate stage alone reads colours and covariances.  bcd_hip_denoise_layers_keep is bcd_hip_denoise_layers with one
// hook at the end of every scale's chain (selection_store, called by mono_accumulate); bcd_hip_selection_denoise drives layers_follow -- the function the
// frame path runs for the layers beyond the first -- over the kept buffers, with every layer of the call as a follower.
#include "bcd_ctx.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

static_assert(BCD_HIP_SELECTION_MAX_SCALES == MAX_SCALES, "bcd_hip_selection_info has a slot per scale the drivers admit");

#pragma GCC visibility push(hidden)
// one scale: 4 * words + 4 + 1 + 4 + 4 + 4 bytes per pixel (41 at b = 6) and the two list lengths
struct KeptScale {
    DevBuf mask, nsim, state; // as they stand after the estimate
    DevBuf lists;             // W * H items: the full-estimate list, then the fallback list (together they are the processed pixels)
    DevBuf len;               // n_strong, n_weak on the device (the list kernels of other patch radii read them there)
    DevBuf cnt, ns;           // the count image; the sample counts of this pyramid level
    int W = 0, H = 0;
    int n_strong = 0, n_weak = 0;
    int64_t sim_total = 0;
    int path = 0;
};
#pragma GCC visibility pop

struct bcd_hip_selection {
    bcd_hip_ctx *ctx = nullptr;
    bool valid = false;
    int W = 0, H = 0, D = 0, S = 0;
    bcd_hip_params prm;
    KeptScale sc[MAX_SCALES];
};

namespace {

size_t mask_words(int b) { return ((size_t)(2 * b + 1) * (2 * b + 1) + 31) / 32; }

int64_t held_bytes(const bcd_hip_selection *sel)
{
    size_t n = 0;
    for (const KeptScale &k : sel->sc) n += k.mask.bytes + k.nsim.bytes + k.state.bytes + k.lists.bytes + k.len.bytes + k.cnt.bytes + k.ns.bytes;
    return (int64_t)n;
}

// grow-only, before the frame runs: a failure leaves nothing half-filled behind a valid flag
int selection_reserve(bcd_hip_ctx *ctx, bcd_hip_selection *sel, int W, int H, int nb_scales, int b)
{
    for (int s = 0; s < nb_scales; ++s, W /= 2, H /= 2) {
        const size_t npix = (size_t)W * H;
        KeptScale &k = sel->sc[s];
        RCCHK(ensure(ctx, k.mask, npix * mask_words(b) * sizeof(uint32_t)));
        RCCHK(ensure(ctx, k.nsim, npix * sizeof(int32_t)));
        RCCHK(ensure(ctx, k.state, npix));
        RCCHK(ensure(ctx, k.lists, npix * sizeof(int32_t)));
        RCCHK(ensure(ctx, k.len, 2 * sizeof(int32_t)));
        RCCHK(ensure(ctx, k.cnt, npix * sizeof(int32_t)));
        RCCHK(ensure(ctx, k.ns, npix * sizeof(float)));
    }
    return BCD_HIP_OK;
}

// the estimate stage of one scale on the kept selection: per-pixel covariances and cleared sums (the workspace's layer slices), layers_follow for ALL
// layers, which also finalises them with the kept count image and synchronises the scale's stream
int reuse_scale(bcd_hip_ctx *ctx, const bcd_hip_selection *sel, Work &wk, int scale, const LayerView &lv, const float *d_ns)
{
    const KeptScale &k = sel->sc[scale];
    const int W = k.W, H = k.H, w = sel->prm.patch_radius, b = sel->prm.search_radius, L = lv.n;
    const size_t npix = (size_t)W * H;
    RCCHK(ensure(ctx, wk.counters, sizeof(Counters)));
    RCCHK(ensure(ctx, wk.work_q, BCD_WORK_INTS * sizeof(int32_t)));
    RCCHK(ensure(ctx, wk.lay_pixcov, (size_t)L * npix * 6 * sizeof(float)));
    RCCHK(ensure(ctx, wk.lay_sum, (size_t)L * npix * 3 * sizeof(float)));
    touch(wk);
    BcdLayerTable t = {};
    for (int i = 0; i < L; ++i) t.a[i] = lv.cov[i];
    HIPCHK(ctx, bcd_launch_layers_pixel_cov_clear(t, L, d_ns, (int64_t)npix, (float *)wk.lay_pixcov.p, (float *)wk.lay_sum.p, wk.stream));
    const float *pixcov[BCD_MAX_LAYERS];
    float *sum[BCD_MAX_LAYERS];
    for (int i = 0; i < L; ++i) { pixcov[i] = (const float *)wk.lay_pixcov.p + (size_t)i * npix * 6; sum[i] = (float *)wk.lay_sum.p + (size_t)i * npix * 3; }
    const KeptLists kl = { (const int32_t *)k.lists.p, (const int32_t *)k.lists.p + k.n_strong, (const int32_t *)k.len.p, k.n_strong };
    int32_t spectral[BCD_MAX_LAYERS + 1] = { 0 }; // [0]: the (absent) first layer's chain, [1 + i]: layer i
    RCCHK(layers_follow(ctx, wk, lv, (const uint32_t *)k.mask.p, (const int32_t *)k.nsim.p, (const uint8_t *)k.state.p, pixcov, sum, W, H, w, b, sel->prm.min_eigen_value,
                        (const int32_t *)k.cnt.p, spectral, &kl));
    for (int i = 0; i < L; ++i) ctx->layer_spectral[scale][i] = spectral[1 + i];
    bcd_hip_scale_stats &st = ctx->stats[scale];
    memset(&st, 0, sizeof(st)); // (ms_similarity = ms_active = 0: nothing was selected or marked)
    st.width = W; st.height = H;
    st.main_pixels = (int64_t)std::max(0, W - 2 * w) * std::max(0, H - 2 * w);
    st.processed = (int64_t)k.n_strong + k.n_weak; st.fallback = k.n_weak; st.similar_total = k.sim_total;
    st.similarity_path = k.path;
    st.cu_share = ctx->cu_share_pct * (&wk != &ctx->main ? ctx->coarse_share : 100) / 100;
    st.spectral_inverses = wk.h_counters->lists.spectral;
    return BCD_HIP_OK;
}

// one pyramid level of a reuse call from the finer one: the layers' colours and covariances, and -- only when the caller brought sample counts of its own --
// the counts (their sum, as build_level); no histogram level
int reuse_build_level(bcd_hip_ctx *ctx, const LayerView &fine, const LayerView &coarse, const float *ns_fine, float *ns_coarse, int W, int H, hipStream_t st)
{
    if (ns_coarse) HIPCHK(ctx, bcd_launch_downscale(0, ns_fine, W, H, 1, ns_coarse, st));
    return build_level_layers(ctx, fine, coarse, ns_fine, W, H, st);
}

} // namespace

int selection_store(bcd_hip_ctx *ctx, Work &wk, int scale, const float *d_ns, int W, int H, int b, const int32_t *d_count, const bcd_hip_scale_stats &st)
{
    bcd_hip_selection *sel = ctx->keep;
    if (scale < 0 || scale >= MAX_SCALES) return bad(ctx, "selection: scale out of range");
    KeptScale &k = sel->sc[scale];
    const size_t npix = (size_t)W * H;
    const Counters::Lists &h = wk.h_counters->lists;
    if (h.n_strong < 0 || h.n_weak < 0 || (size_t)h.n_strong + (size_t)h.n_weak > npix) return bad(ctx, "selection: the lists exceed the frame");
    if (k.mask.bytes < npix * mask_words(b) * sizeof(uint32_t) || k.lists.bytes < npix * sizeof(int32_t) || k.state.bytes < npix || k.nsim.bytes < npix * sizeof(int32_t) ||
        k.cnt.bytes < npix * sizeof(int32_t) || k.ns.bytes < npix * sizeof(float) || k.len.bytes < 2 * sizeof(int32_t))
        return bad(ctx, "selection: buffers not reserved for this scale");
    k.W = W; k.H = H;
    k.n_strong = h.n_strong; k.n_weak = h.n_weak; k.sim_total = h.sim_total;
    k.path = st.similarity_path;
    hipStream_t s = wk.stream;
    HIPCHK(ctx, hipMemcpyAsync(k.mask.p, wk.mask.p, npix * mask_words(b) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(k.nsim.p, wk.nsim.p, npix * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(k.state.p, wk.state.p, npix, hipMemcpyDeviceToDevice, s));
    if (k.n_strong > 0) HIPCHK(ctx, hipMemcpyAsync(k.lists.p, wk.strong.p, (size_t)k.n_strong * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (k.n_weak > 0) HIPCHK(ctx, hipMemcpyAsync((int32_t *)k.lists.p + k.n_strong, wk.weak.p, (size_t)k.n_weak * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(k.len.p, &wk.d_counters()->lists.n_strong, 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(k.cnt.p, d_count, npix * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(k.ns.p, d_ns, npix * sizeof(float), hipMemcpyDeviceToDevice, s));
    return BCD_HIP_OK;
}

namespace {
// the end of a call that kept its selection: the copies went to the stream of each scale's workspace, a reuse call may drive the scales on other streams
// (bcd_hip_set_concurrent_scales)
int selection_complete(bcd_hip_ctx *ctx, bcd_hip_selection *sel, int W, int H, int D, int nb_scales, const bcd_hip_params *prm)
{
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
    for (int s = 1; s < nb_scales; ++s)
        if (ctx->extra[s].initialised) HIPCHK(ctx, hipStreamSynchronize(ctx->extra[s].stream));
    sel->W = W; sel->H = H; sel->D = D; sel->S = nb_scales; sel->prm = *prm;
    sel->valid = true;
    return BCD_HIP_OK;
}
} // namespace

extern "C" {

int bcd_hip_selection_create(bcd_hip_ctx *ctx, bcd_hip_selection **out)
{
    if (!out) return ctx ? bad(ctx, "null selection handle") : BCD_HIP_EINVAL;
    *out = nullptr;
    if (!ctx) return BCD_HIP_EINVAL;
    bcd_hip_selection *sel = new (std::nothrow) bcd_hip_selection();
    if (!sel) { set_err(ctx, "out of host memory"); return BCD_HIP_ENOMEM; }
    sel->ctx = ctx;
    bcd_hip_default_params(&sel->prm);
    *out = sel;
    return BCD_HIP_OK;
}

void bcd_hip_selection_destroy(bcd_hip_selection *sel)
{
    if (!sel) return;
    DeviceGuard guard(sel->ctx);
    (void)hipDeviceSynchronize();
    for (KeptScale &k : sel->sc)
        for (DevBuf *b : { &k.mask, &k.nsim, &k.state, &k.lists, &k.len, &k.cnt, &k.ns })
            if (b->p) (void)hipFree(b->p);
    delete sel;
}

int bcd_hip_denoise_layers_keep(bcd_hip_ctx *ctx, const float *d_ns, const float *d_hist, int W, int H, int D, int nb_scales, const bcd_hip_params *prm,
                                const bcd_hip_layer *layers, int nb_layers, bcd_hip_selection *sel)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!sel) return bad(ctx, "null selection");
    if (sel->ctx != ctx) return bad(ctx, "the selection belongs to another context");
    sel->valid = false; // (whatever it held is replaced, or lost with a call that fails)
    RCCHK(check_layers_call(ctx, d_ns, d_hist, W, H, D, nb_scales, prm, layers, nb_layers));
    {
        DEVICE_GUARD(ctx);
        RCCHK(selection_reserve(ctx, sel, W, H, nb_scales, prm->search_radius));
    }
    ctx->keep = sel;
    const int rc = denoise_layers_checked(ctx, d_ns, d_hist, W, H, D, nb_scales, prm, layers, nb_layers);
    ctx->keep = nullptr;
    RCCHK(rc);
    return selection_complete(ctx, sel, W, H, D, nb_scales, prm);
}

int bcd_hip_denoise_moments(bcd_hip_ctx *ctx, const float *d_ns, int W, int H, int nb_scales, const bcd_hip_params *prm, float var_floor, const bcd_hip_layer *layers,
                            int nb_layers, bcd_hip_selection *sel)
{
    if (!ctx) return BCD_HIP_EINVAL;
    // ---- everything is checked before any device work
    if (!(var_floor >= 0.f) || !std::isfinite(var_floor)) return bad(ctx, "the variance floor must be finite and not negative");
    if (sel && sel->ctx != ctx) return bad(ctx, "the selection belongs to another context");
    if (sel) sel->valid = false; // (as bcd_hip_denoise_layers_keep)
    RCCHK(check_layers_call(ctx, d_ns, nullptr, W, H, 0, nb_scales, prm, layers, nb_layers, true));
    if (sel) {
        DEVICE_GUARD(ctx);
        RCCHK(selection_reserve(ctx, sel, W, H, nb_scales, prm->search_radius));
    }
    ctx->moments.on = true; ctx->moments.var_floor = var_floor;
    ctx->keep = sel;
    const int rc = denoise_layers_checked(ctx, d_ns, nullptr, W, H, 0, nb_scales, prm, layers, nb_layers);
    ctx->keep = nullptr;
    ctx->moments.on = false;
    RCCHK(rc);
    return sel ? selection_complete(ctx, sel, W, H, 0, nb_scales, prm) : BCD_HIP_OK;
}

int bcd_hip_denoise_guided(bcd_hip_ctx *ctx, const float *d_ns, const float *d_hist, int W, int H, int D, int nb_scales, const bcd_hip_params *prm, float var_floor,
                           const bcd_hip_layer *layers, int nb_layers, const bcd_hip_guide *guide, bcd_hip_selection *sel)
{
    if (!ctx) return BCD_HIP_EINVAL;
    const bool moments = d_hist == nullptr;
    if (moments) D = 0;
    // ---- everything is checked before any device work
    if (moments && (!(var_floor >= 0.f) || !std::isfinite(var_floor))) return bad(ctx, "the variance floor must be finite and not negative");
    if (sel && sel->ctx != ctx) return bad(ctx, "the selection belongs to another context");
    if (sel) sel->valid = false; // (as bcd_hip_denoise_layers_keep)
    RCCHK(check_layers_call(ctx, d_ns, d_hist, W, H, D, nb_scales, prm, layers, nb_layers, moments));
    if ((int64_t)W * H >= (1ll << 31) / BCD_HIP_GUIDE_MAX_CHANNELS) return bad(ctx, "image too large for 32-bit DeepImage indices");
    RCCHK(check_guide(ctx, guide, prm->search_radius));
    {
        DEVICE_GUARD(ctx);
        if (sel) RCCHK(selection_reserve(ctx, sel, W, H, nb_scales, prm->search_radius));
        RCCHK(guide_begin(ctx, guide, guide->features, guide->variances, W, H, nb_scales));
    }
    ctx->moments.on = moments; ctx->moments.var_floor = var_floor;
    ctx->keep = sel;
    const int rc = denoise_layers_checked(ctx, d_ns, d_hist, W, H, D, nb_scales, prm, layers, nb_layers);
    ctx->keep = nullptr;
    ctx->moments.on = false;
    guide_end(ctx);
    RCCHK(rc);
    return sel ? selection_complete(ctx, sel, W, H, D, nb_scales, prm) : BCD_HIP_OK;
}

int bcd_hip_selection_denoise(bcd_hip_selection *sel, const float *d_nsamples, const bcd_hip_layer *layers, int nb_layers)
{
    if (!sel) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = sel->ctx;
    // ---- everything is checked before any device work
    if (!sel->valid) return bad(ctx, "the selection holds no frame (bcd_hip_denoise_layers_keep fills it)");
    if (!layers) return bad(ctx, "null layer list");
    if (nb_layers < 1 || nb_layers > BCD_HIP_MAX_LAYERS) return bad(ctx, "the number of layers must be between 1 and 16 (BCD_HIP_MAX_LAYERS)");
    for (int k = 0; k < nb_layers; ++k)
        if (!layers[k].d_colors || !layers[k].d_covariances || !layers[k].d_out) return bad(ctx, "null image pointer in a layer");
    const int W = sel->W, H = sel->H, S = sel->S, L = nb_layers;
    {
        const size_t npix = (size_t)W * H, f = sizeof(float);
        for (int k = 0; k < L; ++k) {
            const float *o = layers[k].d_out;
            if (d_nsamples && bytes_overlap(o, npix * 3 * f, d_nsamples, npix * f)) return bad(ctx, "a layer's output overlaps the sample counts");
            for (int j = 0; j < L; ++j) {
                if (bytes_overlap(o, npix * 3 * f, layers[j].d_colors, npix * 3 * f) || bytes_overlap(o, npix * 3 * f, layers[j].d_covariances, npix * 6 * f))
                    return bad(ctx, "a layer's output overlaps an input image");
                if (j != k && bytes_overlap(o, npix * 3 * f, layers[j].d_out, npix * 3 * f)) return bad(ctx, "two layers share (part of) an output image");
            }
        }
    }
    DEVICE_GUARD(ctx);
    // ---- the layers and the sample counts at every pyramid level (level 0: the caller's; the kept counts have their levels already)
    std::vector<LayerView> lvs(S);
    const float *ns[MAX_SCALES];
    float *ns_built[MAX_SCALES] = { nullptr };
    lvs[0].n = L;
    for (int k = 0; k < L; ++k) { lvs[0].col[k] = layers[k].d_colors; lvs[0].cov[k] = layers[k].d_covariances; lvs[0].out[k] = layers[k].d_out; }
    ns[0] = d_nsamples ? d_nsamples : (const float *)sel->sc[0].ns.p;
    for (int s = 1; s < S; ++s) {
        const size_t np = (size_t)sel->sc[s].W * sel->sc[s].H;
        RCCHK(ensure(ctx, ctx->lay_pyr[s][0], (size_t)L * np * 3 * sizeof(float)));
        RCCHK(ensure(ctx, ctx->lay_pyr[s][1], (size_t)L * np * 6 * sizeof(float)));
        RCCHK(ensure(ctx, ctx->lay_pyr[s][2], (size_t)L * np * 3 * sizeof(float)));
        lvs[s].n = L;
        for (int k = 0; k < L; ++k) {
            lvs[s].col[k] = (const float *)ctx->lay_pyr[s][0].p + k * np * 3;
            lvs[s].cov[k] = (const float *)ctx->lay_pyr[s][1].p + k * np * 6;
            lvs[s].out[k] = (float *)ctx->lay_pyr[s][2].p + k * np * 3;
        }
        if (d_nsamples) {
            RCCHK(ensure(ctx, ctx->pyr[s][1], np * sizeof(float)));
            ns_built[s] = (float *)ctx->pyr[s][1].p;
            ns[s] = ns_built[s];
        } else ns[s] = (const float *)sel->sc[s].ns.p;
    }
    memset(ctx->layer_spectral, 0, sizeof(ctx->layer_spectral));
    ctx->layer_count = 0;
    if (S > 1 && ctx->concurrent_scales) {
        // as denoise_impl: one stream + host thread + workspace per scale, level s built on its own stream once level s - 1 is complete, the merge into
        // scale s once scale s + 1 is done.  The coarse scales' share of the CU slots is read, not steered.
        HIPCHK(ctx, hipEventRecord(ctx->ev_pyramid, ctx->stream)); // the caller's inputs are ready
        int rcs[MAX_SCALES];
        std::thread threads[MAX_SCALES];
        std::atomic<int> built[MAX_SCALES], done[MAX_SCALES]; // 0 = pending, 1 = event recorded, -1 = failed
        for (int s = 0; s < MAX_SCALES; ++s) { built[s].store(0); done[s].store(0); }
        for (int s = 1; s < S; ++s) RCCHK(work_init(ctx, ctx->extra[s], nullptr));
        auto await = [](std::atomic<int> &f) { int v; while ((v = f.load()) == 0) std::this_thread::yield(); return v; };
        for (int s = S - 1; s >= 0; --s) {
            Work *w = s == 0 ? &ctx->main : &ctx->extra[s];
            rcs[s] = BCD_HIP_OK;
            auto job = [&, s, w]() {
                int rc = BCD_HIP_OK;
                bool built_set = s == 0, done_set = s == 0;
                do {
                    if (hipSetDevice(ctx->device) != hipSuccess) { rc = BCD_HIP_EDEVICE; break; }
                    if (s != 0) {
                        if (hipStreamWaitEvent(w->stream, ctx->ev_pyramid, 0) != hipSuccess) { rc = BCD_HIP_EDEVICE; break; }
                        if (s >= 2) {
                            if (await(built[s - 1]) < 0) { rc = BCD_HIP_EDEVICE; break; }
                            if (hipStreamWaitEvent(w->stream, ctx->extra[s - 1].ev_built, 0) != hipSuccess) { rc = BCD_HIP_EDEVICE; break; }
                        }
                        rc = reuse_build_level(ctx, lvs[s - 1], lvs[s], ns[s - 1], ns_built[s], sel->sc[s - 1].W, sel->sc[s - 1].H, w->stream);
                        if (rc != BCD_HIP_OK) break;
                        if (hipEventRecord(w->ev_built, w->stream) != hipSuccess) { rc = BCD_HIP_EDEVICE; break; }
                        built[s].store(1); built_set = true;
                    }
                    rc = reuse_scale(ctx, sel, *w, s, lvs[s], ns[s]);
                    if (rc != BCD_HIP_OK) break;
                    if (s < S - 1) {
                        if (await(done[s + 1]) < 0) { rc = BCD_HIP_EDEVICE; break; }
                        if (hipStreamWaitEvent(w->stream, ctx->extra[s + 1].ev_done, 0) != hipSuccess) { rc = BCD_HIP_EDEVICE; break; }
                        rc = merge_layers_on(ctx, *w, w->lay_tmp_lo, lvs[s], sel->sc[s].W, sel->sc[s].H, lvs[s + 1]);
                        if (rc != BCD_HIP_OK) break;
                    }
                    if (s != 0) {
                        if (hipEventRecord(w->ev_done, w->stream) != hipSuccess) { rc = BCD_HIP_EDEVICE; break; }
                        done[s].store(1); done_set = true;
                    }
                } while (false);
                if (!built_set) built[s].store(-1); // never leave a waiter spinning
                if (!done_set) done[s].store(-1);
                rcs[s] = rc;
            };
            if (s == 0) job(); else threads[s] = std::thread(job);
        }
        for (int s = 1; s < S; ++s) threads[s].join();
        for (int s = 0; s < S; ++s) RCCHK(rcs[s]);
    } else {
        for (int s = 1; s < S; ++s)
            RCCHK(reuse_build_level(ctx, lvs[s - 1], lvs[s], ns[s - 1], ns_built[s], sel->sc[s - 1].W, sel->sc[s - 1].H, ctx->stream));
        for (int s = S - 1; s >= 0; --s) { // coarse to fine, one after the other
            RCCHK(reuse_scale(ctx, sel, ctx->main, s, lvs[s], ns[s]));
            if (s < S - 1) RCCHK(merge_layers_on(ctx, ctx->main, ctx->main.lay_tmp_lo, lvs[s], sel->sc[s].W, sel->sc[s].H, lvs[s + 1]));
        }
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream)); // (the last merge)
    ctx->layer_count = L;
    return BCD_HIP_OK;
}

int bcd_hip_selection_info(const bcd_hip_selection *sel, struct bcd_hip_selection_info *out)
{
    if (!sel || !out) return BCD_HIP_EINVAL;
    memset(out, 0, sizeof(*out));
    out->valid = sel->valid ? 1 : 0;
    out->device_bytes = held_bytes(sel);
    out->params = sel->prm;
    if (!sel->valid) return BCD_HIP_OK;
    out->W = sel->W; out->H = sel->H; out->D = sel->D; out->nb_scales = sel->S;
    for (int s = 0; s < sel->S; ++s) {
        const KeptScale &k = sel->sc[s];
        bcd_hip_selection_scale &o = out->scale[s];
        o.width = k.W; o.height = k.H;
        o.processed = (int64_t)k.n_strong + k.n_weak; o.fallback = k.n_weak; o.similar_total = k.sim_total;
        o.similarity_path = k.path;
    }
    return BCD_HIP_OK;
}

int bcd_hip_selection_read(bcd_hip_selection *sel, int scale, uint32_t *d_mask, int32_t *d_nsim, uint8_t *d_state, int32_t *d_count)
{
    if (!sel) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = sel->ctx;
    if (!sel->valid) return bad(ctx, "the selection holds no frame (bcd_hip_denoise_layers_keep fills it)");
    if (scale < 0 || scale >= sel->S) return bad(ctx, "selection: scale out of range");
    DEVICE_GUARD(ctx);
    const KeptScale &k = sel->sc[scale];
    const size_t npix = (size_t)k.W * k.H;
    hipStream_t s = ctx->stream;
    if (d_mask) HIPCHK(ctx, hipMemcpyAsync(d_mask, k.mask.p, npix * mask_words(sel->prm.search_radius) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    if (d_nsim) HIPCHK(ctx, hipMemcpyAsync(d_nsim, k.nsim.p, npix * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (d_state) HIPCHK(ctx, hipMemcpyAsync(d_state, k.state.p, npix, hipMemcpyDeviceToDevice, s));
    if (d_count) HIPCHK(ctx, hipMemcpyAsync(d_count, k.cnt.p, npix * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return BCD_HIP_OK;
}

} // extern "C"
