// bcd_temporal_layers.hip -- the colour layers of a frame denoised with similar patches from its neighbour frames ("Layers"):
// bcd_hip_denoise_temporal_layers[_host] and the stage entry point bcd_hip_bayes_accumulate_temporal_layers.  layers_run builds the pyramids
// (temporal_build_level) and fills the table of the scale stage every call with neighbour frames runs (temporal_scale; bcd_temporal.hip).  The selection of a
// scale -- the in-frame set, the cross sets, the total |S|, the marking, the lists -- reads sample counts and histograms only and is computed once
// (temporal_select, temporal_lists); the estimate stage (bayes_temporal_layers, here) runs per layer: one launch of k_bayes_weak_temporal_layers serves the fallback
// pixels of every layer on the side stream, the chain of full estimates (temporal_full_chain: k_prepare27t, then the unchanged solver and finish kernels) runs
// once per layer over the same lists, records and work queues.  The count image is filled once: by the first group of the fallback kernel and by the first
// layer's finish kernels.
// Every buffer of the call lives in ctx->temporal (grow-only): the workspace's lay_* slices, which bcd_hip_denoise_layers owns, are not touched.
// bcd_hip_denoise_temporal_layers_motion[_host] and bcd_hip_warp_layers (section 16, "Motion") are layers_run with motion fields: a neighbour with a field is
// warped (temporal_warp_neighbour, with its further layers) before its pyramid is built, its cross masks pass the gate at every scale.
// bcd_hip_denoise_temporal_guided[_host] (section 16, "Features") are layers_run / layers_host_run with the guide mode of temporal_select switched on by
// temporal_guide_begin (bcd_temporal.hip): the feature pyramids of every frame, the warped features of a neighbour with a field.
// bcd_hip_denoise_temporal_moments[_host] (section 16, "Moments") are the same drivers with ctx->moments set: no histogram image is read, uploaded, warped or
// reduced, temporal_select selects from layer 0's colours and per-pixel covariances, and a single layer takes the layered path too.
#include "bcd_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

constexpr int ML = BCD_MAX_LAYERS;

// the part of bayes_temporal_layers behind the fork: the wait for the list lengths, then one chain of full estimates per layer -- records and work queues are
// reused, the redo counter runs on and its total is copied out behind each layer.  The side stream is NOT joined here.
int layer_chains(bcd_hip_ctx *ctx, Work &wk, const LayerFrames &lf, int W, int H, int b, float min_eig, float *const *d_sum, int32_t *d_count, int cus)
{
    Counters *h = wk.h_counters;
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    for (int k = 0; k < lf.L; ++k) {
        BcdFrameTable t = {};
        t.n = lf.nf;
        for (int f = 0; f < lf.nf; ++f) { t.col[f] = lf.col[f][k]; t.pixcov[f] = lf.pixcov[f][k]; t.mask[f] = lf.mask[f]; }
        RCCHK(temporal_full_chain(ctx, wk, t, d_sum[k], k == 0 ? d_count : nullptr, h->lists.n_strong, cus, W, H, b, min_eig));
        HIPCHK(ctx, hipMemcpyAsync(&h->layer_redo_total[k], &wk.d_counters()->lists.spectral, sizeof(int32_t), hipMemcpyDeviceToHost, wk.stream)); // (running total: the layers so far)
    }
    return BCD_HIP_OK;
}

} // namespace

// bayes_temporal (bcd_temporal.hip) for L layers on one selection: the lists once, the layered fallback kernel on the side stream, per layer one chain of full
// estimates on that layer's images of every frame, the in-frame masks and its sum image.  d_count goes to the fallback kernel and to the first layer's chain
// only.  redo[k]: the items of layer k that took the redo list; their sum is left in wk.h_counters->lists.spectral beside the list lengths and the sum of |S|.
// Synchronises the stream at its end.  Whatever fails behind the fork, nothing is left running on the side stream when the call returns: the accumulators
// may be the caller's.
int bayes_temporal_layers(bcd_hip_ctx *ctx, Work &wk, const LayerFrames &lf, const int32_t *d_nsim_total, const uint8_t *d_state, int W, int H, int b, float min_eig,
                          float *const *d_sum, int32_t *d_count, int32_t *redo)
{
    const int L = lf.L;
    TemporalLists ls;
    RCCHK(temporal_lists(ctx, wk, d_nsim_total, d_state, (int64_t)W * H, &ls));
    Counters::Lists *d_c = &wk.d_counters()->lists, *h_c = &wk.h_counters->lists;
    Counters *h = wk.h_counters;
    // ---- the fallback pixels of every layer: one launch on the side stream, behind the lists
    BcdFrameLayerTable t = {};
    t.n = lf.nf; t.layers = L;
    for (int f = 0; f < lf.nf; ++f) {
        t.mask[f] = lf.mask[f];
        for (int k = 0; k < L; ++k) t.col[f][k] = lf.col[f][k];
    }
    for (int k = 0; k < L; ++k) t.sum[k] = d_sum[k];
    RCCHK(fork_aux(ctx, wk));
    int rc = BCD_HIP_OK;
    {
        const hipError_t e = bcd_launch_bayes_weak_temporal_layers(t, (const int32_t *)wk.weak.p, &d_c->n_weak, ls.weak_grid, W, b, d_count, wk.aux);
        if (e != hipSuccess) { set_err(ctx, std::string("bcd_launch_bayes_weak_temporal_layers: ") + hipGetErrorString(e)); rc = BCD_HIP_EDEVICE; }
    }
    // ---- the full estimates on the workspace's own stream, then the join
    if (rc == BCD_HIP_OK) rc = layer_chains(ctx, wk, lf, W, H, b, min_eig, d_sum, d_count, ls.cus);
    if (rc != BCD_HIP_OK) {
        (void)hipStreamSynchronize(wk.aux); // (the fallback kernel adds into the accumulators: it ends before the error is reported)
        (void)hipStreamSynchronize(wk.stream);
        return rc;
    }
    HIPCHK(ctx, hipEventRecord(wk.ev_join, wk.aux));
    HIPCHK(ctx, hipStreamWaitEvent(wk.stream, wk.ev_join, 0));
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    for (int k = 0; k < L; ++k) redo[k] = h->layer_redo_total[k] - (k == 0 ? 0 : h->layer_redo_total[k - 1]);
    h_c->spectral = h->layer_redo_total[L - 1]; // the scale's figure: the sum over the layers
    return BCD_HIP_OK;
}

namespace {

// the refusals of the two frame calls, before any device work
// (no_hist: a call of the moment selection -- there are no histogram images, `hist`, D and the neighbours' d_histograms are not looked at)
int check_call(bcd_hip_ctx *ctx, const float *ns, const float *hist, const bcd_hip_frame_layers *nb, int n, int W, int H, int D, int nb_scales, const bcd_hip_params *prm,
               const bcd_hip_layer *layers, int L, bool no_hist = false)
{
    if (n < 0 || n > BCD_HIP_MAX_NEIGHBOURS) return bad(ctx, "the number of neighbour frames must be between 0 and 4 (BCD_HIP_MAX_NEIGHBOURS)");
    RCCHK(check_layers_call(ctx, ns, hist, W, H, D, nb_scales, prm, layers, L, no_hist)); // (null images, the number of layers, the parameters, the scales, the frame's own overlaps)
    if (n > 0 && !nb) return bad(ctx, "null neighbour list");
    for (int f = 0; f < n; ++f) {
        if (!nb[f].d_nsamples || (!nb[f].d_histograms && !no_hist)) return bad(ctx, "null image pointer in a neighbour frame");
        if (!nb[f].layers) return bad(ctx, "null layer list in a neighbour frame");
        if (nb[f].reserved) return bad(ctx, "the reserved pointer of a neighbour frame must be NULL");
        for (int k = 0; k < L; ++k)
            if (!nb[f].layers[k].d_colors || !nb[f].layers[k].d_covariances) return bad(ctx, "null image pointer in a layer of a neighbour frame");
    }
    RCCHK(check_temporal_geometry(ctx, W, H, nb_scales, prm, n > 0, nullptr)); // (check_layers_call has passed the scales: what can fail here is the radii)
    const size_t npix = (size_t)W * H, no = npix * 3 * sizeof(float);
    for (int k = 0; k < L; ++k)
        for (int f = 0; f < n; ++f)
            for (int j = 0; j < L; ++j) // (the neighbour's sample counts and histograms are looked at with each of its layers)
                if (overlaps_frame_images(layers[k].d_out, no, nb[f].layers[j].d_colors, nb[f].d_nsamples, no_hist ? nullptr : nb[f].d_histograms,
                                          nb[f].layers[j].d_covariances, npix, D))
                    return bad(ctx, "a layer's output overlaps an image of a neighbour frame");
    return BCD_HIP_OK;
}

} // namespace

static int guided_host_run(bcd_hip_ctx *ctx, const float *h_ns, const float *h_hist, const bcd_hip_frame_layers *neighbours, int nb_neighbours, const float *const *h_motion,
                           int W, int H, int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer *layers, int nb_layers, const bcd_hip_guide *guide,
                           const bcd_hip_guide_images *neighbour_guides);

extern "C" {

int bcd_hip_bayes_accumulate_temporal_layers(bcd_hip_ctx *ctx, const bcd_hip_stage_frame_layers *frames, int nb_frames, int nb_layers, const int32_t *d_nsim_total,
                                             const uint8_t *d_state, int W, int H, int w, int b, float min_eig, float *const *d_sum, int32_t *d_count, int32_t *h_redo)
{
    if (!ctx) return BCD_HIP_EINVAL;
    // ---- everything is checked before any device work
    if (!frames) return bad(ctx, "null frame list");
    if (nb_frames < 1 || nb_frames > BCD_HIP_MAX_NEIGHBOURS + 1) return bad(ctx, "the number of frames must be between 1 and 5 (the frame and up to BCD_HIP_MAX_NEIGHBOURS neighbours)");
    if (nb_layers < 1 || nb_layers > BCD_HIP_MAX_LAYERS) return bad(ctx, "the number of layers must be between 1 and 16 (BCD_HIP_MAX_LAYERS)");
    if (!d_nsim_total || !d_state || !d_sum || !d_count || !h_redo) return bad(ctx, "null image pointer");
    for (int k = 0; k < nb_layers; ++k) if (!d_sum[k]) return bad(ctx, "null sum image of a layer");
    for (int f = 0; f < nb_frames; ++f) {
        if (!frames[f].d_colors || !frames[f].d_pixel_cov || !frames[f].d_mask) return bad(ctx, "null image pointer in a frame");
        for (int k = 0; k < nb_layers; ++k) if (!frames[f].d_colors[k] || !frames[f].d_pixel_cov[k]) return bad(ctx, "null image pointer in a layer of a frame");
    }
    bcd_hip_params p; bcd_hip_default_params(&p); p.patch_radius = w; p.search_radius = b;
    RCCHK(check_params(ctx, W, H, 1, &p));
    if (w != 1 || b != 6) { set_err(ctx, "the estimate over several frames supports patch radius 1 and search radius 6"); return BCD_HIP_EUNSUPPORTED; }
    {
        const size_t npix = (size_t)W * H, f4 = sizeof(float), ns = npix * 3 * f4, words = ((size_t)(2 * b + 1) * (2 * b + 1) + 31) / 32;
        if (bytes_overlap(d_count, npix * 4, d_nsim_total, npix * 4) || bytes_overlap(d_count, npix * 4, d_state, npix)) return bad(ctx, "the accumulators overlap each other or the selection");
        for (int k = 0; k < nb_layers; ++k) {
            const void *s = d_sum[k];
            if (bytes_overlap(s, ns, d_count, npix * 4) || bytes_overlap(s, ns, d_nsim_total, npix * 4) || bytes_overlap(s, ns, d_state, npix)) return bad(ctx, "the accumulators overlap each other or the selection");
            for (int j = 0; j < k; ++j) if (bytes_overlap(s, ns, d_sum[j], ns)) return bad(ctx, "two layers share (part of) a sum image");
        }
        for (int f = 0; f < nb_frames; ++f) {
            if (bytes_overlap(d_count, npix * 4, frames[f].d_mask, npix * words * 4)) return bad(ctx, "an accumulator overlaps an input image");
            for (int j = 0; j < nb_layers; ++j) {
                if (bytes_overlap(d_count, npix * 4, frames[f].d_colors[j], ns) || bytes_overlap(d_count, npix * 4, frames[f].d_pixel_cov[j], npix * 6 * f4)) return bad(ctx, "an accumulator overlaps an input image");
                for (int k = 0; k < nb_layers; ++k)
                    if (bytes_overlap(d_sum[k], ns, frames[f].d_colors[j], ns) || bytes_overlap(d_sum[k], ns, frames[f].d_pixel_cov[j], npix * 6 * f4) ||
                        bytes_overlap(d_sum[k], ns, frames[f].d_mask, npix * words * 4))
                        return bad(ctx, "an accumulator overlaps an input image");
            }
        }
    }
    DEVICE_GUARD(ctx);
    LayerFrames lf;
    lf.nf = nb_frames; lf.L = nb_layers;
    for (int f = 0; f < nb_frames; ++f) {
        lf.mask[f] = frames[f].d_mask;
        for (int k = 0; k < nb_layers; ++k) { lf.col[f][k] = frames[f].d_colors[k]; lf.pixcov[f][k] = frames[f].d_pixel_cov[k]; }
    }
    return bayes_temporal_layers(ctx, ctx->main, lf, d_nsim_total, d_state, W, H, b, min_eig, d_sum, d_count, h_redo);
}

// one layer is the frame call (host: of host buffers) on that layer; motion: null, or the list of a motion call
static int single_layer_call(bcd_hip_ctx *ctx, bool host, const float *ns, const float *hist, const bcd_hip_frame_layers *neighbours, int nb_neighbours, int W, int H, int D,
                             int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer &layer, const float *const *motion)
{
    bcd_hip_frame nb[BCD_HIP_MAX_NEIGHBOURS];
    for (int f = 0; f < nb_neighbours; ++f)
        nb[f] = { neighbours[f].layers[0].d_colors, neighbours[f].d_nsamples, neighbours[f].d_histograms, neighbours[f].layers[0].d_covariances, nullptr };
    if (motion)
        RCCHK((host ? bcd_hip_denoise_temporal_motion_host : bcd_hip_denoise_temporal_motion)(ctx, layer.d_colors, ns, hist, layer.d_covariances, nb, nb_neighbours, motion, W,
                                                                                             H, D, nb_scales, prm, layer.d_out));
    else
        RCCHK((host ? bcd_hip_denoise_temporal_host : bcd_hip_denoise_temporal)(ctx, layer.d_colors, ns, hist, layer.d_covariances, nb, nb_neighbours, W, H, D, nb_scales, prm,
                                                                               layer.d_out));
    memset(ctx->layer_spectral, 0, sizeof(ctx->layer_spectral));
    for (int s = 0; s < nb_scales; ++s) ctx->layer_spectral[s][0] = ctx->stats[s].spectral_inverses;
    ctx->layer_count = 1;
    return BCD_HIP_OK;
}

// the checked device call; motion: null, or per neighbour a device motion field or null
static int layers_run(bcd_hip_ctx *ctx, const float *d_ns, const float *d_hist, const bcd_hip_frame_layers *neighbours, int nb_neighbours, int W, int H, int D,
                      int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer *layers, int nb_layers, const float *const *motion)
{
    const bool moments = ctx->moments.on; // ("Moments": no histogram images, D = 0, at least one neighbour; one layer takes the layered path too)
    if (nb_neighbours == 0) return bcd_hip_denoise_layers(ctx, d_ns, d_hist, W, H, D, nb_scales, prm, layers, nb_layers);
    if (nb_layers == 1 && !moments) return single_layer_call(ctx, false, d_ns, d_hist, neighbours, nb_neighbours, W, H, D, nb_scales, prm, layers[0], motion);
    DEVICE_GUARD(ctx);
    const int nf = nb_neighbours + 1, S = nb_scales, L = nb_layers;
    auto &tp = ctx->temporal;
    hipStream_t st = ctx->main.stream;
    memset(ctx->layer_spectral, 0, sizeof(ctx->layer_spectral));
    ctx->layer_count = 0;
    // ---- the pyramids of every frame: sample counts and histograms summed, the layers' colours averaged and their covariances weighted by the frame's counts
    std::vector<TemporalFrame> lv((size_t)S * nf, TemporalFrame());
    LayerView outs[MAX_SCALES]; // (the outputs of every level, for the stage and the merge)
    int ws[MAX_SCALES], hs[MAX_SCALES];
    ws[0] = W; hs[0] = H;
    for (int f = 0; f < nf; ++f) {
        TemporalFrame &l = lv[f];
        l.sel.ns = f ? neighbours[f - 1].d_nsamples : d_ns; l.sel.hist = moments ? nullptr : f ? neighbours[f - 1].d_histograms : d_hist;
        for (int k = 0; k < L; ++k) {
            l.col[k] = f ? neighbours[f - 1].layers[k].d_colors : layers[k].d_colors;
            l.cov[k] = f ? neighbours[f - 1].layers[k].d_covariances : layers[k].d_covariances;
        }
    }
    outs[0].n = L;
    for (int k = 0; k < L; ++k) outs[0].out[k] = layers[k].d_out;
    std::vector<const uint8_t *> valid((size_t)S * nf, nullptr);
    for (int f = 1; motion && f < nf; ++f) {
        if (!motion[f - 1]) continue;
        // the neighbour reprojected into the frame's pixel grid, at full resolution: sample counts, histograms and the first layer by the frame kernel, the further
        // layers by the layered one (it writes the same validity bytes again); the pyramid is built from the warped images
        const size_t npix = (size_t)W * H;
        TemporalFrame &l = lv[f];
        DevBuf(&lw)[2] = tp.lay_warp[f];
        RCCHK(ensure(ctx, lw[0], (size_t)(L - 1) * npix * 3 * sizeof(float)));
        RCCHK(ensure(ctx, lw[1], (size_t)(L - 1) * npix * 6 * sizeof(float)));
        BcdWarpLayerTable t = {};
        for (int k = 1; k < L; ++k) {
            t.col[k - 1] = l.col[k]; t.cov[k - 1] = l.cov[k];
            t.ocol[k - 1] = (float *)lw[0].p + (size_t)(k - 1) * npix * 3; t.ocov[k - 1] = (float *)lw[1].p + (size_t)(k - 1) * npix * 6;
        }
        const float *wp[4];
        RCCHK(temporal_warp_neighbour(ctx, f, nf, l.col[0], l.sel.ns, l.sel.hist, l.cov[0], motion[f - 1], W, H, D, S, L > 1 ? &t : nullptr, L - 1, valid.data(), wp));
        l.col[0] = wp[0]; l.sel.ns = wp[1]; l.sel.hist = moments ? nullptr : wp[2]; l.cov[0] = wp[3]; // ("Moments": D = 0, nothing of a histogram is gathered)
        for (int k = 1; k < L; ++k) { l.col[k] = t.ocol[k - 1]; l.cov[k] = t.ocov[k - 1]; }
    }
    for (int s = 1; s < S; ++s) {
        ws[s] = ws[s - 1] / 2; hs[s] = hs[s - 1] / 2;
        const size_t np = (size_t)ws[s] * hs[s];
        RCCHK(ensure(ctx, tp.lay_out[s], (size_t)L * np * 3 * sizeof(float)));
        outs[s].n = L;
        for (int k = 0; k < L; ++k) outs[s].out[k] = (float *)tp.lay_out[s].p + (size_t)k * np * 3;
        for (int f = 0; f < nf; ++f) {
            DevBuf(&l)[4] = tp.pyr[f][s];
            DevBuf(&ll)[2] = tp.lay_pyr[f][s];
            RCCHK(ensure(ctx, l[1], np * sizeof(float)));
            if (!moments) RCCHK(ensure(ctx, l[2], np * D * sizeof(float)));
            RCCHK(ensure(ctx, ll[0], (size_t)L * np * 3 * sizeof(float)));
            RCCHK(ensure(ctx, ll[1], (size_t)L * np * 6 * sizeof(float)));
            TemporalFrame &coarse = lv[(size_t)s * nf + f];
            coarse.sel.ns = (const float *)l[1].p; coarse.sel.hist = moments ? nullptr : (const float *)l[2].p; // ("Moments": the pyramids have no histogram level)
            for (int k = 0; k < L; ++k) { coarse.col[k] = (const float *)ll[0].p + (size_t)k * np * 3; coarse.cov[k] = (const float *)ll[1].p + (size_t)k * np * 6; }
            RCCHK(temporal_build_level(ctx, lv[(size_t)(s - 1) * nf + f], coarse, L, true, ws[s - 1], hs[s - 1], D, st));
        }
    }
    for (int s = S - 1; s >= 0; --s) { // coarse to fine; the merge is mergeOutputs, one pair of launches for all layers
        const size_t npix = (size_t)ws[s] * hs[s];
        TemporalScale sc;
        sc.nf = nf; sc.L = L; sc.layered = true;
        RCCHK(ensure(ctx, tp.lay_sum, (size_t)L * npix * 3 * sizeof(float)));
        sc.sum = (float *)tp.lay_sum.p;
        for (int k = 0; k < L; ++k) sc.out[k] = outs[s].out[k];
        for (int f = 0; f < nf; ++f) {
            TemporalFrame &fr = sc.fr[f] = lv[(size_t)s * nf + f];
            RCCHK(ensure(ctx, tp.lay_pixcov[f], (size_t)L * npix * 6 * sizeof(float)));
            fr.pixcov = (float *)tp.lay_pixcov[f].p;
            fr.sel.valid = valid[(size_t)s * nf + f]; // (null: the frame is not warped)
            temporal_guide_level(ctx, f, s, &fr.sel);
        }
        RCCHK(temporal_scale(ctx, sc, ws[s], hs[s], D, prm, s));
        if (s < S - 1) RCCHK(merge_layers_on(ctx, ctx->main, tp.lay_tmp_lo, outs[s], ws[s], hs[s], outs[s + 1]));
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    ctx->layer_count = L;
    return BCD_HIP_OK;
}

// the outputs of the layers, for check_motion_list
static void layer_outs(const bcd_hip_layer *layers, int L, float **outs) { for (int k = 0; k < L; ++k) outs[k] = layers[k].d_out; }

int bcd_hip_denoise_temporal_layers(bcd_hip_ctx *ctx, const float *d_ns, const float *d_hist, const bcd_hip_frame_layers *neighbours, int nb_neighbours, int W, int H, int D,
                                    int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer *layers, int nb_layers)
{
    if (!ctx) return BCD_HIP_EINVAL;
    RCCHK(check_call(ctx, d_ns, d_hist, neighbours, nb_neighbours, W, H, D, nb_scales, prm, layers, nb_layers));
    return layers_run(ctx, d_ns, d_hist, neighbours, nb_neighbours, W, H, D, nb_scales, prm, layers, nb_layers, nullptr);
}

int bcd_hip_denoise_temporal_layers_motion(bcd_hip_ctx *ctx, const float *d_ns, const float *d_hist, const bcd_hip_frame_layers *neighbours, int nb_neighbours,
                                           const float *const *d_motion, int W, int H, int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer *layers,
                                           int nb_layers)
{
    if (!ctx) return BCD_HIP_EINVAL;
    RCCHK(check_call(ctx, d_ns, d_hist, neighbours, nb_neighbours, W, H, D, nb_scales, prm, layers, nb_layers));
    float *outs[ML];
    layer_outs(layers, nb_layers, outs);
    RCCHK(check_motion_list(ctx, d_motion, nb_neighbours, W, H, outs, nb_layers));
    return layers_run(ctx, d_ns, d_hist, neighbours, nb_neighbours, W, H, D, nb_scales, prm, layers, nb_layers, any_field(d_motion, nb_neighbours) ? d_motion : nullptr);
}

// the checked host call; h_motion: null, or per neighbour a host motion field or null
static int layers_host_run(bcd_hip_ctx *ctx, const float *h_ns, const float *h_hist, const bcd_hip_frame_layers *neighbours, int nb_neighbours, int W, int H,
                           int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer *layers, int nb_layers, const float *const *h_motion)
{
    const int L = nb_layers;
    if (nb_neighbours == 0) {
        bcd_hip_host_layer hl[BCD_HIP_MAX_LAYERS];
        for (int k = 0; k < L; ++k) hl[k] = { layers[k].d_colors, layers[k].d_covariances, layers[k].d_out };
        return bcd_hip_denoise_layers_host(ctx, h_ns, h_hist, W, H, D, nb_scales, prm, nullptr, hl, L);
    }
    const bool moments = ctx->moments.on; // ("Moments": no histogram image is uploaded)
    if (L == 1 && !moments) return single_layer_call(ctx, true, h_ns, h_hist, neighbours, nb_neighbours, W, H, D, nb_scales, prm, layers[0], h_motion);
    DEVICE_GUARD(ctx);
    auto &tp = ctx->temporal;
    const size_t npix = (size_t)W * H, f4 = sizeof(float), bc = npix * 3 * f4, bv = npix * 6 * f4;
    hipStream_t st = ctx->main.stream;
    bcd_hip_frame_layers dev[BCD_HIP_MAX_NEIGHBOURS + 1];
    std::vector<bcd_hip_frame_layer> dl((size_t)(nb_neighbours + 1) * L);
    for (int f = 0; f <= nb_neighbours; ++f) { // whole uploads, no streaming
        const float *ns = f ? neighbours[f - 1].d_nsamples : h_ns, *hist = f ? neighbours[f - 1].d_histograms : h_hist;
        RCCHK(ensure(ctx, tp.host[f][1], npix * f4));
        if (!moments) RCCHK(ensure(ctx, tp.host[f][2], npix * D * f4));
        RCCHK(ensure(ctx, tp.lay_host[f][0], (size_t)L * bc));
        RCCHK(ensure(ctx, tp.lay_host[f][1], (size_t)L * bv));
        HIPCHK(ctx, hipMemcpyAsync(tp.host[f][1].p, ns, npix * f4, hipMemcpyHostToDevice, st));
        if (!moments) HIPCHK(ctx, hipMemcpyAsync(tp.host[f][2].p, hist, npix * D * f4, hipMemcpyHostToDevice, st));
        for (int k = 0; k < L; ++k) {
            float *dc = (float *)tp.lay_host[f][0].p + (size_t)k * npix * 3, *dv = (float *)tp.lay_host[f][1].p + (size_t)k * npix * 6;
            HIPCHK(ctx, hipMemcpyAsync(dc, f ? neighbours[f - 1].layers[k].d_colors : layers[k].d_colors, bc, hipMemcpyHostToDevice, st));
            HIPCHK(ctx, hipMemcpyAsync(dv, f ? neighbours[f - 1].layers[k].d_covariances : layers[k].d_covariances, bv, hipMemcpyHostToDevice, st));
            dl[(size_t)f * L + k] = { dc, dv };
        }
        dev[f] = { (const float *)tp.host[f][1].p, moments ? nullptr : (const float *)tp.host[f][2].p, &dl[(size_t)f * L], nullptr };
    }
    RCCHK(ensure(ctx, tp.lay_host_out, (size_t)L * bc));
    bcd_hip_layer lay[BCD_HIP_MAX_LAYERS];
    for (int k = 0; k < L; ++k) lay[k] = { dl[k].d_colors, dl[k].d_covariances, (float *)tp.lay_host_out.p + (size_t)k * npix * 3 };
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int f = 0; tp.prefilter > 0.f && f <= nb_neighbours; ++f) { // ("Prefilter": every frame on its own, in its own pixel grid, in place in its uploaded copies)
        float *col[BCD_HIP_MAX_LAYERS], *cov[BCD_HIP_MAX_LAYERS];
        for (int k = 0; k < L; ++k) { col[k] = const_cast<float *>(dl[(size_t)f * L + k].d_colors); cov[k] = const_cast<float *>(dl[(size_t)f * L + k].d_covariances); }
        RCCHK(spike_filter_frame_inplace(ctx, (float *)tp.host[f][1].p, moments ? nullptr : (float *)tp.host[f][2].p, W, H, D, tp.prefilter, col, cov, L, nullptr, nullptr));
    }
    const float *dmv[BCD_HIP_MAX_NEIGHBOURS];
    if (h_motion) RCCHK(temporal_upload_motion(ctx, h_motion, nb_neighbours, W, H, dmv));
    RCCHK(layers_run(ctx, dev[0].d_nsamples, dev[0].d_histograms, dev + 1, nb_neighbours, W, H, D, nb_scales, prm, lay, L, h_motion ? dmv : nullptr));
    for (int k = 0; k < L; ++k) HIPCHK(ctx, hipMemcpyAsync(layers[k].d_out, lay[k].d_out, bc, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return BCD_HIP_OK;
}

int bcd_hip_denoise_temporal_layers_host(bcd_hip_ctx *ctx, const float *h_ns, const float *h_hist, const bcd_hip_frame_layers *neighbours, int nb_neighbours, int W, int H,
                                         int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer *layers, int nb_layers)
{
    if (!ctx) return BCD_HIP_EINVAL;
    RCCHK(check_call(ctx, h_ns, h_hist, neighbours, nb_neighbours, W, H, D, nb_scales, prm, layers, nb_layers));
    return layers_host_run(ctx, h_ns, h_hist, neighbours, nb_neighbours, W, H, D, nb_scales, prm, layers, nb_layers, nullptr);
}

int bcd_hip_denoise_temporal_layers_motion_host(bcd_hip_ctx *ctx, const float *h_ns, const float *h_hist, const bcd_hip_frame_layers *neighbours, int nb_neighbours,
                                                const float *const *h_motion, int W, int H, int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer *layers,
                                                int nb_layers)
{
    if (!ctx) return BCD_HIP_EINVAL;
    RCCHK(check_call(ctx, h_ns, h_hist, neighbours, nb_neighbours, W, H, D, nb_scales, prm, layers, nb_layers));
    float *outs[ML];
    layer_outs(layers, nb_layers, outs);
    RCCHK(check_motion_list(ctx, h_motion, nb_neighbours, W, H, outs, nb_layers));
    return layers_host_run(ctx, h_ns, h_hist, neighbours, nb_neighbours, W, H, D, nb_scales, prm, layers, nb_layers, any_field(h_motion, nb_neighbours) ? h_motion : nullptr);
}

// ---- "Features": the layered motion call with the selection gated by auxiliary feature buffers ----------------------------------
// the refusals of the two guided frame calls with at least one neighbour, before any device work (the pointers are compared as addresses: device or host)
static int check_guided_call(bcd_hip_ctx *ctx, const float *ns, const float *hist, const bcd_hip_frame_layers *neighbours, int n, const float *const *motion, int W, int H,
                             int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer *layers, int L, const bcd_hip_guide *guide,
                             const bcd_hip_guide_images *ng, bool no_hist = false)
{
    RCCHK(check_call(ctx, ns, hist, neighbours, n, W, H, D, nb_scales, prm, layers, L, no_hist));
    float *outs[ML];
    layer_outs(layers, L, outs);
    if (motion) RCCHK(check_motion_list(ctx, motion, n, W, H, outs, L)); // (a NULL list: nothing is warped)
    if ((int64_t)W * H >= (1ll << 31) / BCD_HIP_GUIDE_MAX_CHANNELS) return bad(ctx, "image too large for 32-bit DeepImage indices");
    RCCHK(check_guide(ctx, guide, prm->search_radius));
    if (!ng) return bad(ctx, "null list of the neighbour frames' feature images");
    const bool var = guide->variances != nullptr;
    for (int f = 0; f < n; ++f) {
        if (!ng[f].features) return bad(ctx, "null feature image of a neighbour frame");
        if ((ng[f].variances != nullptr) != var) return bad(ctx, "feature variances must be given for every frame or for none");
    }
    if (bcd_pairdist_guide_cross_band(guide->nb_channels, var, prm->search_radius) < 1) {
        set_err(ctx, "the cross feature distance kernel cannot be launched for this number of channels and search radius (LDS)");
        return BCD_HIP_EUNSUPPORTED;
    }
    const size_t npix = (size_t)W * H, no = npix * 3 * sizeof(float), nfeat = npix * guide->nb_channels * sizeof(float);
    for (int k = 0; k < L; ++k)
        for (int f = 0; f <= n; ++f) {
            const float *feat = f ? ng[f - 1].features : guide->features, *vv = f ? ng[f - 1].variances : guide->variances;
            if (bytes_overlap(outs[k], no, feat, nfeat) || (vv && bytes_overlap(outs[k], no, vv, nfeat))) return bad(ctx, "a layer's output overlaps a feature or variance image");
        }
    return BCD_HIP_OK;
}

int bcd_hip_denoise_temporal_guided(bcd_hip_ctx *ctx, const float *d_ns, const float *d_hist, const bcd_hip_frame_layers *neighbours, int nb_neighbours,
                                    const float *const *d_motion, int W, int H, int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer *layers, int nb_layers,
                                    const bcd_hip_guide *guide, const bcd_hip_guide_images *neighbour_guides)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_hist) return bad(ctx, "the guided temporal call needs histograms: the cross-frame selection from means and covariances is bcd_hip_denoise_temporal_moments");
    if (nb_neighbours == 0) return bcd_hip_denoise_guided(ctx, d_ns, d_hist, W, H, D, nb_scales, prm, 0.f, layers, nb_layers, guide, nullptr);
    RCCHK(check_guided_call(ctx, d_ns, d_hist, neighbours, nb_neighbours, d_motion, W, H, D, nb_scales, prm, layers, nb_layers, guide, neighbour_guides));
    int rc;
    {
        DEVICE_GUARD(ctx);
        rc = temporal_guide_begin(ctx, guide, neighbour_guides, nb_neighbours, d_motion, W, H, nb_scales);
    }
    if (rc == BCD_HIP_OK)
        rc = layers_run(ctx, d_ns, d_hist, neighbours, nb_neighbours, W, H, D, nb_scales, prm, layers, nb_layers, any_field(d_motion, nb_neighbours) ? d_motion : nullptr);
    temporal_guide_end(ctx);
    return rc;
}

// every pointer a host pointer: whole uploads of the feature images (and of the motion fields, which warp them) into ctx->temporal.guide_host, the set-up on
// the device copies, then the layered host call -- its own uploads, the resident call, one download per layer -- with the guide mode on
int bcd_hip_denoise_temporal_guided_host(bcd_hip_ctx *ctx, const float *h_ns, const float *h_hist, const bcd_hip_frame_layers *neighbours, int nb_neighbours,
                                         const float *const *h_motion, int W, int H, int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer *layers,
                                         int nb_layers, const bcd_hip_guide *guide, const bcd_hip_guide_images *neighbour_guides)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!h_hist) return bad(ctx, "the guided temporal call needs histograms: the cross-frame selection from means and covariances is bcd_hip_denoise_temporal_moments");
    if (nb_neighbours == 0) {
        if (!layers) return bad(ctx, "null layer list");
        if (nb_layers < 1 || nb_layers > BCD_HIP_MAX_LAYERS) return bad(ctx, "the number of layers must be between 1 and 16 (BCD_HIP_MAX_LAYERS)");
        bcd_hip_host_layer hl[BCD_HIP_MAX_LAYERS];
        for (int k = 0; k < nb_layers; ++k) hl[k] = { layers[k].d_colors, layers[k].d_covariances, layers[k].d_out };
        return bcd_hip_denoise_guided_host(ctx, h_ns, h_hist, W, H, D, nb_scales, prm, nullptr, 0.f, hl, nb_layers, guide);
    }
    RCCHK(check_guided_call(ctx, h_ns, h_hist, neighbours, nb_neighbours, h_motion, W, H, D, nb_scales, prm, layers, nb_layers, guide, neighbour_guides));
    return guided_host_run(ctx, h_ns, h_hist, neighbours, nb_neighbours, h_motion, W, H, D, nb_scales, prm, layers, nb_layers, guide, neighbour_guides);
}

} // extern "C"

// the checked guided host call with at least one neighbour (h_hist NULL and D = 0: a call of the moment selection, ctx->moments set)
static int guided_host_run(bcd_hip_ctx *ctx, const float *h_ns, const float *h_hist, const bcd_hip_frame_layers *neighbours, int nb_neighbours, const float *const *h_motion,
                           int W, int H, int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer *layers, int nb_layers, const bcd_hip_guide *guide,
                           const bcd_hip_guide_images *neighbour_guides)
{
    const float *const *motion = any_field(h_motion, nb_neighbours) ? h_motion : nullptr;
    int rc;
    {
        DEVICE_GUARD(ctx);
        auto &tp = ctx->temporal;
        hipStream_t st = ctx->main.stream;
        const size_t bytes = (size_t)W * H * guide->nb_channels * sizeof(float);
        const bool var = guide->variances != nullptr;
        bcd_hip_guide dg = *guide;
        bcd_hip_guide_images dn[BCD_HIP_MAX_NEIGHBOURS];
        for (int f = 0; f <= nb_neighbours; ++f) {
            const float *src[2] = { f ? neighbour_guides[f - 1].features : guide->features, f ? neighbour_guides[f - 1].variances : guide->variances };
            for (int k = 0; k < (var ? 2 : 1); ++k) {
                RCCHK(ensure(ctx, tp.guide_host[f][k], bytes));
                HIPCHK(ctx, hipMemcpyAsync(tp.guide_host[f][k].p, src[k], bytes, hipMemcpyHostToDevice, st));
            }
            const float *df = (const float *)tp.guide_host[f][0].p, *dv = var ? (const float *)tp.guide_host[f][1].p : nullptr;
            if (f == 0) { dg.features = df; dg.variances = dv; }
            else dn[f - 1] = { df, dv };
        }
        HIPCHK(ctx, hipStreamSynchronize(st)); // (the sources are pageable host memory of the caller)
        const float *dmv[BCD_HIP_MAX_NEIGHBOURS];
        if (motion) RCCHK(temporal_upload_motion(ctx, motion, nb_neighbours, W, H, dmv));
        rc = temporal_guide_begin(ctx, &dg, dn, nb_neighbours, motion ? dmv : nullptr, W, H, nb_scales);
    }
    if (rc == BCD_HIP_OK) rc = layers_host_run(ctx, h_ns, h_hist, neighbours, nb_neighbours, W, H, D, nb_scales, prm, layers, nb_layers, motion);
    temporal_guide_end(ctx);
    return rc;
}

// ---- "Moments": the layered motion call, optionally feature-gated, with every selection made from means and covariances -------------
// the refusals of the two frame calls with at least one neighbour, before any device work (the pointers are compared as addresses: device or host)
static int check_moments_call(bcd_hip_ctx *ctx, const float *ns, const bcd_hip_frame_layers *neighbours, int n, const float *const *motion, int W, int H, int nb_scales,
                              const bcd_hip_params *prm, const bcd_hip_layer *layers, int L, const bcd_hip_guide *guide, const bcd_hip_guide_images *ng)
{
    if ((guide == nullptr) != (ng == nullptr)) return bad(ctx, "guide and neighbour_guides must both be NULL or both be given");
    if (guide) return check_guided_call(ctx, ns, nullptr, neighbours, n, motion, W, H, 0, nb_scales, prm, layers, L, guide, ng, true);
    RCCHK(check_call(ctx, ns, nullptr, neighbours, n, W, H, 0, nb_scales, prm, layers, L, true));
    float *outs[ML];
    layer_outs(layers, L, outs);
    if (motion) RCCHK(check_motion_list(ctx, motion, n, W, H, outs, L)); // (a NULL list: nothing is warped)
    return BCD_HIP_OK;
}

// what both frame calls refuse ahead of their delegations
static int check_moments_head(bcd_hip_ctx *ctx, int nb_neighbours, float var_floor)
{
    if (!(var_floor >= 0.f) || !std::isfinite(var_floor)) return bad(ctx, "the variance floor must be finite and not negative");
    if (nb_neighbours < 0 || nb_neighbours > BCD_HIP_MAX_NEIGHBOURS) return bad(ctx, "the number of neighbour frames must be between 0 and 4 (BCD_HIP_MAX_NEIGHBOURS)");
    return BCD_HIP_OK;
}

extern "C" {

int bcd_hip_denoise_temporal_moments(bcd_hip_ctx *ctx, const float *d_ns, const bcd_hip_frame_layers *neighbours, int nb_neighbours, const float *const *d_motion, int W,
                                     int H, int nb_scales, const bcd_hip_params *prm, float var_floor, const bcd_hip_layer *layers, int nb_layers,
                                     const bcd_hip_guide *guide, const bcd_hip_guide_images *neighbour_guides)
{
    if (!ctx) return BCD_HIP_EINVAL;
    RCCHK(check_moments_head(ctx, nb_neighbours, var_floor));
    if (nb_neighbours == 0)
        return guide ? bcd_hip_denoise_guided(ctx, d_ns, nullptr, W, H, 0, nb_scales, prm, var_floor, layers, nb_layers, guide, nullptr)
                     : bcd_hip_denoise_moments(ctx, d_ns, W, H, nb_scales, prm, var_floor, layers, nb_layers, nullptr);
    RCCHK(check_moments_call(ctx, d_ns, neighbours, nb_neighbours, d_motion, W, H, nb_scales, prm, layers, nb_layers, guide, neighbour_guides));
    const float *const *motion = any_field(d_motion, nb_neighbours) ? d_motion : nullptr;
    int rc = BCD_HIP_OK;
    if (guide) {
        DEVICE_GUARD(ctx);
        rc = temporal_guide_begin(ctx, guide, neighbour_guides, nb_neighbours, motion, W, H, nb_scales);
    }
    ctx->moments.on = true; ctx->moments.var_floor = var_floor;
    if (rc == BCD_HIP_OK) rc = layers_run(ctx, d_ns, nullptr, neighbours, nb_neighbours, W, H, 0, nb_scales, prm, layers, nb_layers, motion);
    ctx->moments.on = false;
    temporal_guide_end(ctx);
    return rc;
}

int bcd_hip_denoise_temporal_moments_host(bcd_hip_ctx *ctx, const float *h_ns, const bcd_hip_frame_layers *neighbours, int nb_neighbours, const float *const *h_motion, int W,
                                          int H, int nb_scales, const bcd_hip_params *prm, float var_floor, const bcd_hip_layer *layers, int nb_layers,
                                          const bcd_hip_guide *guide, const bcd_hip_guide_images *neighbour_guides)
{
    if (!ctx) return BCD_HIP_EINVAL;
    RCCHK(check_moments_head(ctx, nb_neighbours, var_floor));
    if (nb_neighbours == 0) {
        if (!layers) return bad(ctx, "null layer list");
        if (nb_layers < 1 || nb_layers > BCD_HIP_MAX_LAYERS) return bad(ctx, "the number of layers must be between 1 and 16 (BCD_HIP_MAX_LAYERS)");
        bcd_hip_host_layer hl[BCD_HIP_MAX_LAYERS];
        for (int k = 0; k < nb_layers; ++k) hl[k] = { layers[k].d_colors, layers[k].d_covariances, layers[k].d_out };
        return guide ? bcd_hip_denoise_guided_host(ctx, h_ns, nullptr, W, H, 0, nb_scales, prm, nullptr, var_floor, hl, nb_layers, guide)
                     : bcd_hip_denoise_moments_host(ctx, h_ns, W, H, nb_scales, prm, nullptr, var_floor, hl, nb_layers);
    }
    RCCHK(check_moments_call(ctx, h_ns, neighbours, nb_neighbours, h_motion, W, H, nb_scales, prm, layers, nb_layers, guide, neighbour_guides));
    ctx->moments.on = true; ctx->moments.var_floor = var_floor;
    int rc;
    if (guide) rc = guided_host_run(ctx, h_ns, nullptr, neighbours, nb_neighbours, h_motion, W, H, 0, nb_scales, prm, layers, nb_layers, guide, neighbour_guides);
    else rc = layers_host_run(ctx, h_ns, nullptr, neighbours, nb_neighbours, W, H, 0, nb_scales, prm, layers, nb_layers, any_field(h_motion, nb_neighbours) ? h_motion : nullptr);
    ctx->moments.on = false;
    return rc;
}

// ---- "Prefilter": the host frame calls behind one entry point, every frame through the spike prefilter on its own -------------------
int bcd_hip_denoise_temporal_host_ex(bcd_hip_ctx *ctx, const float *h_ns, const float *h_hist, const bcd_hip_frame_layers *neighbours, int nb_neighbours,
                                     const float *const *h_motion, int W, int H, int D, int nb_scales, const bcd_hip_params *prm, float var_floor,
                                     const bcd_hip_layer *layers, int nb_layers, const bcd_hip_guide *guide, const bcd_hip_guide_images *neighbour_guides,
                                     const bcd_hip_temporal_host_options *opt)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (opt && opt->reserved) return bad(ctx, "the reserved pointer of the options must be NULL");
    if (opt && !std::isfinite(opt->spike_factor)) return bad(ctx, "the spike factor must be finite");
    const float factor = opt ? opt->spike_factor : 0.f;
    if (factor > 0.f && (W < 3 || H < 3)) return bad(ctx, "image smaller than 3x3");
    if (factor > 0.f && nb_neighbours == 0) { // the single-frame host call of the mode with the factor over every layer
        if (!layers) return bad(ctx, "null layer list");
        if (nb_layers < 1 || nb_layers > BCD_HIP_MAX_LAYERS) return bad(ctx, "the number of layers must be between 1 and 16 (BCD_HIP_MAX_LAYERS)");
        bcd_hip_host_layer hl[BCD_HIP_MAX_LAYERS];
        for (int k = 0; k < nb_layers; ++k) hl[k] = { layers[k].d_colors, layers[k].d_covariances, layers[k].d_out };
        const bcd_hip_layers_host_options so = { factor, 0, 1 };
        // (the refusals the delegated call makes of these arguments ahead of ITS single-frame delegation: the layered calls check the whole call and the
        // motion list, the guided and the moment call go straight to the single-frame call)
        if (h_hist && !guide) {
            RCCHK(check_call(ctx, h_ns, h_hist, neighbours, nb_neighbours, W, H, D, nb_scales, prm, layers, nb_layers));
            float *outs[ML];
            layer_outs(layers, nb_layers, outs);
            if (h_motion) RCCHK(check_motion_list(ctx, h_motion, nb_neighbours, W, H, outs, nb_layers));
        }
        if (!h_hist) {
            RCCHK(check_moments_head(ctx, nb_neighbours, var_floor));
            return guide ? bcd_hip_denoise_guided_host(ctx, h_ns, nullptr, W, H, 0, nb_scales, prm, &so, var_floor, hl, nb_layers, guide)
                         : bcd_hip_denoise_moments_host(ctx, h_ns, W, H, nb_scales, prm, &so, var_floor, hl, nb_layers);
        }
        return guide ? bcd_hip_denoise_guided_host(ctx, h_ns, h_hist, W, H, D, nb_scales, prm, &so, 0.f, hl, nb_layers, guide)
                     : bcd_hip_denoise_layers_host_ex(ctx, h_ns, h_hist, W, H, D, nb_scales, prm, &so, hl, nb_layers);
    }
    // the existing host call that takes exactly these arguments; with a factor its uploads are followed by the in-place filter of every frame
    ctx->temporal.prefilter = factor > 0.f ? factor : 0.f;
    int rc;
    if (!h_hist)
        rc = bcd_hip_denoise_temporal_moments_host(ctx, h_ns, neighbours, nb_neighbours, h_motion, W, H, nb_scales, prm, var_floor, layers, nb_layers, guide, neighbour_guides);
    else if (guide)
        rc = bcd_hip_denoise_temporal_guided_host(ctx, h_ns, h_hist, neighbours, nb_neighbours, h_motion, W, H, D, nb_scales, prm, layers, nb_layers, guide, neighbour_guides);
    else if (h_motion)
        rc = bcd_hip_denoise_temporal_layers_motion_host(ctx, h_ns, h_hist, neighbours, nb_neighbours, h_motion, W, H, D, nb_scales, prm, layers, nb_layers);
    else
        rc = bcd_hip_denoise_temporal_layers_host(ctx, h_ns, h_hist, neighbours, nb_neighbours, W, H, D, nb_scales, prm, layers, nb_layers);
    ctx->temporal.prefilter = 0.f;
    return rc;
}

int bcd_hip_warp_layers(bcd_hip_ctx *ctx, const bcd_hip_frame_layer *layers, int nb_layers, const float *d_motion, int W, int H, const bcd_hip_warped_layer *out,
                        uint8_t *d_valid)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!layers || !out || !d_valid) return bad(ctx, "null argument");
    if (nb_layers < 1 || nb_layers > BCD_HIP_MAX_LAYERS) return bad(ctx, "the number of layers must be between 1 and 16 (BCD_HIP_MAX_LAYERS)");
    for (int k = 0; k < nb_layers; ++k)
        if (!layers[k].d_colors || !layers[k].d_covariances || !out[k].d_colors || !out[k].d_covariances) return bad(ctx, "null image pointer in a layer");
    bcd_hip_params p; bcd_hip_default_params(&p); p.patch_radius = 0; p.search_radius = 0;
    RCCHK(check_params(ctx, W, H, 1, &p));
    {
        const size_t npix = (size_t)W * H, bc = npix * 3 * sizeof(float), bv = npix * 6 * sizeof(float);
        std::vector<std::pair<const void *, size_t>> in, dst;
        for (int k = 0; k < nb_layers; ++k) {
            in.push_back({ layers[k].d_colors, bc }); in.push_back({ layers[k].d_covariances, bv });
            dst.push_back({ out[k].d_colors, bc }); dst.push_back({ out[k].d_covariances, bv });
        }
        if (d_motion) in.push_back({ d_motion, npix * 2 * sizeof(float) });
        dst.push_back({ d_valid, npix });
        for (size_t i = 0; i < dst.size(); ++i) {
            for (const auto &x : in) if (bytes_overlap(dst[i].first, dst[i].second, x.first, x.second)) return bad(ctx, "a warp destination overlaps an input image or the motion field");
            for (size_t j = 0; j < i; ++j) if (bytes_overlap(dst[i].first, dst[i].second, dst[j].first, dst[j].second)) return bad(ctx, "two warp destinations overlap");
        }
    }
    DEVICE_GUARD(ctx);
    BcdWarpLayerTable t = {};
    for (int k = 0; k < nb_layers; ++k) { t.col[k] = layers[k].d_colors; t.cov[k] = layers[k].d_covariances; t.ocol[k] = out[k].d_colors; t.ocov[k] = out[k].d_covariances; }
    HIPCHK(ctx, bcd_launch_warp_layers(t, nb_layers, d_motion, W, H, d_valid, ctx->main.stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
    return BCD_HIP_OK;
}

} // extern "C"
