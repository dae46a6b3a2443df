// bcd_temporal.hip -- similar patches from neighbouring frames of a sequence: the frame calls bcd_hip_denoise_temporal[_host], the
// stage entry points of the cross-frame selection and of the estimate over several frames, and the driver glue.  The kernels are in k_similarity_cross.hip
// and k_bayes_temporal.hip; the planes of one neighbour live in the main workspace's plane buffers (grow-only) and are consumed before the next
// neighbour's are written.  The motion calls (section 16, "Motion": bcd_hip_denoise_temporal_motion[_host], the stages bcd_hip_warp_frame,
// bcd_hip_valid_downscale, bcd_hip_gate_masks_valid) are here too: temporal_run warps a neighbour that has a motion field (k_warp.hip) before its pyramid is
// built and gates its cross masks at every scale; the plain call is temporal_run without fields.
// The feature gate of the cross-frame selection (section 16, "Features") is here as well: temporal_select's guide mode, the set-up of a guided temporal call
// (temporal_guide_begin) and the stages bcd_hip_similarity_masks_guide_cross, bcd_hip_window_distances_guide_cross, bcd_hip_warp_features; the kernels are in
// k_similarity_guide_cross.hip and k_warp.hip.
// The cross-frame selection from means and covariances (section 16, "Moments") is temporal_select's moments mode; its stages
// bcd_hip_similarity_masks_moments_cross and bcd_hip_window_distances_moments_cross are here, the kernels in k_similarity_moments_cross.hip, the frame calls
// bcd_hip_denoise_temporal_moments[_host] in bcd_temporal_layers.hip.
// What the frame calls, the layered calls (bcd_temporal_layers.hip) and the pops and pushes of a sequence (bcd_sequence.hip) share is defined here and
// declared in bcd_ctx.h: the one scale stage (temporal_scale: temporal_select, the estimate of either kind, the finalisation, temporal_stats_tail), the one
// pyramid level of a frame (temporal_build_level), the geometry refusals of a call with neighbour frames (check_temporal_geometry), the lists and the chain of
// full estimates of the estimate stage (temporal_lists, temporal_full_chain), the motion set-up of a neighbour (temporal_warp_neighbour).  The drivers --
// temporal_run here, layers_run, the pop of a sequence -- fill the tables of temporal_scale and merge the scales.
#include "bcd_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

static_assert(BCD_MAX_NEIGHBOURS == BCD_HIP_MAX_NEIGHBOURS, "the frame table of the kernels holds what the C ABI admits");

namespace {

// what the three kinds of cross planes share ahead of their kernel: room for the T / C planes of every displacement in the main workspace's plane buffers
// (whose own planes they overwrite) and, for a kernel that is timed like the other distance kernels (bcd_hip_kernel_time), the event pair with its first
// event recorded.  -> *e1 (null: untimed, or the pool is used up), which the caller records behind the kernel
int cross_planes_begin(bcd_hip_ctx *ctx, Work &wk, int W, int H, int b, bool timed, hipEvent_t *e1)
{
    const size_t npix = (size_t)W * H, n = (size_t)(2 * b + 1) * (2 * b + 1);
    RCCHK(ensure(ctx, wk.T, npix * n * sizeof(float)));
    RCCHK(ensure(ctx, wk.Cn, count_plane_bytes(npix, (int)n)));
    wk.planes.ready = false; // (the workspace's planes are overwritten)
    hipEvent_t e0 = nullptr;
    *e1 = nullptr;
    if (timed) RCCHK(distance_timing_events(ctx, wk, &e0, e1));
    if (e0) HIPCHK(ctx, hipEventRecord(e0, wk.stream));
    return BCD_HIP_OK;
}

// the T / C planes of every displacement between the frame and one neighbour
int temporal_cross_planes(bcd_hip_ctx *ctx, Work &wk, const float *d_hist, const float *d_ns, const float *d_hist_nb, const float *d_ns_nb, int W, int H, int D, int b)
{
    hipEvent_t e1;
    RCCHK(cross_planes_begin(ctx, wk, W, H, b, false, &e1));
    HIPCHK(ctx, bcd_launch_pairdist_cross(d_hist, d_ns, d_hist_nb, d_ns_nb, W, H, D, b, (float *)wk.T.p, (uint8_t *)wk.Cn.p, wk.stream));
    return BCD_HIP_OK;
}

// "Features": the T / C planes of every displacement between the feature images of the frame and of one neighbour, in the same plane buffers -- the histogram
// planes of that neighbour are consumed by then.  The kernel is timed
int temporal_guide_cross_planes(bcd_hip_ctx *ctx, Work &wk, const float *d_feat, const float *d_var, const float *d_feat_nb, const float *d_var_nb, int F,
                                const float *floors, int W, int H, int b)
{
    hipEvent_t e1;
    RCCHK(cross_planes_begin(ctx, wk, W, H, b, true, &e1));
    HIPCHK(ctx, bcd_launch_pairdist_guide_cross(d_feat, d_var, d_feat_nb, d_var_nb, F, floors, W, H, b, (float *)wk.T.p, (uint8_t *)wk.Cn.p, wk.stream));
    if (e1) HIPCHK(ctx, hipEventRecord(e1, wk.stream));
    return BCD_HIP_OK;
}

// "Features": the gate of one neighbour's cross masks, behind k_masks_cross (and the validity gate) on wk.stream: the cross feature planes, k_masks_cross on
// them with tau_g into the workspace's gate buffers, then mask &= G_j and |S_j| = the bits that remain.  Channels, floors and threshold are ctx->guide's
int temporal_guide_gate(bcd_hip_ctx *ctx, Work &wk, const TemporalSelFrame &frame, const TemporalSelFrame &nb, int W, int H, int w, int b, uint32_t *d_mask_nb,
                        int32_t *d_count_nb)
{
    const size_t npix = (size_t)W * H, words = ((size_t)(2 * b + 1) * (2 * b + 1) + 31) / 32;
    RCCHK(ensure(ctx, wk.gate_mask, npix * words * sizeof(uint32_t)));
    RCCHK(ensure(ctx, wk.gate_nsim, npix * sizeof(int32_t)));
    ++ctx->temporal.guide_cross_passes;
    RCCHK(temporal_guide_cross_planes(ctx, wk, frame.feat, frame.var, nb.feat, nb.var, ctx->guide.F, ctx->guide.floors, W, H, b));
    HIPCHK(ctx, bcd_launch_masks_cross((const float *)wk.T.p, (const uint8_t *)wk.Cn.p, W, H, w, b, ctx->guide.tau, (uint32_t *)wk.gate_mask.p, (int32_t *)wk.gate_nsim.p,
                                       wk.stream));
    HIPCHK(ctx, bcd_launch_gate_masks(d_mask_nb, (const uint32_t *)wk.gate_mask.p, d_count_nb, W, H, b, wk.stream));
    return BCD_HIP_OK;
}

// "Moments": the form of the moment cross pass that `form` asks for (0: the production choice) at this geometry -- 1 the planes, 2 the kernel without planes.
// The production choice is the fused kernel where it applies (w = 1, b <= 6: the only geometry of the frame calls) and the planes elsewhere: at 1080p, b = 6 the
// cross stage of one neighbour takes 2.32 ms fused against 3.40 ms as planes + k_masks_cross (docs/EXPERIMENTS.md section 27)
constexpr int MOMENTS_CROSS_PRODUCTION_FORM = 2;
int moments_cross_form(int form, int w, int b)
{
    if (form == 0) form = MOMENTS_CROSS_PRODUCTION_FORM;
    return form == 2 && !bcd_masks_moments_cross_fused_applies(w, b) ? 1 : form;
}

// "Moments": the T / C planes of every displacement between the guide layers of the frame and of one neighbour, in the same plane buffers; the kernel is timed
int temporal_moments_cross_planes(bcd_hip_ctx *ctx, Work &wk, const float *d_col, const float *d_pixcov, const float *d_col_nb, const float *d_pixcov_nb, int W, int H,
                                  int b, float var_floor)
{
    hipEvent_t e1;
    RCCHK(cross_planes_begin(ctx, wk, W, H, b, true, &e1));
    HIPCHK(ctx, bcd_launch_pairdist_moments_cross(d_col, d_pixcov, d_col_nb, d_pixcov_nb, W, H, b, var_floor, (float *)wk.T.p, (uint8_t *)wk.Cn.p, wk.stream));
    if (e1) HIPCHK(ctx, hipEventRecord(e1, wk.stream));
    return BCD_HIP_OK;
}

// "Moments": the cross masks and counts of one neighbour on wk.stream, in the form `form` (1 or 2, from moments_cross_form)
int temporal_moments_cross_masks(bcd_hip_ctx *ctx, Work &wk, const float *d_col, const float *d_pixcov, const float *d_col_nb, const float *d_pixcov_nb, int W, int H,
                                 int w, int b, float tau, float var_floor, int form, uint32_t *d_mask_nb, int32_t *d_count_nb)
{
    if (form == 2) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        RCCHK(distance_timing_events(ctx, wk, &e0, &e1));
        if (e0) HIPCHK(ctx, hipEventRecord(e0, wk.stream));
        HIPCHK(ctx, bcd_launch_masks_moments_cross_fused(d_col, d_pixcov, d_col_nb, d_pixcov_nb, W, H, b, tau, var_floor, d_mask_nb, d_count_nb, wk.stream));
        if (e1) HIPCHK(ctx, hipEventRecord(e1, wk.stream));
        return BCD_HIP_OK;
    }
    RCCHK(temporal_moments_cross_planes(ctx, wk, d_col, d_pixcov, d_col_nb, d_pixcov_nb, W, H, b, var_floor));
    HIPCHK(ctx, bcd_launch_masks_cross((const float *)wk.T.p, (const uint8_t *)wk.Cn.p, W, H, w, b, tau, d_mask_nb, d_count_nb, wk.stream));
    return BCD_HIP_OK;
}

// the gate of a warped neighbour's cross masks (the stream's next step behind k_masks_cross): pvalid from the level's validity bytes, then the bits and |S_f|
int temporal_gate(bcd_hip_ctx *ctx, Work &wk, const uint8_t *d_valid, int W, int H, int w, int b, uint32_t *d_mask_nb, int32_t *d_count_nb)
{
    DevBuf &pv = ctx->temporal.pvalid;
    RCCHK(ensure(ctx, pv, (size_t)W * H));
    HIPCHK(ctx, bcd_launch_valid_patch(d_valid, W, H, w, (uint8_t *)pv.p, wk.stream));
    HIPCHK(ctx, bcd_launch_masks_gate_valid(d_mask_nb, d_count_nb, (const uint8_t *)pv.p, W, H, w, b, wk.stream));
    return BCD_HIP_OK;
}

} // namespace

int temporal_warp_neighbour(bcd_hip_ctx *ctx, int f, int nf, const float *col, const float *ns, const float *hist, const float *cov, const float *motion, int W, int H,
                            int D, int S, const BcdWarpLayerTable *more, int nb_more, const uint8_t **valid, const float *warped[4])
{
    auto &tp = ctx->temporal;
    hipStream_t st = ctx->main.stream;
    const size_t npix = (size_t)W * H, floats[4] = { npix * 3, npix, npix * D, npix * 6 };
    DevBuf(&wb)[4] = tp.warp[f];
    for (int k = 0; k < 4; ++k) RCCHK(ensure(ctx, wb[k], floats[k] * sizeof(float)));
    RCCHK(ensure(ctx, tp.valid[f][0], npix));
    uint8_t *v0 = (uint8_t *)tp.valid[f][0].p;
    HIPCHK(ctx, bcd_launch_warp_frame(col, ns, hist, cov, motion, W, H, D, (float *)wb[0].p, (float *)wb[1].p, (float *)wb[2].p, (float *)wb[3].p, v0, st));
    if (more) HIPCHK(ctx, bcd_launch_warp_layers(*more, nb_more, motion, W, H, v0, st)); // (it writes the same validity bytes again)
    for (int s = 1, ws = W, hs = H; s < S; ++s, ws /= 2, hs /= 2) {
        RCCHK(ensure(ctx, tp.valid[f][s], (size_t)(ws / 2) * (hs / 2)));
        HIPCHK(ctx, bcd_launch_valid_down((const uint8_t *)tp.valid[f][s - 1].p, ws, hs, (uint8_t *)tp.valid[f][s].p, st));
    }
    for (int k = 0; k < 4; ++k) warped[k] = (const float *)wb[k].p;
    for (int s = 0; s < S; ++s) valid[(size_t)s * nf + f] = (const uint8_t *)tp.valid[f][s].p;
    return BCD_HIP_OK;
}

int check_motion_list(bcd_hip_ctx *ctx, const float *const *motion, int nb_neighbours, int W, int H, float *const *outs, int nb_outs)
{
    if (nb_neighbours > 0 && !motion) return bad(ctx, "null motion list with neighbour frames present (an entry may be NULL: zero motion)");
    const size_t npix = (size_t)W * H;
    for (int f = 0; f < nb_neighbours; ++f)
        for (int k = 0; motion[f] && k < nb_outs; ++k)
            if (bytes_overlap(outs[k], npix * 3 * sizeof(float), motion[f], npix * 2 * sizeof(float))) return bad(ctx, "an output overlaps a motion field");
    return BCD_HIP_OK;
}

bool overlaps_frame_images(const void *out, size_t bytes, const void *col, const void *ns, const void *hist, const void *cov, size_t npix, int D)
{
    const size_t f4 = sizeof(float);
    return (col && bytes_overlap(out, bytes, col, npix * 3 * f4)) || (ns && bytes_overlap(out, bytes, ns, npix * f4)) ||
           (hist && bytes_overlap(out, bytes, hist, npix * D * f4)) || (cov && bytes_overlap(out, bytes, cov, npix * 6 * f4));
}

int temporal_lists(bcd_hip_ctx *ctx, Work &wk, const int32_t *d_nsim_total, const uint8_t *d_state, int64_t npix, TemporalLists *out)
{
    constexpr int K = 27;
    wk.redo.pending = false;
    RCCHK(ensure(ctx, wk.strong, npix * sizeof(int32_t)));
    RCCHK(ensure(ctx, wk.weak, npix * sizeof(int32_t)));
    RCCHK(ensure(ctx, wk.counters, sizeof(Counters)));
    RCCHK(ensure(ctx, wk.work_q, BCD_WORK_INTS * sizeof(int32_t)));
    Counters::Lists *d_c = &wk.d_counters()->lists, *h_c = &wk.h_counters->lists;
    touch(wk); // (the counters and work queues are cleared here, whatever k_scale_begin left)
    h_c->spectral = 0;
    HIPCHK(ctx, hipMemsetAsync(d_c, 0, sizeof(*d_c), wk.stream));
    HIPCHK(ctx, bcd_launch_active_lists(d_state, d_nsim_total, 0, npix, K + 1, (int32_t *)wk.strong.p, (int32_t *)wk.weak.p, &d_c->n_strong, wk.stream, nullptr));
    HIPCHK(ctx, hipMemcpyAsync(h_c, d_c, offsetof(Counters::Lists, generic_work), hipMemcpyDeviceToHost, wk.stream)); // (the list lengths and the sum of |S|)
    out->cus = std::max(1, ctx->num_cus * ctx->cu_share_pct / 100);
    out->weak_grid = (int)std::min<int64_t>(std::max<int64_t>(1, npix / 7), (int64_t)out->cus * 32);
    return BCD_HIP_OK;
}

int temporal_full_chain(bcd_hip_ctx *ctx, Work &wk, const BcdFrameTable &t, float *d_sum, int32_t *d_count, int n_strong, int cus, int W, int H, int b, float min_eig)
{
    if (n_strong < 0 || n_strong > (int64_t)W * H) return bad(ctx, "temporal estimate: the list exceeds the frame");
    if (n_strong > 0) RCCHK(ensure(ctx, wk.gscratch, bcd_bayes27_record_bytes() * (size_t)std::min(n_strong, ESTIMATE_CHUNK)));
    for (int first = 0; first < n_strong; first += ESTIMATE_CHUNK) {
        const int n = std::min(ESTIMATE_CHUNK, n_strong - first);
        HIPCHK(ctx, hipMemsetAsync(wk.work_q.p, 0, BCD_WORK_INTS * sizeof(int32_t), wk.stream)); // the work queues of the four kernels
        HIPCHK(ctx, bcd_launch_prepare27t(t, (const int32_t *)wk.strong.p, first, n, (int *)wk.work_q.p, cus, W, b, (float *)wk.gscratch.p, wk.stream));
        HIPCHK(ctx, bcd_launch_solve_finish27(t.col[0], t.pixcov[0], t.mask[0], (const int32_t *)wk.strong.p, first, n, (int *)wk.work_q.p, cus, W, H, min_eig,
                                              (float *)wk.gscratch.p, d_sum, d_count, &wk.d_counters()->lists.spectral, wk.stream));
    }
    return BCD_HIP_OK;
}

namespace {

// the refusals the stage calls share: the geometry rules of bcd_hip_similarity_masks
int check_cross_stage(bcd_hip_ctx *ctx, int W, int H, int D, int w, int b)
{
    bcd_hip_params p; bcd_hip_default_params(&p); p.patch_radius = w; p.search_radius = b;
    return check_params(ctx, W, H, D, &p);
}

// the tail of the three bcd_hip_window_distances_*_cross calls, behind the planes on wk.stream: the window of one main pixel, through ctx->tmp_lo to the host
int window_distances_tail(bcd_hip_ctx *ctx, Work &wk, int W, int H, int w, int b, int line, int col, float *h_out)
{
    const int n = (2 * b + 1) * (2 * b + 1);
    RCCHK(ensure(ctx, ctx->tmp_lo, n * sizeof(float)));
    HIPCHK(ctx, bcd_launch_window_distances_cross((const float *)wk.T.p, (const uint8_t *)wk.Cn.p, W, H, w, b, line, col, (float *)ctx->tmp_lo.p, wk.stream));
    HIPCHK(ctx, hipMemcpyAsync(h_out, ctx->tmp_lo.p, n * sizeof(float), hipMemcpyDeviceToHost, wk.stream));
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    return BCD_HIP_OK;
}

} // namespace

// The estimate stage over the members of several frames (patch radius 1, search radius 6): the lists, the fallback kernel over all frames, the wait for the
// list lengths, one chain of full estimates on the frame's own colours and in-frame masks, the redo count.  The list lengths and the sum of |S| are in
// wk.h_counters->lists when the call returns (it synchronises the stream at its end).
int bayes_temporal(bcd_hip_ctx *ctx, Work &wk, const BcdFrameTable &t, const int32_t *d_nsim_total, const uint8_t *d_state, int W, int H, int b, float min_eig,
                   float *d_sum, int32_t *d_count)
{
    TemporalLists ls;
    RCCHK(temporal_lists(ctx, wk, d_nsim_total, d_state, (int64_t)W * H, &ls));
    Counters::Lists *d_c = &wk.d_counters()->lists, *h_c = &wk.h_counters->lists;
    HIPCHK(ctx, bcd_launch_bayes_weak_temporal(t, (const int32_t *)wk.weak.p, &d_c->n_weak, ls.weak_grid, W, b, d_sum, d_count, wk.stream));
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    RCCHK(temporal_full_chain(ctx, wk, t, d_sum, d_count, h_c->n_strong, ls.cus, W, H, b, min_eig));
    HIPCHK(ctx, hipMemcpyAsync(&h_c->spectral, &d_c->spectral, sizeof(int32_t), hipMemcpyDeviceToHost, wk.stream));
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    return BCD_HIP_OK;
}

extern "C" {

int bcd_hip_bayes_accumulate_temporal(bcd_hip_ctx *ctx, const bcd_hip_stage_frame *frames, int nb_frames, const int32_t *d_nsim_total, const uint8_t *d_state, int W,
                                      int H, int w, int b, float min_eig, float *d_sum, int32_t *d_count)
{
    if (!ctx) return BCD_HIP_EINVAL;
    // ---- everything is checked before any device work
    if (!frames) return bad(ctx, "null frame list");
    if (nb_frames < 1 || nb_frames > BCD_HIP_MAX_NEIGHBOURS + 1) return bad(ctx, "the number of frames must be between 1 and 5 (the frame and up to BCD_HIP_MAX_NEIGHBOURS neighbours)");
    if (!d_nsim_total || !d_state || !d_sum || !d_count) return bad(ctx, "null image pointer");
    for (int f = 0; f < nb_frames; ++f)
        if (!frames[f].d_colors || !frames[f].d_pixel_cov || !frames[f].d_mask) return bad(ctx, "null image pointer in a frame");
    bcd_hip_params p; bcd_hip_default_params(&p); p.patch_radius = w; p.search_radius = b;
    RCCHK(check_params(ctx, W, H, 1, &p));
    if (w != 1 || b != 6) { set_err(ctx, "the estimate over several frames supports patch radius 1 and search radius 6"); return BCD_HIP_EUNSUPPORTED; }
    {
        const size_t npix = (size_t)W * H, f4 = sizeof(float), words = ((size_t)(2 * b + 1) * (2 * b + 1) + 31) / 32, nsum = npix * 3 * f4, ncnt = npix * 4;
        if (bytes_overlap(d_sum, nsum, d_count, ncnt) || bytes_overlap(d_sum, nsum, d_nsim_total, npix * 4) || bytes_overlap(d_sum, nsum, d_state, npix) ||
            bytes_overlap(d_count, ncnt, d_nsim_total, npix * 4) || bytes_overlap(d_count, ncnt, d_state, npix))
            return bad(ctx, "the accumulators overlap each other or the selection");
        for (int f = 0; f < nb_frames; ++f)
            for (const void *o : { (const void *)d_sum, (const void *)d_count })
                if (overlaps_frame_images(o, o == d_sum ? nsum : ncnt, frames[f].d_colors, nullptr, nullptr, frames[f].d_pixel_cov, npix, 0) ||
                    bytes_overlap(o, o == d_sum ? nsum : ncnt, frames[f].d_mask, npix * words * 4))
                    return bad(ctx, "an accumulator overlaps an input image");
    }
    DEVICE_GUARD(ctx);
    BcdFrameTable t = {};
    t.n = nb_frames;
    for (int f = 0; f < nb_frames; ++f) { t.col[f] = frames[f].d_colors; t.pixcov[f] = frames[f].d_pixel_cov; t.mask[f] = frames[f].d_mask; }
    return bayes_temporal(ctx, ctx->main, t, d_nsim_total, d_state, W, H, b, min_eig, d_sum, d_count);
}

int bcd_hip_similarity_masks_cross(bcd_hip_ctx *ctx, const float *d_hist, const float *d_ns, const float *d_hist_nb, const float *d_ns_nb, int W, int H, int D,
                                   int w, int b, float tau, uint32_t *d_mask_nb, int32_t *d_count_nb)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_hist || !d_ns || !d_hist_nb || !d_ns_nb || !d_mask_nb || !d_count_nb) return bad(ctx, "bad argument");
    RCCHK(check_cross_stage(ctx, W, H, D, w, b));
    DEVICE_GUARD(ctx);
    Work &wk = ctx->main;
    RCCHK(temporal_cross_planes(ctx, wk, d_hist, d_ns, d_hist_nb, d_ns_nb, W, H, D, b));
    HIPCHK(ctx, bcd_launch_masks_cross((const float *)wk.T.p, (const uint8_t *)wk.Cn.p, W, H, w, b, tau, d_mask_nb, d_count_nb, wk.stream));
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    return BCD_HIP_OK;
}

int bcd_hip_window_distances_cross(bcd_hip_ctx *ctx, const float *d_hist, const float *d_ns, const float *d_hist_nb, const float *d_ns_nb, int W, int H, int D,
                                   int w, int b, int line, int col, float *h_out)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_hist || !d_ns || !d_hist_nb || !d_ns_nb || !h_out) return bad(ctx, "bad argument");
    RCCHK(check_cross_stage(ctx, W, H, D, w, b));
    if (line < w || line > H - 1 - w || col < w || col > W - 1 - w) return bad(ctx, "not a main pixel");
    DEVICE_GUARD(ctx);
    Work &wk = ctx->main;
    RCCHK(temporal_cross_planes(ctx, wk, d_hist, d_ns, d_hist_nb, d_ns_nb, W, H, D, b));
    return window_distances_tail(ctx, wk, W, H, w, b, line, col, h_out);
}

} // extern "C"

// =====================================================================================================================
// The frame call.  Every neighbour gets its own pyramid, built with the reducers of the frame's; scale s uses level s of every frame; the scales run
// coarse to fine, one after the other, on the main workspace, each through the stage calls of this library in the order of DESIGN.md section 16: the
// in-frame selection (the code that computes it today), one cross pass per neighbour ahead of the marking, the marking on the in-frame masks and the
// total |S|, the estimate over all frames, the finalisation, then the merge of the (already merged) coarser scale as in bcd_hip_denoise.
// =====================================================================================================================
void temporal_free(bcd_hip_ctx *ctx)
{
    auto &t = ctx->temporal;
    free_bufs(t.pyr, sizeof t.pyr);
    free_bufs(t.out, sizeof t.out);
    free_bufs(t.pixcov, sizeof t.pixcov);
    free_bufs(t.mask, sizeof t.mask);
    free_bufs(&t.count_nb, sizeof t.count_nb);
    free_bufs(t.host, sizeof t.host);
    free_bufs(&t.host_out, sizeof t.host_out);
    free_bufs(t.lay_pyr, sizeof t.lay_pyr);
    free_bufs(t.lay_out, sizeof t.lay_out);
    free_bufs(t.lay_pixcov, sizeof t.lay_pixcov);
    free_bufs(&t.lay_sum, sizeof t.lay_sum);
    free_bufs(&t.lay_tmp_lo, sizeof t.lay_tmp_lo);
    free_bufs(t.lay_host, sizeof t.lay_host);
    free_bufs(&t.lay_host_out, sizeof t.lay_host_out);
    free_bufs(t.warp, sizeof t.warp);
    free_bufs(t.lay_warp, sizeof t.lay_warp);
    free_bufs(t.valid, sizeof t.valid);
    free_bufs(&t.pvalid, sizeof t.pvalid);
    free_bufs(t.motion_host, sizeof t.motion_host);
    free_bufs(t.guide_pyr, sizeof t.guide_pyr);
    free_bufs(t.guide_warp, sizeof t.guide_warp);
    free_bufs(t.guide_host, sizeof t.guide_host);
}

int temporal_select(bcd_hip_ctx *ctx, const TemporalSelFrame *frames, int nf, int W, int H, int D, const bcd_hip_params *prm, int scale,
                    const std::function<int()> &per_pixel_cov, TemporalPath *path)
{
    Work &wk = ctx->main;
    auto &tp = ctx->temporal;
    const int w = prm->patch_radius, b = prm->search_radius;
    const float tau = prm->hist_dist_threshold;
    const size_t npix = (size_t)W * H, words = ((size_t)(2 * b + 1) * (2 * b + 1) + 31) / 32;
    RCCHK(ensure(ctx, wk.mask, npix * words * sizeof(uint32_t)));
    RCCHK(ensure(ctx, wk.nsim, npix * sizeof(int32_t)));
    RCCHK(ensure(ctx, wk.state, npix));
    RCCHK(ensure(ctx, wk.cnt, npix * sizeof(int32_t)));
    RCCHK(ensure(ctx, tp.count_nb, npix * sizeof(int32_t)));
    for (int f = 1; f < nf; ++f) if (!frames[f].mask_dst) RCCHK(ensure(ctx, tp.mask[f], npix * words * sizeof(uint32_t)));
    bcd_hip_scale_stats &st = ctx->stats[scale];
    memset(&st, 0, sizeof(st));
    st.width = W; st.height = H;
    st.main_pixels = (int64_t)std::max(0, W - 2 * w) * std::max(0, H - 2 * w);
    const bool prof = ctx->profiling;
    if (prof) HIPCHK(ctx, hipEventRecord(wk.ev_stage[0], wk.stream));
    // S_0: today's set, by the code that computes it today (its verdict and re-runs are inside the call); the cross passes follow it, ahead of the marking
    const bool moments = ctx->moments.on; // ("Moments": the per-pixel covariances first, S_0 by similarity_moments, every S_j by the moment cross pass)
    const float eps = ctx->moments.var_floor;
    if (moments) {
        RCCHK(per_pixel_cov());
        RCCHK(moments_masks(ctx, wk, frames[0].col, frames[0].pixcov, W, H, w, b, tau, eps, (uint32_t *)wk.mask.p, (int32_t *)wk.nsim.p));
        path->path = 3; path->borderline = 0;
    } else {
        RCCHK(bcd_hip_similarity_masks(ctx, frames[0].hist, frames[0].ns, W, H, D, w, b, tau, (uint32_t *)wk.mask.p, (int32_t *)wk.nsim.p));
        int32_t capacity = 0;
        RCCHK(bcd_hip_similarity_last_path(ctx, &path->path, &path->borderline, &capacity));
    }
    const bool guided = frames[0].feat != nullptr; // ("Features": S_0 is gated as a guided scale gates it, every S_j by its cross feature mask)
    if (guided) RCCHK(guide_gate_masks(ctx, wk, frames[0].feat, frames[0].var, W, H, w, b, (uint32_t *)wk.mask.p, (int32_t *)wk.nsim.p));
    if (!moments) RCCHK(per_pixel_cov());
    for (int f = 1; f < nf; ++f) {
        uint32_t *mask = frames[f].mask_dst ? frames[f].mask_dst : (uint32_t *)tp.mask[f].p; // ("Sequences": the sequence's own buffer)
        int32_t *count = (int32_t *)tp.count_nb.p;
        if (frames[f].transpose_from) { // ("Sequences": the pair was searched from the other side; no planes are written)
            HIPCHK(ctx, bcd_launch_masks_transpose(frames[f].transpose_from, W, H, b, mask, count, wk.stream));
        } else if (moments) {
            RCCHK(temporal_moments_cross_masks(ctx, wk, frames[0].col, frames[0].pixcov, frames[f].col, frames[f].pixcov, W, H, w, b, tau, eps, moments_cross_form(0, w, b),
                                               mask, count));
        } else {
            RCCHK(temporal_cross_planes(ctx, wk, frames[0].hist, frames[0].ns, frames[f].hist, frames[f].ns, W, H, D, b));
            HIPCHK(ctx, bcd_launch_masks_cross((const float *)wk.T.p, (const uint8_t *)wk.Cn.p, W, H, w, b, tau, mask, count, wk.stream));
        }
        if (frames[f].valid) RCCHK(temporal_gate(ctx, wk, frames[f].valid, W, H, w, b, mask, count)); // (a warped neighbour)
        // ("Sequences": kept masks are the gated ones, and transposition distributes over the AND -- a transposed neighbour is not gated again)
        if (guided && !frames[f].transpose_from) RCCHK(temporal_guide_gate(ctx, wk, frames[0], frames[f], W, H, w, b, mask, count));
        HIPCHK(ctx, bcd_launch_add_counts((int32_t *)wk.nsim.p, count, (int64_t)npix, wk.stream));
    }
    if (prof) HIPCHK(ctx, hipEventRecord(wk.ev_stage[1], wk.stream));
    RCCHK(bcd_hip_active_set(ctx, (const uint32_t *)wk.mask.p, (const int32_t *)wk.nsim.p, W, H, w, b, 0, H, prm->marked_skip_probability, prm->use_random_pixel_order,
                             bcd_hip_scale_seed(prm->order_seed, scale), (uint8_t *)wk.state.p, &st.active_rounds));
    if (prof) HIPCHK(ctx, hipEventRecord(wk.ev_stage[2], wk.stream));
    return BCD_HIP_OK;
}

void temporal_stats_tail(bcd_hip_ctx *ctx, int scale, const TemporalPath &path)
{
    Work &wk = ctx->main;
    bcd_hip_scale_stats &st = ctx->stats[scale];
    const Counters::Lists &h = wk.h_counters->lists;
    st.processed = (int64_t)h.n_strong + h.n_weak; st.fallback = h.n_weak; st.similar_total = h.sim_total; // (the sum of the TOTAL |S|)
    st.similarity_path = path.path; st.borderline_pairs = path.borderline;                                // (those of the in-frame pass)
    st.cu_share = ctx->cu_share_pct;
    st.spectral_inverses = h.spectral;                                                                    // (a layered call: the sum over the layers)
    if (ctx->profiling) {
        st.ms_similarity = stage_ms(wk, 0, 1); // (includes the cross passes)
        st.ms_active = stage_ms(wk, 1, 2);
        st.ms_bayes = stage_ms(wk, 2, 3);
        st.ms_total = stage_ms(wk, 0, 3);
    }
}

int temporal_build_level(bcd_hip_ctx *ctx, const TemporalFrame &fine, const TemporalFrame &coarse, int L, bool layered, int W, int H, int D, hipStream_t st)
{
    if (!layered) HIPCHK(ctx, bcd_launch_downscale(1, fine.col[0], W, H, 3, const_cast<float *>(coarse.col[0]), st));
    HIPCHK(ctx, bcd_launch_downscale(0, fine.sel.ns, W, H, 1, const_cast<float *>(coarse.sel.ns), st));
    if (fine.sel.hist) HIPCHK(ctx, bcd_launch_downscale(0, fine.sel.hist, W, H, D, const_cast<float *>(coarse.sel.hist), st));
    if (!layered) {
        HIPCHK(ctx, bcd_launch_downscale_cov(fine.cov[0], fine.sel.ns, W, H, const_cast<float *>(coarse.cov[0]), st));
        return BCD_HIP_OK;
    }
    LayerView lf, lc;
    lf.n = lc.n = L;
    for (int k = 0; k < L; ++k) { lf.col[k] = fine.col[k]; lf.cov[k] = fine.cov[k]; lc.col[k] = coarse.col[k]; lc.cov[k] = coarse.cov[k]; }
    return build_level_layers(ctx, lf, lc, fine.sel.ns, W, H, st);
}

namespace {

constexpr int NF = BCD_MAX_NEIGHBOURS + 1, ML = BCD_MAX_LAYERS;

// the estimate of one layer of histograms and its finalisation (the stage-3 event between them): bayes_temporal on the frames' first layers
int scale_estimate(bcd_hip_ctx *ctx, Work &wk, const TemporalScale &sc, const uint32_t *const *mask, int W, int H, const bcd_hip_params *prm)
{
    BcdFrameTable t = {};
    t.n = sc.nf;
    for (int f = 0; f < sc.nf; ++f) { t.col[f] = sc.fr[f].col[0]; t.pixcov[f] = sc.fr[f].pixcov; t.mask[f] = mask[f]; }
    RCCHK(bayes_temporal(ctx, wk, t, (const int32_t *)wk.nsim.p, (const uint8_t *)wk.state.p, W, H, prm->search_radius, prm->min_eigen_value, sc.sum, (int32_t *)wk.cnt.p));
    if (ctx->profiling) HIPCHK(ctx, hipEventRecord(wk.ev_stage[3], wk.stream));
    HIPCHK(ctx, bcd_launch_finalize(sc.sum, (const int32_t *)wk.cnt.p, (int64_t)W * H, sc.out[0], wk.stream));
    return BCD_HIP_OK;
}

// the layered estimate and its finalisation: bayes_temporal_layers on every layer of the frames; redo[k]: the items of layer k that took the redo list
int scale_estimate_layers(bcd_hip_ctx *ctx, Work &wk, const TemporalScale &sc, const uint32_t *const *mask, int W, int H, const bcd_hip_params *prm, int32_t *redo)
{
    const int L = sc.L;
    const size_t npix = (size_t)W * H;
    LayerFrames lf;
    lf.nf = sc.nf; lf.L = L;
    float *sum[ML];
    for (int k = 0; k < L; ++k) sum[k] = sc.sum + (size_t)k * npix * 3;
    for (int f = 0; f < sc.nf; ++f) {
        for (int k = 0; k < L; ++k) { lf.col[f][k] = sc.fr[f].col[k]; lf.pixcov[f][k] = sc.fr[f].pixcov + (size_t)k * npix * 6; }
        lf.mask[f] = mask[f];
    }
    RCCHK(bayes_temporal_layers(ctx, wk, lf, (const int32_t *)wk.nsim.p, (const uint8_t *)wk.state.p, W, H, prm->search_radius, prm->min_eigen_value, sum, (int32_t *)wk.cnt.p,
                                redo));
    if (ctx->profiling) HIPCHK(ctx, hipEventRecord(wk.ev_stage[3], wk.stream));
    BcdLayerTable t = {};
    for (int k = 0; k < L; ++k) { t.a[k] = sum[k]; t.o[k] = sc.out[k]; }
    HIPCHK(ctx, bcd_launch_layers_finalize(t, L, (const int32_t *)wk.cnt.p, (int64_t)npix, wk.stream));
    return BCD_HIP_OK;
}

} // namespace

// One scale of every call with neighbour frames (the frame calls, the layered calls, the pops of a sequence), sc.fr[0] the frame itself at this level: the
// selection stage (temporal_select), the cleared accumulators, the estimate of the kind sc.layered names, the finalisation, the stats tail.  Where the
// per-pixel covariances come from, where a neighbour's masks go and whether the in-frame masks are copied out is all in `sc`
int temporal_scale(bcd_hip_ctx *ctx, const TemporalScale &sc, int W, int H, int D, const bcd_hip_params *prm, int scale)
{
    Work &wk = ctx->main;
    const int nf = sc.nf, L = sc.L;
    const size_t npix = (size_t)W * H, sum_bytes = npix * 3 * sizeof(float);
    TemporalSelFrame sel[NF];
    for (int f = 0; f < nf; ++f) {
        sel[f] = sc.fr[f].sel;
        if (ctx->moments.on) { sel[f].col = sc.fr[f].col[0]; sel[f].pixcov = sc.fr[f].pixcov; } // ("Moments": the guide layer is layer 0)
    }
    TemporalPath path;
    // the per-pixel covariances of every frame unless the pushes of a sequence computed them; a layered estimate clears its sums here: in the one launch
    // that produces the covariances of a frame's layers (so once per frame: there is no layered launcher that leaves the sums alone), or by hipMemsetAsync
    RCCHK(temporal_select(ctx, sel, nf, W, H, D, prm, scale, [&]() -> int {
        if (sc.pixcov_ready && sc.layered) HIPCHK(ctx, hipMemsetAsync(sc.sum, 0, L * sum_bytes, wk.stream));
        for (int f = 0; f < nf && !sc.pixcov_ready; ++f) {
            const TemporalFrame &fr = sc.fr[f];
            if (!sc.layered) { HIPCHK(ctx, bcd_launch_pixel_cov(fr.cov[0], fr.sel.ns, (int64_t)npix, fr.pixcov, wk.stream)); continue; }
            BcdLayerTable t = {};
            for (int k = 0; k < L; ++k) t.a[k] = fr.cov[k];
            HIPCHK(ctx, bcd_launch_layers_pixel_cov_clear(t, L, fr.sel.ns, (int64_t)npix, fr.pixcov, sc.sum, wk.stream));
        }
        return BCD_HIP_OK;
    }, &path));
    const size_t words = ((size_t)(2 * prm->search_radius + 1) * (2 * prm->search_radius + 1) + 31) / 32;
    if (sc.self_copy) HIPCHK(ctx, hipMemcpyAsync(sc.self_copy, wk.mask.p, npix * words * sizeof(uint32_t), hipMemcpyDeviceToDevice, wk.stream));
    const uint32_t *mask[NF]; // what temporal_select left: the in-frame masks, and per neighbour the caller's buffer or the context's
    for (int f = 0; f < nf; ++f) mask[f] = f == 0 ? (const uint32_t *)wk.mask.p : sel[f].mask_dst ? sel[f].mask_dst : (const uint32_t *)ctx->temporal.mask[f].p;
    if (!sc.layered) HIPCHK(ctx, hipMemsetAsync(sc.sum, 0, sum_bytes, wk.stream));
    HIPCHK(ctx, hipMemsetAsync(wk.cnt.p, 0, npix * sizeof(int32_t), wk.stream));
    int32_t redo[ML] = {};
    RCCHK(sc.layered ? scale_estimate_layers(ctx, wk, sc, mask, W, H, prm, redo) : scale_estimate(ctx, wk, sc, mask, W, H, prm));
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    temporal_stats_tail(ctx, scale, path);
    for (int k = 0; sc.layered && k < L; ++k) ctx->layer_spectral[scale][k] = redo[k];
    return BCD_HIP_OK;
}

int check_temporal_geometry(bcd_hip_ctx *ctx, int W, int H, int nb_scales, const bcd_hip_params *prm, bool neighbours, const int *sequence_radius)
{
    if (nb_scales < 1 || nb_scales > MAX_SCALES) return bad(ctx, "bad number of scales");
    if (sequence_radius && (*sequence_radius < 1 || *sequence_radius > BCD_HIP_MAX_NEIGHBOURS / 2))
        return bad(ctx, "the temporal radius of a sequence must be 1 or 2 (2 radius <= BCD_HIP_MAX_NEIGHBOURS)");
    if (neighbours && (prm->patch_radius != 1 || prm->search_radius != 6)) {
        set_err(ctx, "neighbour frames are supported with patch radius 1 and search radius 6");
        return BCD_HIP_EUNSUPPORTED;
    }
    for (int s = 1, ws = W, hs = H; s < nb_scales; ++s) {
        ws /= 2; hs /= 2;
        if (ws < 2 * prm->patch_radius + 1 || hs < 2 * prm->patch_radius + 1) return bad(ctx, "too many scales for this image size");
    }
    return BCD_HIP_OK;
}

namespace {

// the refusals of the two frame calls, before any device work
int check_temporal_call(bcd_hip_ctx *ctx, const void *col, const void *ns, const void *hist, const void *cov, const bcd_hip_frame *nb, int n, int W, int H, int D,
                        int nb_scales, const bcd_hip_params *prm, const void *out)
{
    if (n < 0 || n > BCD_HIP_MAX_NEIGHBOURS) return bad(ctx, "the number of neighbour frames must be between 0 and 4 (BCD_HIP_MAX_NEIGHBOURS)");
    if (!col || !ns || !hist || !cov || !out) return bad(ctx, "null image pointer");
    if (n > 0 && !nb) return bad(ctx, "null neighbour list");
    for (int f = 0; f < n; ++f) {
        if (!nb[f].d_colors || !nb[f].d_nsamples || !nb[f].d_histograms || !nb[f].d_covariances) return bad(ctx, "null image pointer in a neighbour frame");
        if (nb[f].reserved) return bad(ctx, "the reserved pointer of a neighbour frame must be NULL");
    }
    RCCHK(check_params(ctx, W, H, D, prm));
    RCCHK(check_temporal_geometry(ctx, W, H, nb_scales, prm, n > 0, nullptr));
    const size_t npix = (size_t)W * H, no = npix * 3 * sizeof(float);
    if (overlaps_frame_images(out, no, col, ns, hist, cov, npix, D)) return bad(ctx, "the output overlaps an input image");
    for (int f = 0; f < n; ++f)
        if (overlaps_frame_images(out, no, nb[f].d_colors, nb[f].d_nsamples, nb[f].d_histograms, nb[f].d_covariances, npix, D))
            return bad(ctx, "the output overlaps an image of a neighbour frame");
    return BCD_HIP_OK;
}

// the checked call with at least one neighbour; motion: null, or per neighbour a device motion field (null: that neighbour is read where it lies)
int temporal_run(bcd_hip_ctx *ctx, const float *d_colors, const float *d_nsamples, const float *d_histograms, const float *d_covariances,
                 const bcd_hip_frame *neighbours, int nb_neighbours, int W, int H, int D, int nb_scales, const bcd_hip_params *prm, float *d_out,
                 const float *const *motion)
{
    DEVICE_GUARD(ctx);
    const int nf = nb_neighbours + 1, S = nb_scales;
    auto &tp = ctx->temporal;
    Work &wk = ctx->main;
    // ---- the pyramids (MultiscaleDenoiser.cpp:41-53) of every frame: level s has the dimensions of level s - 1 halved
    std::vector<TemporalFrame> lv((size_t)S * nf, TemporalFrame());
    auto level = [](const float *col, const float *ns, const float *hist, const float *cov) {
        TemporalFrame l = {};
        l.sel.ns = ns; l.sel.hist = hist; l.col[0] = col; l.cov[0] = cov;
        return l;
    };
    int ws[MAX_SCALES], hs[MAX_SCALES];
    ws[0] = W; hs[0] = H;
    lv[0] = level(d_colors, d_nsamples, d_histograms, d_covariances);
    std::vector<const uint8_t *> valid((size_t)S * nf, nullptr);
    for (int f = 1; f < nf; ++f) {
        const bcd_hip_frame &nb = neighbours[f - 1];
        lv[f] = level(nb.d_colors, nb.d_nsamples, nb.d_histograms, nb.d_covariances);
        if (!motion || !motion[f - 1]) continue;
        // the neighbour reprojected into the frame's pixel grid, at full resolution; its pyramid is built from the warped images
        const float *wp[4];
        RCCHK(temporal_warp_neighbour(ctx, f, nf, nb.d_colors, nb.d_nsamples, nb.d_histograms, nb.d_covariances, motion[f - 1], W, H, D, S, nullptr, 0, valid.data(), wp));
        lv[f] = level(wp[0], wp[1], wp[2], wp[3]);
    }
    for (int s = 1; s < S; ++s) {
        ws[s] = ws[s - 1] / 2; hs[s] = hs[s - 1] / 2;
        const size_t np = (size_t)ws[s] * hs[s];
        RCCHK(ensure(ctx, tp.out[s], np * 3 * sizeof(float)));
        for (int f = 0; f < nf; ++f) {
            DevBuf(&l)[4] = tp.pyr[f][s];
            RCCHK(ensure(ctx, l[0], np * 3 * sizeof(float)));
            RCCHK(ensure(ctx, l[1], np * sizeof(float)));
            RCCHK(ensure(ctx, l[2], np * D * sizeof(float)));
            RCCHK(ensure(ctx, l[3], np * 6 * sizeof(float)));
            lv[(size_t)s * nf + f] = level((const float *)l[0].p, (const float *)l[1].p, (const float *)l[2].p, (const float *)l[3].p);
            RCCHK(temporal_build_level(ctx, lv[(size_t)(s - 1) * nf + f], lv[(size_t)s * nf + f], 1, false, ws[s - 1], hs[s - 1], D, wk.stream));
        }
    }
    for (int s = S - 1; s >= 0; --s) { // coarse to fine; the merge is mergeOutputs (MultiscaleDenoiser.cpp:453-466), as in bcd_hip_denoise
        const size_t npix = (size_t)ws[s] * hs[s];
        TemporalScale sc;
        sc.nf = nf;
        RCCHK(ensure(ctx, wk.sum, npix * 3 * sizeof(float)));
        sc.sum = (float *)wk.sum.p;
        sc.out[0] = s == 0 ? d_out : (float *)tp.out[s].p;
        for (int f = 0; f < nf; ++f) {
            TemporalFrame &fr = sc.fr[f] = lv[(size_t)s * nf + f];
            RCCHK(ensure(ctx, tp.pixcov[f], npix * 6 * sizeof(float)));
            fr.pixcov = (float *)tp.pixcov[f].p;
            fr.sel.valid = valid[(size_t)s * nf + f]; // (null: the frame is not warped -- a warped neighbour's cross masks pass the gate)
            temporal_guide_level(ctx, f, s, &fr.sel);
        }
        RCCHK(temporal_scale(ctx, sc, ws[s], hs[s], D, prm, s));
        if (s < S - 1) RCCHK(bcd_hip_merge(ctx, sc.out[0], ws[s], hs[s], (const float *)tp.out[s + 1].p, 3));
    }
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    return BCD_HIP_OK;
}

// whole uploads of the frame and its neighbours (no streaming) into ctx->temporal.host, and room for the output: dev[0] the frame, dev[1..] the neighbours
int upload_frames(bcd_hip_ctx *ctx, const float *h_colors, const float *h_nsamples, const float *h_histograms, const float *h_covariances, const bcd_hip_frame *neighbours,
                  int nb_neighbours, int W, int H, int D, bcd_hip_frame *dev)
{
    auto &tp = ctx->temporal;
    const size_t npix = (size_t)W * H, bytes[4] = { npix * 3 * sizeof(float), npix * sizeof(float), npix * D * sizeof(float), npix * 6 * sizeof(float) };
    hipStream_t st = ctx->main.stream;
    for (int f = 0; f <= nb_neighbours; ++f) {
        const float *src[4] = { f ? neighbours[f - 1].d_colors : h_colors, f ? neighbours[f - 1].d_nsamples : h_nsamples, f ? neighbours[f - 1].d_histograms : h_histograms,
                                f ? neighbours[f - 1].d_covariances : h_covariances };
        for (int k = 0; k < 4; ++k) {
            RCCHK(ensure(ctx, tp.host[f][k], bytes[k]));
            HIPCHK(ctx, hipMemcpyAsync(tp.host[f][k].p, src[k], bytes[k], hipMemcpyHostToDevice, st));
        }
        dev[f] = { (const float *)tp.host[f][0].p, (const float *)tp.host[f][1].p, (const float *)tp.host[f][2].p, (const float *)tp.host[f][3].p, nullptr };
    }
    RCCHK(ensure(ctx, tp.host_out, bytes[0]));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return BCD_HIP_OK;
}

} // namespace

// whole uploads of the motion fields that are not NULL into ctx->temporal.motion_host: dev[f] the device copy, or NULL
int temporal_upload_motion(bcd_hip_ctx *ctx, const float *const *h_motion, int nb_neighbours, int W, int H, const float **dev)
{
    auto &tp = ctx->temporal;
    const size_t bytes = (size_t)W * H * 2 * sizeof(float);
    for (int f = 0; f < nb_neighbours; ++f) {
        dev[f] = nullptr;
        if (!h_motion[f]) continue;
        RCCHK(ensure(ctx, tp.motion_host[f + 1], bytes));
        HIPCHK(ctx, hipMemcpyAsync(tp.motion_host[f + 1].p, h_motion[f], bytes, hipMemcpyHostToDevice, ctx->main.stream));
        dev[f] = (const float *)tp.motion_host[f + 1].p;
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
    return BCD_HIP_OK;
}

// the checked host call with at least one neighbour: whole uploads, the device call on the copies, the output back; h_motion: null, or the list of a motion call
static int temporal_host_run(bcd_hip_ctx *ctx, const float *h_colors, const float *h_nsamples, const float *h_histograms, const float *h_covariances,
                             const bcd_hip_frame *neighbours, int nb_neighbours, const float *const *h_motion, int W, int H, int D, int nb_scales,
                             const bcd_hip_params *prm, float *h_out)
{
    DEVICE_GUARD(ctx);
    auto &tp = ctx->temporal;
    hipStream_t st = ctx->main.stream;
    bcd_hip_frame dev[BCD_HIP_MAX_NEIGHBOURS + 1];
    const float *dmv[BCD_HIP_MAX_NEIGHBOURS];
    if (h_motion) RCCHK(temporal_upload_motion(ctx, h_motion, nb_neighbours, W, H, dmv));
    RCCHK(upload_frames(ctx, h_colors, h_nsamples, h_histograms, h_covariances, neighbours, nb_neighbours, W, H, D, dev));
    for (int f = 0; tp.prefilter > 0.f && f <= nb_neighbours; ++f) { // ("Prefilter": every frame on its own, in its own pixel grid, in place in its uploaded copies)
        float *col = (float *)tp.host[f][0].p, *cov = (float *)tp.host[f][3].p;
        RCCHK(spike_filter_frame_inplace(ctx, (float *)tp.host[f][1].p, (float *)tp.host[f][2].p, W, H, D, tp.prefilter, &col, &cov, 1, nullptr, nullptr));
    }
    float *d_out = (float *)tp.host_out.p;
    if (h_motion)
        RCCHK(bcd_hip_denoise_temporal_motion(ctx, dev[0].d_colors, dev[0].d_nsamples, dev[0].d_histograms, dev[0].d_covariances, dev + 1, nb_neighbours, dmv, W, H, D,
                                              nb_scales, prm, d_out));
    else
        RCCHK(bcd_hip_denoise_temporal(ctx, dev[0].d_colors, dev[0].d_nsamples, dev[0].d_histograms, dev[0].d_covariances, dev + 1, nb_neighbours, W, H, D, nb_scales, prm, d_out));
    HIPCHK(ctx, hipMemcpyAsync(h_out, d_out, (size_t)W * H * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return BCD_HIP_OK;
}

extern "C" {

int bcd_hip_denoise_temporal(bcd_hip_ctx *ctx, const float *d_colors, const float *d_nsamples, const float *d_histograms, const float *d_covariances,
                             const bcd_hip_frame *neighbours, int nb_neighbours, int W, int H, int D, int nb_scales, const bcd_hip_params *prm, float *d_out)
{
    if (!ctx) return BCD_HIP_EINVAL;
    RCCHK(check_temporal_call(ctx, d_colors, d_nsamples, d_histograms, d_covariances, neighbours, nb_neighbours, W, H, D, nb_scales, prm, d_out));
    if (nb_neighbours == 0) return bcd_hip_denoise(ctx, d_colors, d_nsamples, d_histograms, d_covariances, W, H, D, nb_scales, prm, d_out);
    return temporal_run(ctx, d_colors, d_nsamples, d_histograms, d_covariances, neighbours, nb_neighbours, W, H, D, nb_scales, prm, d_out, nullptr);
}

int bcd_hip_denoise_temporal_host(bcd_hip_ctx *ctx, const float *h_colors, const float *h_nsamples, const float *h_histograms, const float *h_covariances,
                                  const bcd_hip_frame *neighbours, int nb_neighbours, int W, int H, int D, int nb_scales, const bcd_hip_params *prm, float *h_out)
{
    if (!ctx) return BCD_HIP_EINVAL;
    RCCHK(check_temporal_call(ctx, h_colors, h_nsamples, h_histograms, h_covariances, neighbours, nb_neighbours, W, H, D, nb_scales, prm, h_out));
    if (nb_neighbours == 0) return bcd_hip_denoise_host(ctx, h_colors, h_nsamples, h_histograms, h_covariances, W, H, D, nb_scales, prm, h_out);
    return temporal_host_run(ctx, h_colors, h_nsamples, h_histograms, h_covariances, neighbours, nb_neighbours, nullptr, W, H, D, nb_scales, prm, h_out);
}

// ---- the motion calls ("Motion") -------------------------------------------------------------------------------------------
int bcd_hip_denoise_temporal_motion(bcd_hip_ctx *ctx, const float *d_colors, const float *d_nsamples, const float *d_histograms, const float *d_covariances,
                                    const bcd_hip_frame *neighbours, int nb_neighbours, const float *const *d_motion, int W, int H, int D, int nb_scales,
                                    const bcd_hip_params *prm, float *d_out)
{
    if (!ctx) return BCD_HIP_EINVAL;
    RCCHK(check_temporal_call(ctx, d_colors, d_nsamples, d_histograms, d_covariances, neighbours, nb_neighbours, W, H, D, nb_scales, prm, d_out));
    RCCHK(check_motion_list(ctx, d_motion, nb_neighbours, W, H, &d_out, 1));
    if (!any_field(d_motion, nb_neighbours))
        return bcd_hip_denoise_temporal(ctx, d_colors, d_nsamples, d_histograms, d_covariances, neighbours, nb_neighbours, W, H, D, nb_scales, prm, d_out);
    return temporal_run(ctx, d_colors, d_nsamples, d_histograms, d_covariances, neighbours, nb_neighbours, W, H, D, nb_scales, prm, d_out, d_motion);
}

int bcd_hip_denoise_temporal_motion_host(bcd_hip_ctx *ctx, const float *h_colors, const float *h_nsamples, const float *h_histograms, const float *h_covariances,
                                         const bcd_hip_frame *neighbours, int nb_neighbours, const float *const *h_motion, int W, int H, int D, int nb_scales,
                                         const bcd_hip_params *prm, float *h_out)
{
    if (!ctx) return BCD_HIP_EINVAL;
    RCCHK(check_temporal_call(ctx, h_colors, h_nsamples, h_histograms, h_covariances, neighbours, nb_neighbours, W, H, D, nb_scales, prm, h_out));
    RCCHK(check_motion_list(ctx, h_motion, nb_neighbours, W, H, &h_out, 1));
    if (!any_field(h_motion, nb_neighbours))
        return bcd_hip_denoise_temporal_host(ctx, h_colors, h_nsamples, h_histograms, h_covariances, neighbours, nb_neighbours, W, H, D, nb_scales, prm, h_out);
    return temporal_host_run(ctx, h_colors, h_nsamples, h_histograms, h_covariances, neighbours, nb_neighbours, h_motion, W, H, D, nb_scales, prm, h_out);
}

// ---- the stage calls of the motion path
int bcd_hip_warp_frame(bcd_hip_ctx *ctx, const bcd_hip_frame *frame, const float *d_motion, int W, int H, int D, const bcd_hip_warped_frame *out, uint8_t *d_valid)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!frame || !out || !d_valid) return bad(ctx, "null argument");
    if (!frame->d_colors || !frame->d_nsamples || !frame->d_histograms || !frame->d_covariances) return bad(ctx, "null image pointer in the frame");
    if (frame->reserved) return bad(ctx, "the reserved pointer of a frame must be NULL");
    if (!out->d_colors || !out->d_nsamples || !out->d_histograms || !out->d_covariances) return bad(ctx, "null image pointer in the destination");
    bcd_hip_params p; bcd_hip_default_params(&p); p.patch_radius = 0; p.search_radius = 0;
    RCCHK(check_params(ctx, W, H, D, &p));
    {
        const size_t npix = (size_t)W * H, f4 = sizeof(float);
        const void *in[5] = { frame->d_colors, frame->d_nsamples, frame->d_histograms, frame->d_covariances, d_motion };
        const size_t nin[5] = { npix * 3 * f4, npix * f4, npix * D * f4, npix * 6 * f4, npix * 2 * f4 };
        const void *dst[5] = { out->d_colors, out->d_nsamples, out->d_histograms, out->d_covariances, d_valid };
        const size_t ndst[5] = { npix * 3 * f4, npix * f4, npix * D * f4, npix * 6 * f4, npix };
        for (int i = 0; i < 5; ++i) {
            for (int j = 0; j < 5; ++j) if (in[j] && bytes_overlap(dst[i], ndst[i], in[j], nin[j])) return bad(ctx, "a warp destination overlaps an input image or the motion field");
            for (int j = 0; j < i; ++j) if (bytes_overlap(dst[i], ndst[i], dst[j], ndst[j])) return bad(ctx, "two warp destinations overlap");
        }
    }
    DEVICE_GUARD(ctx);
    hipStream_t st = ctx->main.stream;
    HIPCHK(ctx, bcd_launch_warp_frame(frame->d_colors, frame->d_nsamples, frame->d_histograms, frame->d_covariances, d_motion, W, H, D, out->d_colors, out->d_nsamples,
                                      out->d_histograms, out->d_covariances, d_valid, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return BCD_HIP_OK;
}

int bcd_hip_valid_downscale(bcd_hip_ctx *ctx, const uint8_t *d_valid, int W, int H, uint8_t *d_out)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_valid || !d_out) return bad(ctx, "null argument");
    if (W < 2 || H < 2 || (int64_t)W * H >= (1ll << 31)) return bad(ctx, "the validity image must be at least 2 x 2 (and below 2^31 pixels)");
    if (bytes_overlap(d_out, (size_t)(W / 2) * (H / 2), d_valid, (size_t)W * H)) return bad(ctx, "the destination overlaps the input");
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_valid_down(d_valid, W, H, d_out, ctx->main.stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
    return BCD_HIP_OK;
}

int bcd_hip_gate_masks_valid(bcd_hip_ctx *ctx, uint32_t *d_mask, int32_t *d_count, const uint8_t *d_valid, int W, int H, int w, int b)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_mask || !d_count || !d_valid) return bad(ctx, "null argument");
    RCCHK(check_cross_stage(ctx, W, H, 1, w, b));
    {
        const size_t npix = (size_t)W * H, words = ((size_t)(2 * b + 1) * (2 * b + 1) + 31) / 32;
        if (bytes_overlap(d_mask, npix * words * 4, d_count, npix * 4) || bytes_overlap(d_mask, npix * words * 4, d_valid, npix) || bytes_overlap(d_count, npix * 4, d_valid, npix))
            return bad(ctx, "the masks, the counts and the validity image overlap");
    }
    DEVICE_GUARD(ctx);
    RCCHK(temporal_gate(ctx, ctx->main, d_valid, W, H, w, b, d_mask, d_count));
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
    return BCD_HIP_OK;
}

} // extern "C"

// =====================================================================================================================
// "Features" (DESIGN.md section 16): the feature gate of the cross-frame selection.  temporal_select does the gating (above); here are the set-up of a guided
// temporal call and the stage calls.  The frame calls bcd_hip_denoise_temporal_guided[_host] are in bcd_temporal_layers.hip, beside the layered calls they run.
// =====================================================================================================================
int temporal_guide_begin(bcd_hip_ctx *ctx, const bcd_hip_guide *g, const bcd_hip_guide_images *nb, int nb_neighbours, const float *const *motion, int W, int H, int nb_scales)
{
    auto &tp = ctx->temporal;
    hipStream_t st = ctx->main.stream;
    const int F = g->nb_channels;
    const bool var = g->variances != nullptr;
    const size_t npix = (size_t)W * H;
    tp.guide.on = false;
    RCCHK(guide_begin(ctx, g, g->features, g->variances, W, H, nb_scales));
    ctx->guide.on = false; // (no scale of bcd_hip_denoise runs in this call: temporal_select reads the constants and the frame's pyramid)
    for (int s = 0; s < MAX_SCALES; ++s)
        for (int f = 0; f <= BCD_MAX_NEIGHBOURS; ++f) { tp.guide.f[f][s] = f == 0 ? ctx->guide.f[s] : nullptr; tp.guide.v[f][s] = f == 0 ? ctx->guide.v[s] : nullptr; }
    for (int f = 1; f <= nb_neighbours; ++f) {
        const float *feat = nb[f - 1].features, *vv = var ? nb[f - 1].variances : nullptr;
        if (motion && motion[f - 1]) { // gathered by the source pixels and the validity of the neighbour's other images, at full resolution
            DevBuf(&gw)[2] = tp.guide_warp[f];
            RCCHK(ensure(ctx, gw[0], npix * F * sizeof(float)));
            if (var) RCCHK(ensure(ctx, gw[1], npix * F * sizeof(float)));
            RCCHK(ensure(ctx, tp.valid[f][0], npix));
            HIPCHK(ctx, bcd_launch_warp_features(feat, vv, F, motion[f - 1], W, H, (float *)gw[0].p, var ? (float *)gw[1].p : nullptr, (uint8_t *)tp.valid[f][0].p, st));
            feat = (const float *)gw[0].p;
            vv = var ? (const float *)gw[1].p : nullptr;
        }
        tp.guide.f[f][0] = feat; tp.guide.v[f][0] = vv;
        for (int s = 1, ws = W, hs = H; s < nb_scales && s < MAX_SCALES; ++s, ws /= 2, hs /= 2) {
            const size_t np = (size_t)(ws / 2) * (hs / 2);
            DevBuf(&l)[2] = tp.guide_pyr[f][s];
            RCCHK(ensure(ctx, l[0], np * F * sizeof(float)));
            if (var) RCCHK(ensure(ctx, l[1], np * F * sizeof(float)));
            RCCHK(guide_build_level(ctx, tp.guide.f[f][s - 1], tp.guide.v[f][s - 1], ws, hs, F, (float *)l[0].p, (float *)l[1].p, st));
            tp.guide.f[f][s] = (const float *)l[0].p;
            if (var) tp.guide.v[f][s] = (const float *)l[1].p;
        }
    }
    tp.guide.on = true;
    return BCD_HIP_OK;
}

namespace {

// the refusals the two stage calls of the cross feature gate share: the geometry of bcd_hip_similarity_masks_cross, the guide's own rules, the neighbour's images
int check_guide_cross_stage(bcd_hip_ctx *ctx, const bcd_hip_guide *g, const bcd_hip_guide_images *nb, int W, int H, int w, int b)
{
    RCCHK(check_cross_stage(ctx, W, H, BCD_HIP_GUIDE_MAX_CHANNELS, w, b)); // (indices of W*H*F floats stay below 2^31 for every F)
    RCCHK(check_guide(ctx, g, -1));                                        // (-1: the in-frame kernel is not launched)
    if (!nb || !nb->features) return bad(ctx, "null feature image of the neighbour frame");
    if ((g->variances == nullptr) != (nb->variances == nullptr)) return bad(ctx, "feature variances must be given for both frames or for neither");
    if (bcd_pairdist_guide_cross_band(g->nb_channels, g->variances != nullptr, b) < 1) {
        set_err(ctx, "the cross feature distance kernel cannot be launched for this number of channels and search radius (LDS)");
        return BCD_HIP_EUNSUPPORTED;
    }
    return BCD_HIP_OK;
}

} // namespace

extern "C" {

int bcd_hip_similarity_masks_guide_cross(bcd_hip_ctx *ctx, const bcd_hip_guide *guide, const bcd_hip_guide_images *neighbour, int W, int H, int w, int b,
                                         uint32_t *d_mask, int32_t *d_count)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_mask || !d_count) return bad(ctx, "bad argument");
    RCCHK(check_guide_cross_stage(ctx, guide, neighbour, W, H, w, b));
    DEVICE_GUARD(ctx);
    Work &wk = ctx->main;
    RCCHK(temporal_guide_cross_planes(ctx, wk, guide->features, guide->variances, neighbour->features, neighbour->variances, guide->nb_channels, guide->floors, W, H, b));
    HIPCHK(ctx, bcd_launch_masks_cross((const float *)wk.T.p, (const uint8_t *)wk.Cn.p, W, H, w, b, guide->threshold, d_mask, d_count, wk.stream));
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    return BCD_HIP_OK;
}

int bcd_hip_window_distances_guide_cross(bcd_hip_ctx *ctx, const bcd_hip_guide *guide, const bcd_hip_guide_images *neighbour, int W, int H, int w, int b, int line,
                                         int col, float *h_out)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!h_out) return bad(ctx, "bad argument");
    RCCHK(check_guide_cross_stage(ctx, guide, neighbour, W, H, w, b));
    if (line < w || line > H - 1 - w || col < w || col > W - 1 - w) return bad(ctx, "not a main pixel");
    DEVICE_GUARD(ctx);
    Work &wk = ctx->main;
    RCCHK(temporal_guide_cross_planes(ctx, wk, guide->features, guide->variances, neighbour->features, neighbour->variances, guide->nb_channels, guide->floors, W, H, b));
    return window_distances_tail(ctx, wk, W, H, w, b, line, col, h_out);
}

// ---- "Moments": the stage calls of the cross-frame moment selection; what they accept is what bcd_hip_similarity_masks_moments accepts
static int check_moments_cross_stage(bcd_hip_ctx *ctx, int W, int H, int w, int b, float var_floor)
{
    if (!(var_floor >= 0.f) || !std::isfinite(var_floor)) return bad(ctx, "the variance floor must be finite and not negative");
    return check_cross_stage(ctx, W, H, 1, w, b);
}

int bcd_hip_similarity_masks_moments_cross(bcd_hip_ctx *ctx, const float *d_colors, const float *d_pixel_cov, const float *d_colors_nb, const float *d_pixel_cov_nb, int W,
                                           int H, int w, int b, float tau, float var_floor, int form, uint32_t *d_mask_nb, int32_t *d_count_nb)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_colors || !d_pixel_cov || !d_colors_nb || !d_pixel_cov_nb || !d_mask_nb || !d_count_nb) return bad(ctx, "bad argument");
    if (form < 0 || form > 2) return bad(ctx, "the form of the moment cross pass must be 0 (production), 1 (planes) or 2 (fused)");
    RCCHK(check_moments_cross_stage(ctx, W, H, w, b, var_floor));
    if (form == 2 && !bcd_masks_moments_cross_fused_applies(w, b)) {
        set_err(ctx, "the fused moment cross pass serves patch radius 1 and search radius 1 to 6");
        return BCD_HIP_EUNSUPPORTED;
    }
    DEVICE_GUARD(ctx);
    Work &wk = ctx->main;
    RCCHK(temporal_moments_cross_masks(ctx, wk, d_colors, d_pixel_cov, d_colors_nb, d_pixel_cov_nb, W, H, w, b, tau, var_floor, moments_cross_form(form, w, b), d_mask_nb,
                                       d_count_nb));
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    return BCD_HIP_OK;
}

int bcd_hip_window_distances_moments_cross(bcd_hip_ctx *ctx, const float *d_colors, const float *d_pixel_cov, const float *d_colors_nb, const float *d_pixel_cov_nb, int W,
                                           int H, int w, int b, float var_floor, int line, int col, float *h_out)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_colors || !d_pixel_cov || !d_colors_nb || !d_pixel_cov_nb || !h_out) return bad(ctx, "bad argument");
    RCCHK(check_moments_cross_stage(ctx, W, H, w, b, var_floor));
    if (line < w || line > H - 1 - w || col < w || col > W - 1 - w) return bad(ctx, "not a main pixel");
    DEVICE_GUARD(ctx);
    Work &wk = ctx->main;
    RCCHK(temporal_moments_cross_planes(ctx, wk, d_colors, d_pixel_cov, d_colors_nb, d_pixel_cov_nb, W, H, b, var_floor));
    return window_distances_tail(ctx, wk, W, H, w, b, line, col, h_out);
}

int bcd_hip_warp_features(bcd_hip_ctx *ctx, const bcd_hip_guide_images *in, int nb_channels, const float *d_motion, int W, int H, float *d_features_out,
                          float *d_variances_out, uint8_t *d_valid)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!in || !in->features || !d_features_out || !d_valid) return bad(ctx, "null argument");
    if (nb_channels < 1 || nb_channels > BCD_HIP_GUIDE_MAX_CHANNELS) return bad(ctx, "the number of feature channels must be between 1 and 8 (BCD_HIP_GUIDE_MAX_CHANNELS)");
    if ((in->variances == nullptr) != (d_variances_out == nullptr)) return bad(ctx, "a variance destination must be given exactly when there is a variance image");
    bcd_hip_params p; bcd_hip_default_params(&p); p.patch_radius = 0; p.search_radius = 0;
    RCCHK(check_params(ctx, W, H, BCD_HIP_GUIDE_MAX_CHANNELS, &p));
    {
        const size_t npix = (size_t)W * H, nf = npix * nb_channels * sizeof(float);
        const void *src[3] = { in->features, in->variances, d_motion };
        const size_t nsrc[3] = { nf, nf, npix * 2 * sizeof(float) };
        const void *dst[3] = { d_features_out, d_valid, d_variances_out };
        const size_t ndst[3] = { nf, npix, nf };
        for (int i = 0; i < 3; ++i) {
            if (!dst[i]) continue;
            for (int j = 0; j < 3; ++j) if (src[j] && bytes_overlap(dst[i], ndst[i], src[j], nsrc[j])) return bad(ctx, "a warp destination overlaps an input image or the motion field");
            for (int j = 0; j < i; ++j) if (bytes_overlap(dst[i], ndst[i], dst[j], ndst[j])) return bad(ctx, "two warp destinations overlap");
        }
    }
    DEVICE_GUARD(ctx);
    hipStream_t st = ctx->main.stream;
    HIPCHK(ctx, bcd_launch_warp_features(in->features, in->variances, nb_channels, d_motion, W, H, d_features_out, d_variances_out, d_valid, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return BCD_HIP_OK;
}

} // extern "C"
