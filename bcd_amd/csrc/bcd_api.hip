// bcd_api.hip -- implementation of the C ABI declared in include/bcd_hip.h: context, workspace,
// the per-scale driver (Denoiser::denoise, src/core/Denoiser.cpp:84-212) and the multiscale driver
// (MultiscaleDenoiser::denoise, src/core/MultiscaleDenoiser.cpp:31-136) on device-resident images, and the stage-level entry points.
// The host-buffer entry points are in bcd_host.hip, the sample accumulator in bcd_accum.hip, a frame's kept selection in bcd_selection.hip, the self-tests in
// bcd_selftest.hip.
#include "bcd_ctx.h"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <new>
#include <thread>
#include <string>
#include <utility>
#include <vector>

// ---- helpers shared with the other host files (declared in bcd_ctx.h) ----------------------------------------------------------------
void set_err(bcd_hip_ctx *ctx, const std::string &msg)
{
    if (!ctx) return;
    std::lock_guard<std::mutex> lock(ctx->err_mutex);
    ctx->err = msg;
}

int ensure(bcd_hip_ctx *ctx, DevBuf &b, size_t bytes)
{
    if (b.bytes >= bytes && b.p) return BCD_HIP_OK;
    if (b.p) { HIPCHK(ctx, hipFree(b.p)); b.p = nullptr; b.bytes = 0; }
    size_t want = bytes + bytes / 16 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) { set_err(ctx, "hipMalloc failed: " + std::string(hipGetErrorString(e))); b.p = nullptr; return BCD_HIP_ENOMEM; }
    b.bytes = want;
    return BCD_HIP_OK;
}

int bad(bcd_hip_ctx *ctx, const char *msg)
{
    set_err(ctx, msg);
    return BCD_HIP_EINVAL;
}

int check_params(bcd_hip_ctx *ctx, int W, int H, int D, const bcd_hip_params *prm)
{
    if (!prm) return bad(ctx, "null parameters");
    if (W <= 0 || H <= 0 || D <= 0) return bad(ctx, "empty input image");            // Denoiser.cpp:294-320
    if (prm->patch_radius < 0 || prm->search_radius < 0) return bad(ctx, "negative radius");
    if (W < 2 * prm->patch_radius + 1 || H < 2 * prm->patch_radius + 1) return bad(ctx, "image smaller than a patch");
    if (D > 255) { set_err(ctx, "histogram depth > 255 is not supported"); return BCD_HIP_EUNSUPPORTED; }
    int side = 2 * prm->search_radius + 1;
    if ((side * side + 31) / 32 > 32) { set_err(ctx, "search radius > 15 is not supported"); return BCD_HIP_EUNSUPPORTED; }
    if (bcd_bayes_lds_bytes(prm->patch_radius, prm->search_radius) > 160 * 1024) {
        set_err(ctx, "patch/search radius combination exceeds the 160 KiB LDS working set");
        return BCD_HIP_EUNSUPPORTED;
    }
    if ((int64_t)W * H >= (1ll << 31) / (D > 6 ? D : 6)) return bad(ctx, "image too large for 32-bit DeepImage indices");
    if (prm->use_random_pixel_order < 0 || prm->use_random_pixel_order > 2) return bad(ctx, "pixel order must be 0 (scanline), 1 (seeded random) or 2 (strips)");
    if (prm->use_random_pixel_order == 2 && (W > 8191 || H > 8191 || prm->patch_radius > 3 || prm->search_radius < 1))
        return bad(ctx, "the strip order supports frames up to 8191 x 8191, patch radius <= 3, search radius >= 1");
    return BCD_HIP_OK;
}

// can the approximate-planes path serve this problem?  (w = 1, a supported depth, a threshold binary16 can decide: bcd_common.h)
bool fast_similarity_applies(const bcd_hip_ctx *ctx, int D, int w, float tau)
{
    return ctx->fast_similarity && w == 1 && bcd_pairdist_rw_supported(D) && tau >= BCD_APPROX_TAU_MIN && tau <= BCD_APPROX_TAU_MAX;
}

// one small reduction and one host round trip (~30 us): *uni_n = the frame's power-of-two sample count, or left as it is when the frame has none
int scan_uniform_count(bcd_hip_ctx *ctx, Work &wk, const float *d_ns, size_t npix, float *uni_n)
{
    Counters *d = wk.d_counters(), *h = wk.h_counters;
    HIPCHK(ctx, bcd_launch_uniform_n(d_ns, (int64_t)npix, &d->flags.scan, wk.stream));
    HIPCHK(ctx, hipMemcpyAsync(&h->flags.scan, &d->flags.scan, sizeof(int), hipMemcpyDeviceToHost, wk.stream));
    HIPCHK(ctx, hipMemcpyAsync(&h->first_count, d_ns, sizeof(float), hipMemcpyDeviceToHost, wk.stream));
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    if (h->flags.scan == 0 && is_pow2_sample_count(h->first_count)) *uni_n = h->first_count;
    return BCD_HIP_OK;
}

float stage_ms(Work &wk, int a, int b)
{
    float ms = 0.f;
    hipEventElapsedTime(&ms, wk.ev_stage[a], wk.ev_stage[b]);
    return ms;
}

namespace {

// `share` of the frame's work (pixels of a scale, weighted) is done
void progress_add(bcd_hip_ctx *ctx, double share)
{
    if (!ctx->progress_fn || !(ctx->progress_total > 0.0)) return;
    std::lock_guard<std::mutex> lock(ctx->progress_mutex);
    ctx->progress_done = std::min(ctx->progress_total, ctx->progress_done + share);
    ctx->progress_fn((float)(ctx->progress_done / ctx->progress_total), ctx->progress_user);
}

// The estimate kernels are persistent (a wavefront per CU slot, items from a counter), so whatever they occupy stays
// occupied until they end.  In a multiscale call the finest scale is the critical path and the coarse scales have slack: they
// take a quarter of the slots, which leaves LDS and wave slots on every CU to the finest scale's short kernels (masks,
// marking, lists) running beside them -- measured 1080p: 306 -> 315 Mpix/s (100 % -> 25 %; 12 %: 320, 6 %: 250).  The share is
// ctx->coarse_share: 25 on a new geometry, then steered by bcd_hip_denoise.
int estimate_cus(const bcd_hip_ctx *ctx, const Work &wk)
{
    int cus = std::max(1, ctx->num_cus * ctx->cu_share_pct / 100);
    if (&wk != &ctx->main) cus = std::max(1, cus * ctx->coarse_share / 100);
    return cus;
}

// ... the same share as a percentage of the chip (bcd_hip_scale_stats::cu_share)
int estimate_share_pct(const bcd_hip_ctx *ctx, const Work &wk) { return ctx->cu_share_pct * (&wk != &ctx->main ? ctx->coarse_share : 100) / 100; }

} // namespace

// what follows on the workspace's side stream comes after what the scale's own stream holds so far (shared with bcd_temporal_layers.hip)
int fork_aux(bcd_hip_ctx *ctx, Work &wk)
{
    HIPCHK(ctx, hipEventRecord(wk.ev_fork, wk.stream));
    HIPCHK(ctx, hipStreamWaitEvent(wk.aux, wk.ev_fork, 0));
    return BCD_HIP_OK;
}

namespace {

// did the last similarity() pass on this workspace leave the range flag raised or overflow its borderline list?  (valid after the
// stream has been synchronised; the caller then repeats the pass with exact_mode = 1)
bool similarity_needs_redo(const Work &wk)
{
    const Counters::Flags &f = wk.h_counters->flags;
    return f.range != 0 || (wk.border_capacity > 0 && (f.other_count != 0 || f.borderline > wk.border_capacity));
}

// ... and with which kernels: 0 = no redo; 3 = the approximate kernels again with the general (non-uniform) formula -- the only complaint
// was that the sample counts are not one power of two (flag bit 1 of k_pairdist_rw); 1 = the exact kernels.  Also keeps the workspace's
// memory of whether its frames have uniform counts (valid after the stream has been synchronised).
int similarity_redo_mode(Work &wk)
{
    const int flag = wk.h_counters->flags.range;
    const bool fast = wk.border_capacity > 0;
    const bool other_count = fast && wk.h_counters->flags.other_count != 0; // a pixel carries another sample count than the uniform kernel was launched for
    const bool overflow = fast && wk.h_counters->flags.borderline > wk.border_capacity;
    if (fast && (wk.speculated || other_count)) wk.nonuniform = other_count;
    if (flag == 0 && !other_count && !overflow) return 0;
    if (fast && wk.ratio_used && (flag & 4) != 0) { // the RATIO form's absolute-error check: the reference's operations serve this frame size on this workspace from now on
        if (!wk.ratio_is_declined(wk.ratio_W, wk.ratio_H)) { wk.ratio_declined[wk.ratio_declined_next] = { wk.ratio_W, wk.ratio_H }; wk.ratio_declined_next = (wk.ratio_declined_next + 1) & 3; }
        if ((flag & ~4) == 0) return 3;
    }
    return (flag == 0 && other_count) ? 3 : 1; // (a void launch has no meaningful list count: other_count alone decides)
}

// an event pair around the distance kernel of a similarity pass (bcd_hip_kernel_time); both stay null once MAX_EVENT_PAIRS are in use
int timing_events(bcd_hip_ctx *ctx, Work &wk, hipEvent_t *e0, hipEvent_t *e1)
{
    *e0 = *e1 = nullptr;
    if (wk.ev_used >= MAX_EVENT_PAIRS) return BCD_HIP_OK;
    if (wk.ev_used == (int)wk.ev_pool.size()) {
        hipEvent_t a, c;
        HIPCHK(ctx, hipEventCreate(&a));
        HIPCHK(ctx, hipEventCreate(&c));
        wk.ev_pool.emplace_back(a, c);
    }
    *e0 = wk.ev_pool[wk.ev_used].first;
    *e1 = wk.ev_pool[wk.ev_used].second;
    ++wk.ev_used;
    return BCD_HIP_OK;
}

// exact_mode: 0 = production kernels, flags checked here (one stream synchronisation); 1 = exact kernels with the compiler's division;
// 2 = production kernels, flags copied to wk.h_counters->flags but NOT checked: the caller validates after its own
// synchronisation with similarity_needs_redo() / similarity_redo_mode(); 3 = like 2 with the general (non-uniform) formula forced.
// Production kernels: w = 1 and a supported depth -> approximate planes (k_pairdist_rw) + exact verification of the borderline
// pairs; otherwise the exact planes with the scale-free division (k_pairdist<FAST>).
int similarity(bcd_hip_ctx *ctx, Work &wk, const float *d_hist, const float *d_ns, int W, int H, int D, int w, int b, float tau,
               uint32_t *d_mask, int32_t *d_count, int exact_mode = 0)
{
    const size_t npix = (size_t)W * H;
    const int nd = bcd_delta_count(b);
    // the approximate path keeps binary16 planes -- one margin plane, or (the RATIO form, BCD_HIP_TC_PLANES=1) T and counts --, the exact kernels fp32 T and counts
    const bool fast_path = exact_mode != 1 && fast_similarity_applies(ctx, D, w, tau);
    const bool margin_wanted = fast_path && ctx->margin_planes;
    RCCHK(ensure(ctx, wk.T, fast_path ? half_plane_bytes(npix, nd) : npix * nd * sizeof(float)));
    RCCHK(ensure(ctx, wk.Cn, count_plane_bytes(npix, nd)));
    RCCHK(ensure(ctx, wk.fwd, npix * ((nd + 31) / 32) * sizeof(uint32_t)));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    RCCHK(timing_events(ctx, wk, &e0, &e1));
    RCCHK(ensure(ctx, wk.counters, sizeof(Counters)));
    Counters::Flags *d_flag = &wk.d_counters()->flags, *h_flag = &wk.h_counters->flags;
    // planes of exactly this problem already computed by the caller (its launches raised the flags in d_flag[0] themselves)?
    const bool pre = wk.planes.ready && exact_mode != 1 && wk.planes.hist == d_hist && wk.planes.ns == d_ns && wk.planes.W == W && wk.planes.H == H &&
                     wk.planes.D == D && wk.planes.b == b && wk.planes.tau == tau && wk.planes.margin == (margin_wanted && !wk.planes.ratio) && w == 1;
    const bool planes_kept = wk.planes.ready; // (k_scale_begin kept words [0] and [2] for the launches that made them)
    wk.planes.ready = false;
    if (wk.clean_flags) { // cleared by k_scale_begin, which kept the words of planes computed ahead ...
        wk.clean_flags = false;
        if (planes_kept && !pre) { // ... of ANOTHER problem (serialised scales: the coarsest scale runs first on this workspace): their flags are not this pass's
            HIPCHK(ctx, hipMemsetAsync(&d_flag->range, 0, sizeof(int), wk.stream));
            HIPCHK(ctx, hipMemsetAsync(&d_flag->other_count, 0, sizeof(int), wk.stream));
        }
    } else if (pre) { // (flags [0] and [2] belong to the launches that made the planes)
        HIPCHK(ctx, hipMemsetAsync(&d_flag->scan, 0, sizeof(int), wk.stream));
        HIPCHK(ctx, hipMemsetAsync(&d_flag->borderline, 0, sizeof(int), wk.stream));
    } else HIPCHK(ctx, hipMemsetAsync(d_flag, 0, sizeof(*d_flag), wk.stream));
    h_flag->range = 0;
    h_flag->other_count = 0;
    h_flag->borderline = 0;
    wk.border_capacity = 0;
    wk.ratio_used = false;
    wk.ratio_W = W; wk.ratio_H = H;
    // fixed samples per pixel, a power of two (the usual case): the distance kernel drops the sample-count products (exactly,
    // see k_pairdist).  One small reduction and one host round trip at the head of the chain (~30 us).
    float uni_n = pre ? wk.planes.uni_n : 0.f;
    wk.speculated = false;
    if (fast_path && !pre) {
        // No scan and no round trip at the head of the chain: the approximate kernel takes the first pixel's count as THE count and checks
        // every pixel against it itself (flag bit 1 -> the pass is repeated with the general formula).  A workspace whose LAST frame was not
        // uniform (adaptive sampling) looks first (round 5: it used to take the general formula blindly and look again every 32nd pass, which
        // cost a uniform frame that followed frames with mixed counts the general formula for up to 31 passes).
        if (exact_mode != 3 && !wk.nonuniform) { uni_n = -1.f; wk.speculated = true; }
        else if (exact_mode != 3) {
            RCCHK(scan_uniform_count(ctx, wk, d_ns, npix, &uni_n));
            wk.nonuniform = uni_n == 0.f;
        }
    } else if (exact_mode != 1 && !pre)
        RCCHK(scan_uniform_count(ctx, wk, d_ns, npix, &uni_n));
    // the approximate path keeps its T plane in binary16: thresholds it cannot decide safely take the exact kernels (bcd_common.h)
    const bool fast = fast_path;
    if (fast) {
        const int capacity = (int)std::min<size_t>(std::max<size_t>(npix, 1u << 16), 1u << 28);
        RCCHK(ensure(ctx, wk.border, (size_t)capacity * sizeof(uint2)));
        wk.border_capacity = capacity;
        BcdBorderline bl = { 0.f, (uint2 *)wk.border.p, &d_flag->borderline, capacity, 0.f, 0.f };
        // General sample counts (adaptive sampling, 24 spp, ...; src/core/DenoisingUnit.cpp:371-383 handles any n1, n2): the RATIO form of the dense kernel
        // (round 6, k_similarity_fast.hip) evaluates them at the cost of uniform ones -- 1.83 ms at 1080p against 1.73 for the uniform kernel, 3.0 ms for the
        // reference's operations and 1.97 + 0.07 ms for the own-list kernel of round 5, which it replaced -- and checks afterwards that the absolute errors it
        // adds stay inside the verified band (flag bit 2: the pass is then repeated with the reference's operations, and the workspace remembers the size).
        const bool use_ratio = !pre && uni_n == 0.f && !wk.ratio_is_declined(W, H);
        wk.ratio_used = pre ? wk.planes.ratio : use_ratio; // (planes computed ahead: the form their launches took; its verdict is in flag word [0])
        const bool margin = margin_wanted && !wk.ratio_used; // (the RATIO form's absolute error is per counted bin: it keeps T / C planes)
        const float margin_tau = margin ? tau : 0.f;
        if (pre) { if (e0) --wk.ev_used; } // (nothing to time: the planes are there)
        else if (use_ratio) {
            RCCHK(ensure(ctx, wk.ratio_stats, 128 * sizeof(unsigned int)));
            if (e0) HIPCHK(ctx, hipEventRecord(e0, wk.stream));
            HIPCHK(ctx, bcd_launch_pairdist_rw_ratio(d_hist, d_ns, W, H, D, b, wk.T.p, (uint8_t *)wk.Cn.p, &d_flag->range, tau, (unsigned int *)wk.ratio_stats.p, wk.stream));
            if (e1) HIPCHK(ctx, hipEventRecord(e1, wk.stream));
        } else {
            if (e0) HIPCHK(ctx, hipEventRecord(e0, wk.stream));
            HIPCHK(ctx, bcd_launch_pairdist_rw(d_hist, d_ns, W, H, D, b, wk.T.p, (uint8_t *)wk.Cn.p, &d_flag->range, uni_n, wk.stream, margin_tau));
            if (e1) HIPCHK(ctx, hipEventRecord(e1, wk.stream));
        }
        if (margin) bcd_margin_band(D, tau, &bl.band_rel, &bl.band_abs);
        HIPCHK(ctx, hipMemcpyAsync(&h_flag->range, &d_flag->range, sizeof(int), hipMemcpyDeviceToHost, wk.stream));
        HIPCHK(ctx, hipMemcpyAsync(&h_flag->other_count, &d_flag->other_count, sizeof(int), hipMemcpyDeviceToHost, wk.stream)); // "another sample count" (plain-store flag)
        HIPCHK(ctx, bcd_launch_masks((const float *)wk.T.p, (const uint8_t *)wk.Cn.p, W, H, w, b, tau, d_mask, d_count, (uint32_t *)wk.fwd.p, wk.stream,
                                     &bl, d_hist, d_ns, D));
        HIPCHK(ctx, hipMemcpyAsync(&h_flag->borderline, &d_flag->borderline, sizeof(int), hipMemcpyDeviceToHost, wk.stream));
        if (exact_mode == 0) {
            HIPCHK(ctx, hipStreamSynchronize(wk.stream));
            const int redo = similarity_redo_mode(wk);
            if (redo == 3) {
                RCCHK(similarity(ctx, wk, d_hist, d_ns, W, H, D, w, b, tau, d_mask, d_count, 3));
                HIPCHK(ctx, hipStreamSynchronize(wk.stream));
                if (similarity_needs_redo(wk) && similarity_redo_mode(wk) == 3) { // (the RATIO form declined: once more with the reference's operations)
                    RCCHK(similarity(ctx, wk, d_hist, d_ns, W, H, D, w, b, tau, d_mask, d_count, 3));
                    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
                }
                if (similarity_needs_redo(wk)) return similarity(ctx, wk, d_hist, d_ns, W, H, D, w, b, tau, d_mask, d_count, 1);
            } else if (redo == 1)
                return similarity(ctx, wk, d_hist, d_ns, W, H, D, w, b, tau, d_mask, d_count, 1);
        }
        return BCD_HIP_OK;
    }
    if (e0) HIPCHK(ctx, hipEventRecord(e0, wk.stream));
    HIPCHK(ctx, bcd_launch_pairdist(d_hist, d_ns, W, H, D, b, (float *)wk.T.p, (uint8_t *)wk.Cn.p, exact_mode == 1 ? 0 : 1, &d_flag->range, uni_n, wk.stream));
    if (e1) HIPCHK(ctx, hipEventRecord(e1, wk.stream));
    // the fast kernel flags inputs outside the range where its division is proven exact: redo with the compiler's division
    if (exact_mode != 1) HIPCHK(ctx, hipMemcpyAsync(&h_flag->range, &d_flag->range, sizeof(int), hipMemcpyDeviceToHost, wk.stream));
    if (exact_mode == 0) {
        HIPCHK(ctx, hipStreamSynchronize(wk.stream));
        if (h_flag->range != 0)
            HIPCHK(ctx, bcd_launch_pairdist(d_hist, d_ns, W, H, D, b, (float *)wk.T.p, (uint8_t *)wk.Cn.p, 0, &d_flag->range, 0.f, wk.stream));
    }
    HIPCHK(ctx, bcd_launch_masks((const float *)wk.T.p, (const uint8_t *)wk.Cn.p, W, H, w, b, tau, d_mask, d_count, (uint32_t *)wk.fwd.p, wk.stream,
                                 nullptr, nullptr, nullptr, 0));
    return BCD_HIP_OK;
}

// The selection from means and covariances: the exact-path planes from the guide's colours and per-pixel covariances
// (k_pairdist_moments), then the mask kernels of the exact histogram pass.  No flag is raised and nothing is ever redone: the pass enters
// mono_accumulate's loop the way similarity(..., exact_mode = 1) does.  d_pixcov must be complete on wk.stream (a frame: wk.ev_pixcov).
int similarity_moments(bcd_hip_ctx *ctx, Work &wk, const float *d_colors, const float *d_pixcov, int W, int H, int w, int b, float tau, float var_floor,
                       uint32_t *d_mask, int32_t *d_count)
{
    const size_t npix = (size_t)W * H;
    const int nd = bcd_delta_count(b);
    RCCHK(ensure(ctx, wk.T, npix * nd * sizeof(float)));
    RCCHK(ensure(ctx, wk.Cn, count_plane_bytes(npix, nd)));
    RCCHK(ensure(ctx, wk.fwd, npix * ((nd + 31) / 32) * sizeof(uint32_t)));
    RCCHK(ensure(ctx, wk.counters, sizeof(Counters)));
    // the planes of the workspace are this pass's from here on: planes a host-stream caller computed ahead are gone, and these are never noted as ready
    wk.planes.ready = false;
    wk.clean_flags = false; // (no flag word is used: the next histogram pass clears its own)
    Counters::Flags *h_flag = &wk.h_counters->flags;
    h_flag->range = 0;
    h_flag->other_count = 0;
    h_flag->borderline = 0;
    wk.border_capacity = 0;
    wk.ratio_used = false;
    wk.speculated = false;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    RCCHK(timing_events(ctx, wk, &e0, &e1));
    if (e0) HIPCHK(ctx, hipEventRecord(e0, wk.stream));
    HIPCHK(ctx, bcd_launch_pairdist_moments(d_colors, d_pixcov, W, H, b, var_floor, (float *)wk.T.p, (uint8_t *)wk.Cn.p, wk.stream));
    if (e1) HIPCHK(ctx, hipEventRecord(e1, wk.stream));
    HIPCHK(ctx, bcd_launch_masks((const float *)wk.T.p, (const uint8_t *)wk.Cn.p, W, H, w, b, tau, d_mask, d_count, (uint32_t *)wk.fwd.p, wk.stream,
                                 nullptr, nullptr, nullptr, 0));
    return BCD_HIP_OK;
}

// The feature masks of a guide: the exact-path planes from the features and their variances (k_pairdist_guide), the mask kernels
// of the exact histogram pass into d_gate / d_gate_count.  Nothing of the workspace's verdict on a preceding selection pass is touched: no flag word is
// used, the host mirror of the flags and the borderline capacity stay what that pass left.  The planes and the forward-mask scratch of the workspace are
// reused -- the selection pass that precedes is complete in stream order, a redo recomputes its own planes --, so planes computed ahead are gone.
int guide_masks(bcd_hip_ctx *ctx, Work &wk, const float *d_features, const float *d_variances, int F, const float *floors, float tau_g, int W, int H, int w, int b,
                uint32_t *d_gate, int32_t *d_gate_count)
{
    const size_t npix = (size_t)W * H;
    const int nd = bcd_delta_count(b);
    RCCHK(ensure(ctx, wk.T, npix * nd * sizeof(float)));
    RCCHK(ensure(ctx, wk.Cn, count_plane_bytes(npix, nd)));
    RCCHK(ensure(ctx, wk.fwd, npix * ((nd + 31) / 32) * sizeof(uint32_t)));
    wk.planes.ready = false;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    RCCHK(timing_events(ctx, wk, &e0, &e1));
    if (e0) HIPCHK(ctx, hipEventRecord(e0, wk.stream));
    HIPCHK(ctx, bcd_launch_pairdist_guide(d_features, d_variances, F, floors, W, H, b, (float *)wk.T.p, (uint8_t *)wk.Cn.p, wk.stream));
    if (e1) HIPCHK(ctx, hipEventRecord(e1, wk.stream));
    HIPCHK(ctx, bcd_launch_masks((const float *)wk.T.p, (const uint8_t *)wk.Cn.p, W, H, w, b, tau_g, d_gate, d_gate_count, (uint32_t *)wk.fwd.p, wk.stream,
                                 nullptr, nullptr, nullptr, 0));
    return BCD_HIP_OK;
}

// The gate of a guided selection: mask = selection mask AND feature mask, |S| = popcount, behind a selection pass on wk.stream.  A pure AND: no special
// case for the centre bit, nothing else of the selection changes.
int guide_gate(bcd_hip_ctx *ctx, Work &wk, const float *d_features, const float *d_variances, int W, int H, int w, int b, uint32_t *d_mask, int32_t *d_count)
{
    const size_t npix = (size_t)W * H;
    const int side = 2 * b + 1, words = (side * side + 31) / 32;
    RCCHK(ensure(ctx, wk.gate_mask, npix * words * sizeof(uint32_t)));
    RCCHK(ensure(ctx, wk.gate_nsim, npix * sizeof(int32_t)));
    RCCHK(guide_masks(ctx, wk, d_features, d_variances, ctx->guide.F, ctx->guide.floors, ctx->guide.tau, W, H, w, b, (uint32_t *)wk.gate_mask.p, (int32_t *)wk.gate_nsim.p));
    HIPCHK(ctx, bcd_launch_gate_masks(d_mask, (const uint32_t *)wk.gate_mask.p, d_count, W, H, b, wk.stream));
    return BCD_HIP_OK;
}

// one batch of marking launches on lines [row_begin, row_end); *undecided_out = pixels of those lines still undecided
// Two halves (round 6): active_step_enqueue launches the batch and the copy of its counters WITHOUT waiting -- with `d_total` it also leaves the rank's
// contribution to the all-reduced count on the device (k_sum_counter_lines; `with_verdict`: + 2^40 when this workspace's last similarity pass has to be
// repeated), so that the band driver's all-reduce follows in stream order and one synchronisation serves both; active_step_collect reads the counters
// after the caller's synchronisation.
int active_step_enqueue(bcd_hip_ctx *ctx, Work &wk, const uint32_t *d_mask, const int32_t *d_nsim, int W, int H, int w, int b, int row_begin,
                        int row_end, int random_order, uint32_t seed, int row_offset, uint8_t *d_state, long long *d_total, bool with_verdict)
{
    const int K = 3 * (2 * w + 1) * (2 * w + 1);
    RCCHK(ensure(ctx, wk.counters, sizeof(Counters)));
    int *d_cnt = wk.d_counters()->undecided;
    // every launch counts the pixels it leaves undecided into its own set of BCD_CNT_LINES sub-counters (one per cache line: a single
    // counter is a serial resource, k_active.hip); one small kernel folds them into d_cnt[launch] for the host
    constexpr size_t LINE_INTS = (size_t)BCD_CNT_LINES * BCD_CNT_STRIDE;
    RCCHK(ensure(ctx, wk.cnt_lines, ROUND_BATCH * LINE_INTS * sizeof(int)));
    int *d_lines = (int *)wk.cnt_lines.p;
    if (wk.clean_lines) wk.clean_lines = false; // (k_scale_begin)
    else {
        HIPCHK(ctx, hipMemsetAsync(d_lines, 0, ROUND_BATCH * LINE_INTS * sizeof(int), wk.stream));
        HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, ROUND_BATCH * sizeof(int), wk.stream));
    }
    // b = 6 / 12: dependency lists extracted once per marking problem, then cheap tile rounds (in-tile chains are resolved
    // inside a launch: few launches for a random order, more for the long chains of the scanline order);
    // other radii: the generic one-level-per-launch kernel
    const bool listed = (b == 6 || b == 12);
    int batch = 4;
    if (listed) {
        const int side = 2 * b + 1, words = (side * side + 31) / 32;
        const int iters = 8; // in-tile iterations per launch
        int i = 0;
        batch = random_order == 1 ? 3 : ROUND_BATCH;
        if (wk.dep_ready && (wk.dep_mask != (const void *)d_mask || wk.dep_state != (const void *)d_state)) wk.dep_ready = false;
        if (!wk.dep_ready) {
            RCCHK(ensure(ctx, wk.dep, (size_t)W * H * words * sizeof(uint32_t)));
            HIPCHK(ctx, bcd_launch_mark_deps(d_mask, d_nsim, d_state, (uint32_t *)wk.dep.p, W, H, b, K + 1, random_order, seed,
                                             row_begin, row_end, row_offset, d_lines + LINE_INTS * i++, wk.stream));
            wk.dep_ready = true;
            wk.dep_mask = d_mask;
            wk.dep_state = d_state;
            // first batch: what the previous marking problem of this workspace needed, plus one (frames of a sequence and
            // the bands of a frame behave alike), so that the usual case costs a single host round trip
            if (random_order == 1) batch = std::min(ROUND_BATCH, std::max(5, wk.rounds_hint + 1));
        }
        for (; i < batch; ++i)
            HIPCHK(ctx, bcd_launch_mark_round((const uint32_t *)wk.dep.p, d_state, W, H, b, row_begin, row_end, iters, d_lines + LINE_INTS * i, wk.stream));
    } else {
        for (int i = 0; i < batch; ++i)
            HIPCHK(ctx, bcd_launch_active_round(d_mask, d_nsim, d_state, W, H, b, K + 1, random_order, seed, row_begin, row_end, row_offset,
                                                d_lines + LINE_INTS * i, wk.stream));
    }
    HIPCHK(ctx, bcd_launch_sum_counter_lines(d_lines, batch, d_cnt, wk.stream, d_total, with_verdict ? &wk.d_counters()->flags.range : nullptr, wk.border_capacity));
    HIPCHK(ctx, hipMemcpyAsync(wk.h_counters->undecided, d_cnt, ROUND_BATCH * sizeof(int), hipMemcpyDeviceToHost, wk.stream));
    wk.last_batch = batch;
    return BCD_HIP_OK;
}

void active_step_collect(Work &wk, int *undecided_out, int *launches_out)
{
    const int batch = wk.last_batch;
    int n = batch;
    for (int i = 0; i < batch; ++i)
        if (wk.h_counters->undecided[i] == 0) { n = i + 1; break; }
    *undecided_out = wk.h_counters->undecided[n - 1];
    if (launches_out) *launches_out = n;
}

// one batch of marking launches on lines [row_begin, row_end); *undecided_out = pixels of those lines still undecided
int active_step(bcd_hip_ctx *ctx, Work &wk, const uint32_t *d_mask, const int32_t *d_nsim, int W, int H, int w, int b, int row_begin,
                int row_end, int random_order, uint32_t seed, int row_offset, bool first_pass, uint8_t *d_state, int *undecided_out,
                int *launches_out)
{
    (void)first_pass; // a hint of the C ABI ("every pixel is still undecided"); the dependency-list kernels do not need it
    RCCHK(active_step_enqueue(ctx, wk, d_mask, d_nsim, W, H, w, b, row_begin, row_end, random_order, seed, row_offset, d_state, nullptr, false));
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    active_step_collect(wk, undecided_out, launches_out);
    return BCD_HIP_OK;
}

int active_set(bcd_hip_ctx *ctx, Work &wk, const uint32_t *d_mask, const int32_t *d_nsim, int W, int H, int w, int b, int row_begin,
               int row_end, float skip_prob, int random_order, uint32_t seed, uint8_t *d_state, int32_t *rounds_out)
{
    HIPCHK(ctx, bcd_launch_active_init(d_nsim, W, H, w, row_begin, row_end, skip_prob, seed, 0, d_state, wk.stream));
    wk.dep_ready = false;
    int rounds = 0;
    if (skip_prob > 0.f) {
        // every launch decides at least the earliest undecided pixel of the visiting order, so the iteration ends after at most
        // (number of main pixels) launches; stop only when a whole batch makes no progress (which would be an engine bug)
        int undecided = 1, before = INT_MAX;
        while (undecided != 0) {
            int n = 0;
            // (strip order: the key needs the frame's geometry, which travels in the seed argument; the skip draws keep the caller's seed)
            const uint32_t key_seed = random_order == 2 ? bcd_strip_order_seed(W, H, w, b) : seed;
            RCCHK(active_step(ctx, wk, d_mask, d_nsim, W, H, w, b, row_begin, row_end, random_order, key_seed, 0, rounds == 0 && skip_prob >= 1.f,
                              d_state, &undecided, &n));
            rounds += n;
            if (undecided != 0 && undecided >= before) { set_err(ctx, "marking fixed point made no progress"); return BCD_HIP_EDEVICE; }
            before = undecided;
        }
        wk.rounds_hint = rounds;
    }
    if (rounds_out) *rounds_out = rounds;
    return BCD_HIP_OK;
}

// lists of processed pixels + the estimate kernels.  The list lengths and the sum of |S| are copied to wk.h_counters->lists:
// read them with bayes_counts() after the stream has been synchronised.
// w = 1: the full estimate is three kernels with a per-pixel record in HBM between them (k_bayes27.hip); the host reads the
// number of full-estimate pixels (one short round trip, the fallback kernel is already running on its side stream) to size the
// record buffer and to cut very long lists (-m 0) into chunks.  Other patch radii: one persistent kernel, no round trip.
// Only processed pixels of lines [row_begin, row_end) are listed / estimated (a row band's owned lines: the states of its halo lines belong to
// the neighbours).
// Speculative use (round 6; w = 1 only): `d_skip` points at a device word that the work enqueued ahead of this call leaves at zero when this call is
// wanted -- the all-reduced count of undecided pixels of the marking batch that precedes it in the stream -- and `h_skip` at the host copy of that word
// (copied on the same stream before the call).  The list and fallback kernels do nothing when the word is not zero, the estimate kernels then find empty
// lists, and *skipped says so once the host has seen the word: the caller goes on marking and calls again.  The host waits for ONE event in here (list
// lengths + that word), with the first chunk of estimate kernels already enqueued behind it.
int bayes(bcd_hip_ctx *ctx, Work &wk, const float *d_colors, const float *d_pixcov, const uint32_t *d_mask, const int32_t *d_nsim,
          const uint8_t *d_state, int W, int H, int w, int b, float min_eig, float *d_sum, int32_t *d_count, bool defer_redo = false,
          int row_begin = 0, int row_end = INT_MAX, const long long *d_skip = nullptr, const long long *h_skip = nullptr, bool *skipped = nullptr)
{
    const int64_t npix = (int64_t)W * H;
    row_begin = std::max(0, row_begin); row_end = std::min(H, row_end);
    if (skipped) *skipped = false;
    if (d_skip && (w != 1 || !h_skip || !skipped)) return bad(ctx, "speculative estimate: patch radius 1 and a host copy of the word are required");
    const int K = 3 * (2 * w + 1) * (2 * w + 1);
    wk.redo.pending = false;
    RCCHK(ensure(ctx, wk.strong, npix * sizeof(int32_t)));
    RCCHK(ensure(ctx, wk.weak, npix * sizeof(int32_t)));
    RCCHK(ensure(ctx, wk.counters, sizeof(Counters)));
    Counters::Lists *d_c = &wk.d_counters()->lists, *h_c = &wk.h_counters->lists;
    const bool weak_tiles = w == 1; // (other patch radii: the list kernel below)
    h_c->spectral = 0;
    // the two paths only meet in the atomic accumulators: the fallback pixels run on a side stream.  The tiled fallback kernel needs no
    // list (it reads states and |S| itself), so it starts at once -- beside the list compaction and the host round trip for the number of
    // full estimates, during which this scale would otherwise leave the chip idle -- and is out of the way when the prepare kernel arrives
    auto fork_weak_tiles = [&]() -> int {
        RCCHK(fork_aux(ctx, wk));
        HIPCHK(ctx, bcd_launch_bayes_weak_tiles(d_colors, d_mask, d_state, d_nsim, K + 1, W, H, b, d_sum, d_count, wk.aux, row_begin, row_end, d_skip));
        HIPCHK(ctx, hipEventRecord(wk.ev_join, wk.aux));
        return BCD_HIP_OK;
    };
    if (wk.clean_dc) wk.clean_dc = false; // (k_scale_begin)
    else HIPCHK(ctx, hipMemsetAsync(d_c, 0, sizeof(*d_c), wk.stream));
    HIPCHK(ctx, bcd_launch_active_lists(d_state, d_nsim, (int64_t)row_begin * W, (int64_t)row_end * W, K + 1, (int32_t *)wk.strong.p, (int32_t *)wk.weak.p, &d_c->n_strong, wk.stream, d_skip));
    HIPCHK(ctx, hipMemcpyAsync(h_c, d_c, offsetof(Counters::Lists, generic_work), hipMemcpyDeviceToHost, wk.stream)); // (the list lengths and the sum of |S|)
    // (round 5) the list compaction is 253 workgroups of 1024 threads: 18 us alone, 150 us when the fallback kernel's 8 160 tiles were launched
    // first and every CU had to drain before one of them fitted.  The fallback kernel starts BEHIND it (it still overlaps the host round trip).
    if (weak_tiles) RCCHK(fork_weak_tiles());
    const int64_t cap = std::max<int64_t>(1, npix);
    const int cus = estimate_cus(ctx, wk);
    const int weak_blocks = (int)std::min<int64_t>(cap, (int64_t)cus * 32);
    if (!weak_tiles) { // the list kernel (other patch radii): many cheap items beside the full estimate's few long ones
        RCCHK(fork_aux(ctx, wk));
        HIPCHK(ctx, bcd_launch_bayes_weak(d_colors, d_mask, (const int32_t *)wk.weak.p, &d_c->n_weak, weak_blocks, W, H, w, b, d_sum, d_count, wk.aux));
        HIPCHK(ctx, hipEventRecord(wk.ev_join, wk.aux));
    }
    if (w == 1) {
        const size_t rec = bcd_bayes27_record_bytes();
        const int chunk_max = ESTIMATE_CHUNK;
        RCCHK(ensure(ctx, wk.work_q, BCD_WORK_INTS * sizeof(int32_t)));
        auto launch_chunk = [&](int first, int n, bool defer, const int *d_n) -> int {
            if (wk.clean_wq) wk.clean_wq = false; // (k_scale_begin)
            else HIPCHK(ctx, hipMemsetAsync(wk.work_q.p, 0, BCD_WORK_INTS * sizeof(int32_t), wk.stream)); // the work queues of the three kernels
            HIPCHK(ctx, bcd_launch_bayes27(d_colors, d_pixcov, d_mask, (const int32_t *)wk.strong.p, first, n, (int *)wk.work_q.p, cus, W, H, b, min_eig,
                                           (float *)wk.gscratch.p, d_sum, d_count, &d_c->spectral, wk.stream, defer ? 1 : 0, d_n));
            return BCD_HIP_OK;
        };
        // Round 6: the first chunk does not wait for the host.  The list's length is on its way back (the copy above), the previous frame of this
        // geometry on this workspace said how many items to expect: the three kernels are launched for that many + 1/8 with the length read on the
        // DEVICE (records sized for the capacity; wavefronts without an item leave at once), the host waits for the COPY only -- while the prepare
        // kernel is already running -- and launches further chunks for whatever the capacity did not cover.  A first frame, a workspace whose last
        // frame had (next to) no full estimates, and lists beyond one chunk take the synchronous path below.
        int ahead = 0;
        HIPCHK(ctx, hipEventRecord(wk.ev_counts, wk.stream));
        if (wk.strong_hint_W == W && wk.strong_hint_H == H && wk.strong_hint >= 512 && wk.strong_hint + wk.strong_hint / 8 + 1024 <= chunk_max) {
            ahead = wk.strong_hint + wk.strong_hint / 8 + 1024;
            RCCHK(ensure(ctx, wk.gscratch, rec * (size_t)ahead));
            RCCHK(launch_chunk(0, ahead, defer_redo, &d_c->n_strong));
        }
        HIPCHK(ctx, hipEventSynchronize(wk.ev_counts));
        if (h_skip && *h_skip != 0) { // the speculation failed: nothing was listed, the kernels enqueued above found nothing to do
            *skipped = true;
            HIPCHK(ctx, hipStreamWaitEvent(wk.stream, wk.ev_join, 0));
            return BCD_HIP_OK;
        }
        const int n_strong = h_c->n_strong;
        wk.strong_hint = n_strong; wk.strong_hint_W = W; wk.strong_hint_H = H;
        if (ahead > 0 && n_strong <= ahead) {
            if (defer_redo) { wk.redo.pending = true; wk.redo.first = 0; wk.redo.n = ahead; wk.redo.cus = cus; } // (the counter is h_counters->lists.spectral, below)
        } else {
            if (ahead > 0 && defer_redo) // the first chunk's records are about to be reused: its redo list (normally empty) is walked now
                HIPCHK(ctx, bcd_launch_bayes27_redo(d_colors, d_pixcov, d_mask, (const int32_t *)wk.strong.p, 0, ahead, (int *)wk.work_q.p, cus, W, H, b, min_eig,
                                                    (float *)wk.gscratch.p, d_sum, d_count, wk.stream));
            const int remaining = n_strong - ahead;
            if (remaining > 0 && ahead == 0) RCCHK(ensure(ctx, wk.gscratch, rec * (size_t)std::min(remaining, chunk_max)));
            const int chunk = ahead > 0 ? ahead : chunk_max; // (the records of a first chunk launched ahead are laid out for `ahead` items)
            for (int first = ahead; first < n_strong; first += chunk) {
                const int n = std::min(chunk, n_strong - first);
                // one chunk (the usual case) and a caller that looks at the redo counter after its last synchronisation: the redo kernel waits for that
                const bool defer = defer_redo && ahead == 0 && n_strong <= chunk_max;
                RCCHK(launch_chunk(first, n, defer, nullptr));
                if (defer) { wk.redo.pending = true; wk.redo.first = first; wk.redo.n = n; wk.redo.cus = cus; }
            }
            if (ahead > 0 && remaining > 0) {
                // the guess was too small (a frame unlike its predecessor: -m 0 after -m 1): this frame has gone through in chunks of the guessed size;
                // the records grow to what the next frame of its kind needs NOW, in the frame that met the change (the growth waits for the chunks)
                HIPCHK(ctx, hipStreamSynchronize(wk.stream));
                RCCHK(ensure(ctx, wk.gscratch, rec * (size_t)std::min(n_strong, chunk_max)));
            }
        }
        HIPCHK(ctx, hipMemcpyAsync(&h_c->spectral, &d_c->spectral, sizeof(int32_t), hipMemcpyDeviceToHost, wk.stream)); // read after the scale's last synchronisation
    } else {
        const size_t per_block = bcd_bayes_scratch_bytes_per_block(w, b);
        const int strong_blocks = (int)std::min<int64_t>(cap, 1024); // generic kernel: 1024 scratch slices
        if (per_block) RCCHK(ensure(ctx, wk.gscratch, per_block * (size_t)strong_blocks));
        HIPCHK(ctx, bcd_launch_bayes_strong(d_colors, d_pixcov, d_mask, (const int32_t *)wk.strong.p, &d_c->n_strong, d_c->generic_work, strong_blocks, W, H, w, b, min_eig,
                                            d_sum, d_count, (float *)wk.gscratch.p, wk.gscratch.bytes, wk.stream));
    }
    HIPCHK(ctx, hipStreamWaitEvent(wk.stream, wk.ev_join, 0));
    return BCD_HIP_OK;
}

void bayes_counts(const Work &wk, int64_t *n_strong, int64_t *n_weak, int64_t *sim_total)
{
    *n_strong = wk.h_counters->lists.n_strong;
    *n_weak = wk.h_counters->lists.n_weak;
    *sim_total = wk.h_counters->lists.sim_total;
}

// The estimate stage of the extra colour layers of a scale, on the selection the first layer's chain has just decided (mono_accumulate; the stream is
// synchronised, wk.h_counters->lists holds the list lengths): nothing is selected, marked or listed again.  The fallback pixels of ALL layers go through one
// launch of the layered tile kernel on the side stream (3 x 3 patches; other radii: the list kernel per layer), the full-estimate chain runs once per
// layer over the same item list and work queues with that layer's colours and covariances -- its 9.9 KB records are reused from layer to layer, its redo
// list (items whose sweep inverse failed ITS matrices' checks) is walked behind each layer's finish kernel.  No kernel gets the count image: it is the
// first layer's.  One launch finalises every layer.
// d_mask / d_nsim / d_state: the selection (a frame: the workspace's); pixcov[k] / sum[k]: per-pixel covariances and (cleared) sums of extra layer k (a frame:
// slices of wk.lay_pixcov / wk.lay_sum); spectral[1 + E]: per layer, the items that took the redo list; lv.out[k] null for every k (the stage-level entry
// point): the sums are left as they are, nothing is finalised.
// `kept` (bcd_hip_selection_denoise): the lists and their lengths are a kept selection's, not the workspace's -- d_mask / d_nsim / d_state / d_count are then
// its buffers too -- every layer of the call is a follower (up to BCD_MAX_LAYERS of them), and the redo counter starts at zero: spectral[0] = 0.
} // namespace

// what the temporal calls (bcd_temporal.hip) share with the guided scale: declared in bcd_ctx.h
int guide_gate_masks(bcd_hip_ctx *ctx, Work &wk, const float *d_features, const float *d_variances, int W, int H, int w, int b, uint32_t *d_mask, int32_t *d_count)
{
    return guide_gate(ctx, wk, d_features, d_variances, W, H, w, b, d_mask, d_count);
}

int distance_timing_events(bcd_hip_ctx *ctx, Work &wk, hipEvent_t *e0, hipEvent_t *e1) { return timing_events(ctx, wk, e0, e1); }

int moments_masks(bcd_hip_ctx *ctx, Work &wk, const float *d_colors, const float *d_pixcov, int W, int H, int w, int b, float tau, float var_floor, uint32_t *d_mask,
                  int32_t *d_count)
{
    return similarity_moments(ctx, wk, d_colors, d_pixcov, W, H, w, b, tau, var_floor, d_mask, d_count);
}

int layers_follow(bcd_hip_ctx *ctx, Work &wk, const LayerView &lv, const uint32_t *d_mask, const int32_t *d_nsim, const uint8_t *d_state,
                  const float *const *pixcov, float *const *sum, int W, int H, int w, int b, float min_eig, const int32_t *d_count, int32_t *spectral,
                  const KeptLists *kept)
{
    const int E = lv.n;
    const int64_t npix = (int64_t)W * H;
    const int K = 3 * (2 * w + 1) * (2 * w + 1);
    Counters::Lists *d_c = &wk.d_counters()->lists;
    Counters *h = wk.h_counters;
    const int32_t *strong = kept ? kept->strong : (const int32_t *)wk.strong.p, *weak = kept ? kept->weak : (const int32_t *)wk.weak.p;
    const int32_t *d_n_strong = kept ? kept->d_len : &d_c->n_strong, *d_n_weak = kept ? kept->d_len + 1 : &d_c->n_weak;
    const int n_strong = kept ? kept->n_strong : h->lists.n_strong;
    if (kept) { // no first layer's chain left a redo count behind
        HIPCHK(ctx, hipMemsetAsync(&d_c->spectral, 0, sizeof(int32_t), wk.stream));
        h->lists.spectral = 0;
    }
    spectral[0] = h->lists.spectral;
    const int cus = estimate_cus(ctx, wk);
    RCCHK(fork_aux(ctx, wk));
    if (w == 1) {
        BcdLayerTable t = {};
        for (int k = 0; k < E; ++k) { t.a[k] = lv.col[k]; t.o[k] = sum[k]; }
        HIPCHK(ctx, bcd_launch_bayes_weak_tiles_layers(t, E, d_mask, d_state, d_nsim, K + 1, W, H, b, wk.aux, 0, H));
    } else {
        const int weak_blocks = (int)std::min<int64_t>(std::max<int64_t>(1, npix), (int64_t)cus * 32);
        for (int k = 0; k < E; ++k)
            HIPCHK(ctx, bcd_launch_bayes_weak(lv.col[k], d_mask, weak, d_n_weak, weak_blocks, W, H, w, b, sum[k], nullptr, wk.aux));
    }
    HIPCHK(ctx, hipEventRecord(wk.ev_join, wk.aux));
    if (w == 1) {
        const size_t rec = bcd_bayes27_record_bytes();
        const int chunk_max = ESTIMATE_CHUNK;
        if (n_strong > 0) RCCHK(ensure(ctx, wk.gscratch, rec * (size_t)std::min(n_strong, chunk_max)));
        for (int k = 0; k < E; ++k) {
            for (int first = 0; first < n_strong; first += chunk_max) {
                HIPCHK(ctx, hipMemsetAsync(wk.work_q.p, 0, BCD_WORK_INTS * sizeof(int32_t), wk.stream));
                HIPCHK(ctx, bcd_launch_bayes27(lv.col[k], pixcov[k], d_mask, strong, first, std::min(chunk_max, n_strong - first),
                                               (int *)wk.work_q.p, cus, W, H, b, min_eig, (float *)wk.gscratch.p, sum[k], nullptr, &d_c->spectral, wk.stream, 0, nullptr));
            }
            HIPCHK(ctx, hipMemcpyAsync(&h->layer_redo_total[k], &d_c->spectral, sizeof(int32_t), hipMemcpyDeviceToHost, wk.stream)); // (running total: the layers so far)
        }
    } else {
        const size_t per_block = bcd_bayes_scratch_bytes_per_block(w, b);
        const int strong_blocks = (int)std::min<int64_t>(std::max<int64_t>(1, npix), 1024);
        if (per_block) RCCHK(ensure(ctx, wk.gscratch, per_block * (size_t)strong_blocks));
        for (int k = 0; k < E; ++k) {
            HIPCHK(ctx, bcd_launch_bayes_strong(lv.col[k], pixcov[k], d_mask, strong, d_n_strong, d_c->generic_work, strong_blocks, W, H, w, b, min_eig,
                                                sum[k], nullptr, (float *)wk.gscratch.p, wk.gscratch.bytes, wk.stream));
            h->layer_redo_total[k] = h->lists.spectral;
        }
    }
    HIPCHK(ctx, hipStreamWaitEvent(wk.stream, wk.ev_join, 0));
    if (lv.out[0]) {
        BcdLayerTable t = {};
        for (int k = 0; k < E; ++k) { t.a[k] = sum[k]; t.o[k] = lv.out[k]; }
        HIPCHK(ctx, bcd_launch_layers_finalize(t, E, d_count, npix, wk.stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    for (int k = 0; k < E; ++k) spectral[k + 1] = h->layer_redo_total[k] - (k == 0 ? h->lists.spectral : h->layer_redo_total[k - 1]);
    h->lists.spectral = h->layer_redo_total[E - 1]; // the scale's figure: the sum over the layers
    return BCD_HIP_OK;
}

namespace {

// one scale: accumulators only (d_sum / d_count are zeroed here)
int mono_accumulate(bcd_hip_ctx *ctx, Work &wk, const float *d_colors, const float *d_ns, const float *d_hist, const float *d_cov,
                    int W, int H, int D, int row_begin, int row_end, const bcd_hip_params *prm, uint32_t seed, int scale,
                    float *d_sum, int32_t *d_count, float *d_out = nullptr /* finalised image, optional */,
                    const LayerView *lv = nullptr /* further colour layers on the same selection (needs d_out and the whole frame), optional */)
{
    const int w = prm->patch_radius, b = prm->search_radius;
    const size_t npix = (size_t)W * H;
    const int side = 2 * b + 1, words = (side * side + 31) / 32;
    RCCHK(ensure(ctx, wk.pixcov, npix * 6 * sizeof(float)));
    RCCHK(ensure(ctx, wk.mask, npix * words * sizeof(uint32_t)));
    RCCHK(ensure(ctx, wk.nsim, npix * sizeof(int32_t)));
    RCCHK(ensure(ctx, wk.state, npix));
    bcd_hip_scale_stats &st = ctx->stats[scale < MAX_SCALES ? scale : MAX_SCALES - 1];
    memset(&st, 0, sizeof(st));
    st.width = W; st.height = H;
    st.main_pixels = (int64_t)std::max(0, W - 2 * w) * std::max(0, std::min(row_end, H - w) - std::max(row_begin, w));
    const bool prof = ctx->profiling;
    // Host round trips of a scale: one per batch of marking launches (normally a single batch; it also brings the range flag of
    // the fast division back), and one at the end for the counters.  The estimate kernels take their list lengths from device
    // memory, the finalisation is enqueued before the last synchronisation.
    if (prof) HIPCHK(ctx, hipEventRecord(wk.ev_stage[0], wk.stream));
    // The per-pixel covariances (only the estimate stage reads them) and the clearing of the accumulators go to the side stream: the scale's
    // own stream starts with the distance kernel, they run beside it instead of ahead of it / between marking and estimate
    RCCHK(fork_aux(ctx, wk)); // (the inputs are ready at this point of the scale's stream)
    HIPCHK(ctx, bcd_launch_pixel_cov_clear(d_cov, d_ns, (int64_t)npix, (float *)wk.pixcov.p, d_sum, d_count, wk.aux)); // (+ the accumulators cleared: one launch)
    if (lv && lv->n > 0) { // the same for every further layer, one launch (their sums; the count image is shared)
        RCCHK(ensure(ctx, wk.lay_pixcov, (size_t)lv->n * npix * 6 * sizeof(float)));
        RCCHK(ensure(ctx, wk.lay_sum, (size_t)lv->n * npix * 3 * sizeof(float)));
        BcdLayerTable t = {};
        for (int k = 0; k < lv->n; ++k) t.a[k] = lv->cov[k];
        HIPCHK(ctx, bcd_launch_layers_pixel_cov_clear(t, lv->n, d_ns, (int64_t)npix, (float *)wk.lay_pixcov.p, (float *)wk.lay_sum.p, wk.aux));
    }
    HIPCHK(ctx, hipEventRecord(wk.ev_pixcov, wk.aux));
    // every counter, flag and work queue of the chain in one launch at the head of the scale's stream (round 4: they were ~7 fills between
    // the kernels of the critical path); flags raised by distance planes computed ahead of this call are kept
    {
        constexpr size_t LINE_INTS = (size_t)BCD_CNT_LINES * BCD_CNT_STRIDE;
        RCCHK(ensure(ctx, wk.counters, sizeof(Counters)));
        RCCHK(ensure(ctx, wk.cnt_lines, ROUND_BATCH * LINE_INTS * sizeof(int)));
        RCCHK(ensure(ctx, wk.work_q, BCD_WORK_INTS * sizeof(int32_t)));
        const bool ahead = wk.planes.ready; // (its launches raise flags.range and flags.other_count)
        HIPCHK(ctx, bcd_launch_scale_begin((int *)wk.counters.p, COUNTER_WORDS, ahead ? COUNTER_WORD(flags.range) : -1, ahead ? COUNTER_WORD(flags.other_count) : -1,
                                           (int *)wk.cnt_lines.p, (int)(ROUND_BATCH * LINE_INTS), (int *)wk.work_q.p, BCD_WORK_INTS, wk.stream));
        wk.clean_flags = wk.clean_lines = wk.clean_dc = wk.clean_wq = true;
    }
    const bool marking = prm->marked_skip_probability > 0.f;
    // Round 6: with marking and 3 x 3 patches the estimate is enqueued BEHIND every marking batch, valid only if that batch decided the last pixel and the
    // masks passed their checks (one device word says so: k_sum_counter_lines); the host waits once per batch -- for that word and the list lengths together,
    // inside bayes() -- where it used to wait for the batch, then for the lists.  A batch that leaves pixels undecided (rare: the batch is sized from the
    // previous frame) costs the empty launches of one skipped estimate.
    const bool speculate = marking && w == 1;
    const long long REDO = 1ll << 40;
    bool estimated = false;
    const bool moments = ctx->moments.on; // (bcd_hip_denoise_moments: one pass that needs no verdict, like the exact kernels)
    const bool guided = ctx->guide.on;    // (bcd_hip_denoise_guided: level `scale` of the feature pyramid gates this scale's selection)
    const int gs = scale >= 0 && scale < MAX_SCALES ? scale : 0;
    for (int attempt = 0, mode = moments ? 1 : 2; attempt < 4; ++attempt) { // production kernels; if they complain: general sample counts (RATIO form, then the reference's operations), then exact kernels
        if (moments) {
            HIPCHK(ctx, hipStreamWaitEvent(wk.stream, wk.ev_pixcov, 0)); // the distance kernel reads the guide's per-pixel covariances (side stream)
            RCCHK(similarity_moments(ctx, wk, d_colors, (const float *)wk.pixcov.p, W, H, w, b, prm->hist_dist_threshold, ctx->moments.var_floor, (uint32_t *)wk.mask.p,
                                     (int32_t *)wk.nsim.p));
        } else
            RCCHK(similarity(ctx, wk, d_hist, d_ns, W, H, D, w, b, prm->hist_dist_threshold, (uint32_t *)wk.mask.p, (int32_t *)wk.nsim.p, mode));
        if (guided) // (bcd_hip_denoise_guided: the gate follows every run and re-run of the selection pass, ahead of the marking)
            RCCHK(guide_gate(ctx, wk, ctx->guide.f[gs], ctx->guide.v[gs], W, H, w, b, (uint32_t *)wk.mask.p, (int32_t *)wk.nsim.p));
        if (prof && attempt == 0) HIPCHK(ctx, hipEventRecord(wk.ev_stage[1], wk.stream));
        if (!speculate) {
            RCCHK(active_set(ctx, wk, (const uint32_t *)wk.mask.p, (const int32_t *)wk.nsim.p, W, H, w, b, row_begin, row_end,
                             prm->marked_skip_probability, prm->use_random_pixel_order, seed, (uint8_t *)wk.state.p, &st.active_rounds));
            if (mode == 1) break;
            if (!marking) HIPCHK(ctx, hipStreamSynchronize(wk.stream)); // no marking batch brought the flag back
        } else {
            HIPCHK(ctx, bcd_launch_active_init((const int32_t *)wk.nsim.p, W, H, w, row_begin, row_end, prm->marked_skip_probability, seed, 0, (uint8_t *)wk.state.p, wk.stream));
            wk.dep_ready = false;
            if (attempt == 0) HIPCHK(ctx, hipStreamWaitEvent(wk.stream, wk.ev_pixcov, 0)); // covariances computed, accumulators cleared (long done)
            long long *d_total = &wk.d_counters()->marking_total, *h_total = &wk.h_counters->marking_total;
            const uint32_t key_seed = prm->use_random_pixel_order == 2 ? bcd_strip_order_seed(W, H, w, b) : seed; // (as active_set)
            int rounds = 0;
            long long before = -1;
            for (;;) {
                RCCHK(active_step_enqueue(ctx, wk, (const uint32_t *)wk.mask.p, (const int32_t *)wk.nsim.p, W, H, w, b, row_begin, row_end, prm->use_random_pixel_order,
                                          key_seed, 0, (uint8_t *)wk.state.p, d_total, mode != 1));
                HIPCHK(ctx, hipMemcpyAsync(h_total, d_total, sizeof(long long), hipMemcpyDeviceToHost, wk.stream));
                bool skipped = false;
                wk.clean_flags = wk.clean_lines = false; // (consumed by the similarity pass and the batch)
                RCCHK(bayes(ctx, wk, d_colors, (const float *)wk.pixcov.p, (const uint32_t *)wk.mask.p, (const int32_t *)wk.nsim.p, (const uint8_t *)wk.state.p, W, H, w, b,
                            prm->min_eigen_value, d_sum, d_count, true, 0, H, d_total, h_total, &skipped));
                int undecided = 0, n = 0;
                active_step_collect(wk, &undecided, &n); // (bayes() waited for an event behind the batch's counters)
                rounds += n;
                if (!skipped) { estimated = true; (void)similarity_redo_mode(wk); break; } // (0 by construction; keeps the workspace's memory of uniform sample counts)
                if (*h_total >= REDO) break; // the masks did not pass: again with the next kind of kernels
                if (before >= 0 && *h_total >= before) { set_err(ctx, "marking fixed point made no progress"); return BCD_HIP_EDEVICE; }
                before = *h_total;
            }
            wk.rounds_hint = rounds;
            st.active_rounds = rounds;
            if (estimated) break;
        }
        const int redo = similarity_redo_mode(wk);
        if (redo == 0) break; // inputs inside the guarded range, uniform-count guess right, borderline list not overflowed
        mode = (redo == 3 && (mode == 2 || wk.ratio_used)) ? 3 : 1; // (wk.ratio_used: the RATIO form declined and the workspace has noted it -- the reference's operations are next)
    }
    progress_add(ctx, 0.5 * (double)npix); // similar patches selected, processed set known
    if (prof) HIPCHK(ctx, hipEventRecord(wk.ev_stage[2], wk.stream));
    if (!estimated) {
        HIPCHK(ctx, hipStreamWaitEvent(wk.stream, wk.ev_pixcov, 0)); // covariances computed, accumulators cleared (long done)
        wk.clean_flags = wk.clean_lines = false; // (consumed, or never used by this configuration)
        RCCHK(bayes(ctx, wk, d_colors, (const float *)wk.pixcov.p, (const uint32_t *)wk.mask.p, (const int32_t *)wk.nsim.p,
                    (const uint8_t *)wk.state.p, W, H, w, b, prm->min_eigen_value, d_sum, d_count, true));
    }
    wk.clean_dc = wk.clean_wq = false;
    if (prof) HIPCHK(ctx, hipEventRecord(wk.ev_stage[3], wk.stream));
    if (d_out) HIPCHK(ctx, bcd_launch_finalize(d_sum, d_count, (int64_t)npix, d_out, wk.stream));
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    if (wk.redo.pending && wk.h_counters->lists.spectral > 0) {
        // items whose sweep inverse failed its checks (large -e, ill-conditioned frames): their list goes through the LDS kernel now
        // (spectral inverse), and the finalisation is repeated on the completed accumulators
        HIPCHK(ctx, bcd_launch_bayes27_redo(d_colors, (const float *)wk.pixcov.p, (const uint32_t *)wk.mask.p, (const int32_t *)wk.strong.p, wk.redo.first, wk.redo.n,
                                            (int *)wk.work_q.p, wk.redo.cus, W, H, b, prm->min_eigen_value, (float *)wk.gscratch.p, d_sum, d_count, wk.stream));
        if (d_out) HIPCHK(ctx, bcd_launch_finalize(d_sum, d_count, (int64_t)npix, d_out, wk.stream));
        HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    }
    wk.redo.pending = false;
    if (lv && lv->n > 0) {
        const float *lay_pixcov[BCD_MAX_LAYERS];
        float *lay_sum[BCD_MAX_LAYERS];
        for (int k = 0; k < lv->n; ++k) { lay_pixcov[k] = (const float *)wk.lay_pixcov.p + (size_t)k * npix * 6; lay_sum[k] = (float *)wk.lay_sum.p + (size_t)k * npix * 3; }
        RCCHK(layers_follow(ctx, wk, *lv, (const uint32_t *)wk.mask.p, (const int32_t *)wk.nsim.p, (const uint8_t *)wk.state.p, lay_pixcov, lay_sum, W, H, w, b,
                            prm->min_eigen_value, d_count, ctx->layer_spectral[scale < MAX_SCALES ? scale : MAX_SCALES - 1]));
    }
    progress_add(ctx, 0.5 * (double)npix);
    int64_t ns = 0, nw = 0, tot = 0;
    bayes_counts(wk, &ns, &nw, &tot);
    st.processed = ns + nw; st.fallback = nw; st.similar_total = tot;
    st.similarity_path = moments ? 3 : wk.border_capacity > 0 ? (wk.ratio_used ? 2 : 1) : 0;
    st.borderline_pairs = wk.border_capacity > 0 ? wk.h_counters->flags.borderline : 0;
    st.cu_share = estimate_share_pct(ctx, wk);
    st.spectral_inverses = wk.h_counters->lists.spectral;
    if (prof) {
        st.ms_similarity = stage_ms(wk, 0, 1);
        st.ms_active = stage_ms(wk, 1, 2);
        st.ms_bayes = stage_ms(wk, 2, 3);
        st.ms_total = stage_ms(wk, 0, 3);
    }
    if (ctx->keep) RCCHK(selection_store(ctx, wk, scale, d_ns, W, H, b, d_count, st)); // (bcd_hip_denoise_layers_keep: copies on this scale's stream)
    return BCD_HIP_OK;
}

// mergeOutputs (MultiscaleDenoiser.cpp:453-466) on a workspace's stream: hi -= up(down(hi)); hi += up(lo)
int merge_on(bcd_hip_ctx *ctx, Work &wk, float *d_hi, int W, int H, const float *d_lo, int D)
{
    const int w2 = W / 2, h2 = H / 2;
    RCCHK(ensure(ctx, wk.tmp_lo, (size_t)w2 * h2 * D * sizeof(float)));
    HIPCHK(ctx, bcd_launch_downscale(1, d_hi, W, H, D, (float *)wk.tmp_lo.p, wk.stream));
    HIPCHK(ctx, bcd_launch_merge_interpolate((const float *)wk.tmp_lo.p, d_lo, w2, h2, D, d_hi, W, H, wk.stream)); // (round 6: the two interpolations in one pass)
    return BCD_HIP_OK;
}

// one pyramid level from the finer one (MultiscaleDenoiser.cpp:41-53) on `st`
int build_level(bcd_hip_ctx *ctx, const float *col, const float *ns, const float *hs, const float *cv, int W, int H, int D,
                DevBuf (&lvl)[5], hipStream_t st)
{
    HIPCHK(ctx, bcd_launch_downscale(1, col, W, H, 3, (float *)lvl[0].p, st));
    HIPCHK(ctx, bcd_launch_downscale(0, ns, W, H, 1, (float *)lvl[1].p, st));
    if (hs) HIPCHK(ctx, bcd_launch_downscale(0, hs, W, H, D, (float *)lvl[2].p, st)); // (null: a selection from means and covariances has no histogram level)
    HIPCHK(ctx, bcd_launch_downscale_cov(cv, ns, W, H, (float *)lvl[3].p, st));
    return BCD_HIP_OK;
}

int mono(bcd_hip_ctx *ctx, Work &wk, const float *d_colors, const float *d_ns, const float *d_hist, const float *d_cov, int W, int H, int D,
         const bcd_hip_params *prm, uint32_t seed, int scale, float *d_out, const LayerView *lv = nullptr)
{
    const size_t npix = (size_t)W * H;
    RCCHK(ensure(ctx, wk.sum, npix * 3 * sizeof(float)));
    RCCHK(ensure(ctx, wk.cnt, npix * sizeof(int32_t)));
    return mono_accumulate(ctx, wk, d_colors, d_ns, d_hist, d_cov, W, H, D, 0, H, prm, seed, scale, (float *)wk.sum.p, (int32_t *)wk.cnt.p, d_out, lv);
}

} // namespace

// the pyramid level of the extra layers (colour averaged, covariance weighted by the SHARED sample counts of the finer level): two launches for all of them
int build_level_layers(bcd_hip_ctx *ctx, const LayerView &fine, const LayerView &coarse, const float *ns_fine, int W, int H, hipStream_t st)
{
    BcdLayerTable t = {};
    for (int k = 0; k < fine.n; ++k) { t.a[k] = fine.col[k]; t.o[k] = const_cast<float *>(coarse.col[k]); }
    HIPCHK(ctx, bcd_launch_layers_downscale_avg(t, fine.n, W, H, st));
    for (int k = 0; k < fine.n; ++k) { t.a[k] = fine.cov[k]; t.o[k] = const_cast<float *>(coarse.cov[k]); }
    HIPCHK(ctx, bcd_launch_layers_downscale_cov(t, fine.n, ns_fine, W, H, st));
    return BCD_HIP_OK;
}

// merge_on for the extra layers' outputs: two launches for all of them.  scratch: the buffer that takes the reduced outputs, one slice per layer (the
// workspace's lay_tmp_lo in a frame's own calls, ctx->temporal.lay_tmp_lo in the temporal calls and the pops of a sequence)
int merge_layers_on(bcd_hip_ctx *ctx, Work &wk, DevBuf &scratch, const LayerView &hi, int W, int H, const LayerView &lo)
{
    const int w2 = W / 2, h2 = H / 2;
    const size_t slice = (size_t)w2 * h2 * 3;
    RCCHK(ensure(ctx, scratch, (size_t)hi.n * slice * sizeof(float)));
    BcdLayerTable t = {};
    for (int k = 0; k < hi.n; ++k) { t.a[k] = hi.out[k]; t.o[k] = (float *)scratch.p + k * slice; }
    HIPCHK(ctx, bcd_launch_layers_downscale_avg(t, hi.n, W, H, wk.stream));
    for (int k = 0; k < hi.n; ++k) { t.a[k] = (const float *)scratch.p + k * slice; t.b[k] = lo.out[k]; t.o[k] = hi.out[k]; }
    HIPCHK(ctx, bcd_launch_layers_merge(t, hi.n, w2, h2, W, H, wk.stream));
    return BCD_HIP_OK;
}

int work_init(bcd_hip_ctx *ctx, Work &w, hipStream_t stream)
{
    if (w.initialised) return BCD_HIP_OK;
    if (w.h_counters || w.aux || w.ev_done) return bad(ctx, "workspace left half-initialised by an earlier failure"); // never run on null handles
    if (stream) w.stream = stream;
    else {
        HIPCHK(ctx, hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
        w.owns_stream = true;
    }
    HIPCHK(ctx, hipHostMalloc((void **)&w.h_counters, sizeof(Counters), hipHostMallocDefault));
    for (int i = 0; i < 4; ++i) HIPCHK(ctx, hipEventCreate(&w.ev_stage[i]));
    HIPCHK(ctx, hipEventCreateWithFlags(&w.ev_done, hipEventDisableTiming));
    HIPCHK(ctx, hipEventCreateWithFlags(&w.ev_built, hipEventDisableTiming));
    HIPCHK(ctx, hipStreamCreateWithFlags(&w.aux, hipStreamNonBlocking));
    HIPCHK(ctx, hipEventCreateWithFlags(&w.ev_fork, hipEventDisableTiming));
    HIPCHK(ctx, hipEventCreateWithFlags(&w.ev_join, hipEventDisableTiming));
    HIPCHK(ctx, hipEventCreateWithFlags(&w.ev_pixcov, hipEventDisableTiming));
    HIPCHK(ctx, hipEventCreateWithFlags(&w.ev_counts, hipEventDisableTiming));
    w.initialised = true;
    return BCD_HIP_OK;
}

namespace {

void work_destroy(Work &w)
{
    DevBuf *bufs[] = { &w.T, &w.Cn, &w.mask, &w.fwd, &w.nsim, &w.state, &w.strong, &w.weak, &w.counters, &w.cnt_lines, &w.work_q, &w.pixcov, &w.sum, &w.cnt, &w.gscratch, &w.dep, &w.tmp_lo, &w.border, &w.ratio_stats, &w.lay_pixcov, &w.lay_sum, &w.lay_tmp_lo, &w.gate_mask, &w.gate_nsim };
    for (DevBuf *b : bufs) if (b->p) (void)hipFree(b->p);
    if (w.h_counters) (void)hipHostFree(w.h_counters);
    for (auto &pr : w.ev_pool) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (int i = 0; i < 4; ++i) if (w.ev_stage[i]) (void)hipEventDestroy(w.ev_stage[i]);
    if (w.ev_done) (void)hipEventDestroy(w.ev_done);
    if (w.ev_built) (void)hipEventDestroy(w.ev_built);
    if (w.ev_fork) (void)hipEventDestroy(w.ev_fork);
    if (w.ev_join) (void)hipEventDestroy(w.ev_join);
    if (w.ev_pixcov) (void)hipEventDestroy(w.ev_pixcov);
    if (w.ev_counts) (void)hipEventDestroy(w.ev_counts);
    if (w.aux) (void)hipStreamDestroy(w.aux);
    if (w.owns_stream && w.stream) (void)hipStreamDestroy(w.stream);
}

} // namespace

// =====================================================================================================
extern "C" {

int bcd_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void bcd_hip_default_params(bcd_hip_params *p)
{
    if (!p) return;
    p->hist_dist_threshold = 1.f;   // IDenoiser.h:23-31
    p->patch_radius = 1;
    p->search_radius = 6;
    p->min_eigen_value = 1.e-8f;
    p->use_random_pixel_order = 1;
    p->marked_skip_probability = 1.f;
    p->order_seed = 1234u;
}

int bcd_hip_ctx_create(bcd_hip_ctx **out, int device, void *hip_stream)
{
    if (!out) return BCD_HIP_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0 || device < 0 || device >= n) return BCD_HIP_EDEVICE;
    bcd_hip_ctx *ctx = new (std::nothrow) bcd_hip_ctx();
    if (!ctx) return BCD_HIP_ENOMEM;
    ctx->device = device;
    DeviceGuard guard(ctx);
    if (!guard.ok) { delete ctx; return BCD_HIP_EDEVICE; }
    memset(ctx->stats, 0, sizeof(ctx->stats));
    memset(ctx->layer_spectral, 0, sizeof(ctx->layer_spectral));
    if (hip_stream) ctx->stream = (hipStream_t)hip_stream;
    else {
        if (hipStreamCreate(&ctx->stream) != hipSuccess) { delete ctx; return BCD_HIP_EDEVICE; }
        ctx->owns_stream = true;
    }
    if (work_init(ctx, ctx->main, ctx->stream) != BCD_HIP_OK || hipEventCreateWithFlags(&ctx->ev_pyramid, hipEventDisableTiming) != hipSuccess) {
        bcd_hip_ctx_destroy(ctx);
        return BCD_HIP_EDEVICE;
    }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) == hipSuccess && cus > 0) ctx->num_cus = cus;
    }
    const char *env = getenv("BCD_HIP_SERIAL_SCALES");
    ctx->concurrent_scales = !(env && env[0] == '1');
    env = getenv("BCD_HIP_EXACT_SIMILARITY");
    ctx->fast_similarity = !(env && env[0] == '1');
    env = getenv("BCD_HIP_TC_PLANES");
    ctx->margin_planes = !(env && env[0] == '1');
    env = getenv("BCD_HIP_STREAM_UPLOADS");
    ctx->stream_uploads = !(env && env[0] == '0');
    env = getenv("BCD_HIP_SPARSE_UPLOAD");
    ctx->sparse_uploads = !(env && env[0] == '0');
    *out = ctx;
    return BCD_HIP_OK;
}

void bcd_hip_ctx_destroy(bcd_hip_ctx *ctx)
{
    if (!ctx) return;
    if (ctx->async.th.joinable()) { // (a frame still in flight is finished first)
        { std::lock_guard<std::mutex> lk(ctx->async.mu); ctx->async.quit = true; }
        ctx->async.cv.notify_all();
        ctx->async.th.join();
    }
    DeviceGuard guard(ctx);
    (void)hipDeviceSynchronize();
    work_destroy(ctx->main);
    for (int s = 0; s < MAX_SCALES; ++s) work_destroy(ctx->extra[s]);
    if (ctx->tmp_lo.p) (void)hipFree(ctx->tmp_lo.p);
    for (DevBuf &hb : ctx->host_stage) if (hb.p) (void)hipFree(hb.p);
    for (DevBuf &hb : ctx->lay_host) if (hb.p) (void)hipFree(hb.p);
    for (DevBuf &hb : ctx->lay_host_f) if (hb.p) (void)hipFree(hb.p);
    if (ctx->spike_map.p) (void)hipFree(ctx->spike_map.p);
    for (DevBuf *hb : { &ctx->spike_count, &ctx->spike_list, &ctx->spike_stage }) if (hb->p) (void)hipFree(hb->p);
    for (int s = 0; s < MAX_SCALES; ++s)
        for (int k = 0; k < 5; ++k) if (ctx->pyr[s][k].p) (void)hipFree(ctx->pyr[s][k].p);
    for (int s = 0; s < MAX_SCALES; ++s)
        for (int k = 0; k < 3; ++k) if (ctx->lay_pyr[s][k].p) (void)hipFree(ctx->lay_pyr[s][k].p);
    for (int s = 0; s < MAX_SCALES; ++s)
        for (int k = 0; k < 2; ++k) if (ctx->guide_pyr[s][k].p) (void)hipFree(ctx->guide_pyr[s][k].p);
    for (DevBuf &hb : ctx->guide_host) if (hb.p) (void)hipFree(hb.p);
    temporal_free(ctx);
    if (ctx->ev_pyramid) (void)hipEventDestroy(ctx->ev_pyramid);
    for (hipEvent_t ev : ctx->ev_upload) (void)hipEventDestroy(ev);
    if (ctx->upload_stream) (void)hipStreamDestroy(ctx->upload_stream);
    if (ctx->upload_stream2) (void)hipStreamDestroy(ctx->upload_stream2);
    if (ctx->ev_upload2) (void)hipEventDestroy(ctx->ev_upload2);
    if (ctx->sparse) bcd_sparse_destroy(ctx->sparse);
    if (ctx->owns_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *bcd_hip_last_error(const bcd_hip_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int bcd_hip_set_profiling(bcd_hip_ctx *ctx, int enabled)
{
    if (!ctx) return BCD_HIP_EINVAL;
    ctx->profiling = enabled != 0;
    return BCD_HIP_OK;
}

int bcd_hip_set_concurrent_scales(bcd_hip_ctx *ctx, int enabled)
{
    if (!ctx) return BCD_HIP_EINVAL;
    ctx->concurrent_scales = enabled != 0;
    return BCD_HIP_OK;
}

int bcd_hip_set_strict_eigensolver(int enabled)
{
    bcd_bayes27_set_strict_eigensolver(enabled);
    return BCD_HIP_OK;
}

int bcd_hip_set_fused_prepare_solve(int enabled)
{
    bcd_bayes27_set_fused_prepare_solve(enabled);
    return BCD_HIP_OK;
}

int bcd_hip_set_fast_similarity(bcd_hip_ctx *ctx, int enabled)
{
    if (!ctx) return BCD_HIP_EINVAL;
    ctx->fast_similarity = enabled != 0;
    return BCD_HIP_OK;
}

int bcd_hip_set_margin_planes(bcd_hip_ctx *ctx, int enabled)
{
    if (!ctx) return BCD_HIP_EINVAL;
    ctx->margin_planes = enabled != 0;
    return BCD_HIP_OK;
}

int bcd_hip_set_cu_share(bcd_hip_ctx *ctx, int percent)
{
    if (!ctx || percent < 1 || percent > 100) return BCD_HIP_EINVAL;
    ctx->cu_share_pct = percent;
    return BCD_HIP_OK;
}

int bcd_hip_get_stats(const bcd_hip_ctx *ctx, int scale, bcd_hip_scale_stats *out)
{
    if (!ctx || !out || scale < 0 || scale >= MAX_SCALES) return BCD_HIP_EINVAL;
    *out = ctx->stats[scale];
    return BCD_HIP_OK;
}

int bcd_hip_kernel_time(const bcd_hip_ctx *cctx, float *ms_pairdist, int32_t *launches)
{
    bcd_hip_ctx *ctx = const_cast<bcd_hip_ctx *>(cctx);
    if (!ctx) return BCD_HIP_EINVAL;
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, hipDeviceSynchronize());
    float tot = 0.f;
    int count = 0;
    Work *works[MAX_SCALES + 1];
    works[0] = &ctx->main;
    for (int s = 0; s < MAX_SCALES; ++s) works[s + 1] = &ctx->extra[s];
    for (Work *w : works)
        for (int i = 0; i < w->ev_used; ++i) {
            float ms = 0.f;
            HIPCHK(ctx, hipEventElapsedTime(&ms, w->ev_pool[i].first, w->ev_pool[i].second));
            tot += ms;
            ++count;
        }
    if (ms_pairdist) *ms_pairdist = tot;
    if (launches) *launches = count;
    return BCD_HIP_OK;
}

int bcd_hip_reset_kernel_time(bcd_hip_ctx *ctx)
{
    if (!ctx) return BCD_HIP_EINVAL;
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, hipDeviceSynchronize());
    ctx->main.ev_used = 0;
    for (int s = 0; s < MAX_SCALES; ++s) ctx->extra[s].ev_used = 0;
    return BCD_HIP_OK;
}

} // extern "C"

// bcd_hip_denoise, and -- with `lv0`: the layers beyond the first at full resolution -- bcd_hip_denoise_layers: the first layer takes exactly the path of a
// plain call, the others follow it scale by scale (pyramid level, estimate on the decided selection, merge)
int denoise_impl(bcd_hip_ctx *ctx, const float *d_colors, const float *d_ns, const float *d_hist, const float *d_cov,
                 int W, int H, int D, int nb_scales, const bcd_hip_params *prm, float *d_out, const LayerView *lv0)
{
    if (!ctx) return BCD_HIP_EINVAL;
    const bool moments = ctx->moments.on; // (bcd_hip_denoise_moments: d_hist is null and D is 0)
    if (!d_colors || !d_ns || (!d_hist && !moments) || !d_cov || !d_out) return bad(ctx, "null image pointer"); // Denoiser.cpp:266-293
    RCCHK(check_params(ctx, W, H, moments ? 1 : D, prm));
    if (nb_scales < 1 || nb_scales > MAX_SCALES) return bad(ctx, "bad number of scales");
    DEVICE_GUARD(ctx);
    const int E = lv0 ? lv0->n : 0; // extra layers
    {
        std::lock_guard<std::mutex> lock(ctx->progress_mutex);
        ctx->progress_done = 0.0;
        ctx->progress_total = 0.0;
        for (int s = 0; s < nb_scales; ++s) ctx->progress_total += (double)(W >> s) * (double)(H >> s);
    }
    if (nb_scales == 1) return mono(ctx, ctx->main, d_colors, d_ns, d_hist, d_cov, W, H, D, prm, bcd_hip_scale_seed(prm->order_seed, 0), 0, d_out, E ? lv0 : nullptr);

    // ---- pyramids (MultiscaleDenoiser.cpp:41-53): level s has dims of level s-1 // 2
    const float *col[MAX_SCALES], *ns[MAX_SCALES], *hs[MAX_SCALES], *cv[MAX_SCALES];
    float *out[MAX_SCALES];
    int ws[MAX_SCALES], hh[MAX_SCALES];
    col[0] = d_colors; ns[0] = d_ns; hs[0] = d_hist; cv[0] = d_cov; out[0] = d_out; ws[0] = W; hh[0] = H;
    for (int s = 1; s < nb_scales; ++s) {
        ws[s] = ws[s - 1] / 2; hh[s] = hh[s - 1] / 2;
        if (ws[s] < 2 * prm->patch_radius + 1 || hh[s] < 2 * prm->patch_radius + 1) return bad(ctx, "too many scales for this image size");
        size_t np = (size_t)ws[s] * hh[s];
        RCCHK(ensure(ctx, ctx->pyr[s][0], np * 3 * sizeof(float)));
        RCCHK(ensure(ctx, ctx->pyr[s][1], np * sizeof(float)));
        if (!moments) RCCHK(ensure(ctx, ctx->pyr[s][2], np * D * sizeof(float)));
        RCCHK(ensure(ctx, ctx->pyr[s][3], np * 6 * sizeof(float)));
        RCCHK(ensure(ctx, ctx->pyr[s][4], np * 3 * sizeof(float)));
        col[s] = (float *)ctx->pyr[s][0].p; ns[s] = (float *)ctx->pyr[s][1].p; hs[s] = moments ? nullptr : (float *)ctx->pyr[s][2].p;
        cv[s] = (float *)ctx->pyr[s][3].p; out[s] = (float *)ctx->pyr[s][4].p;
    }
    std::vector<LayerView> lvs(E ? nb_scales : 0); // the extra layers at every pyramid level
    if (E) lvs[0] = *lv0;
    for (int s = 1; E && s < nb_scales; ++s) {
        const size_t np = (size_t)ws[s] * hh[s];
        RCCHK(ensure(ctx, ctx->lay_pyr[s][0], (size_t)E * np * 3 * sizeof(float)));
        RCCHK(ensure(ctx, ctx->lay_pyr[s][1], (size_t)E * np * 6 * sizeof(float)));
        RCCHK(ensure(ctx, ctx->lay_pyr[s][2], (size_t)E * np * 3 * sizeof(float)));
        lvs[s].n = E;
        for (int k = 0; k < E; ++k) {
            lvs[s].col[k] = (const float *)ctx->lay_pyr[s][0].p + k * np * 3;
            lvs[s].cov[k] = (const float *)ctx->lay_pyr[s][1].p + k * np * 6;
            lvs[s].out[k] = (float *)ctx->lay_pyr[s][2].p + k * np * 3;
        }
    }
    const LayerView *lvp = E ? lvs.data() : nullptr;
    // ---- the scales are independent until the merges (MultiscaleDenoiser.cpp:79-134 runs them coarse to fine, but each
    // Denoiser only reads its own pyramid level): one stream + host thread + workspace per scale.  Scale s > 0 builds its
    // own pyramid level on its stream (from level s-1, once that is complete), so that the finest scale -- the critical
    // path -- starts at once; after its own chain scale s merges the (already merged) scale s+1 into its output.
    if (ctx->concurrent_scales) {
        // The coarse scales' share of the CU slots (bayes()) follows the previous call on the same geometry: they should be through when
        // the finest scale is at 80 - 92 % of its chain -- earlier means their persistent kernels took more room than they needed next to
        // the finest scale's short kernels, later means they have become the critical path.  Small steps down, larger ones up.
        const int64_t key = ((int64_t)W << 40) ^ ((int64_t)H << 20) ^ ((int64_t)nb_scales << 12) ^ ((int64_t)prm->search_radius << 4) ^ (prm->marked_skip_probability > 0.f) ^ ((int64_t)E << 56) ^ ((int64_t)moments << 62) ^ ((int64_t)ctx->guide.on << 61);
        if (key != ctx->share_key) { ctx->coarse_share = 25; ctx->share_key = key; }
        const auto t_start = std::chrono::steady_clock::now();
        double t_done[MAX_SCALES] = { 0 };
        HIPCHK(ctx, hipEventRecord(ctx->ev_pyramid, ctx->stream)); // the caller's inputs are ready
        int rcs[MAX_SCALES];
        std::thread threads[MAX_SCALES];
        std::atomic<int> built[MAX_SCALES], done[MAX_SCALES]; // 0 = pending, 1 = event recorded, -1 = failed
        for (int s = 0; s < MAX_SCALES; ++s) { built[s].store(0); done[s].store(0); }
        for (int s = 1; s < nb_scales; ++s) RCCHK(work_init(ctx, ctx->extra[s], nullptr));
        auto await = [](std::atomic<int> &f) { int v; while ((v = f.load()) == 0) std::this_thread::yield(); return v; };
        for (int s = nb_scales - 1; s >= 0; --s) {
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
                        rc = build_level(ctx, col[s - 1], ns[s - 1], hs[s - 1], cv[s - 1], ws[s - 1], hh[s - 1], D, ctx->pyr[s], w->stream);
                        if (rc != BCD_HIP_OK) break;
                        if (lvp) rc = build_level_layers(ctx, lvp[s - 1], lvp[s], ns[s - 1], ws[s - 1], hh[s - 1], w->stream);
                        if (rc != BCD_HIP_OK) break;
                        if (hipEventRecord(w->ev_built, w->stream) != hipSuccess) { rc = BCD_HIP_EDEVICE; break; }
                        built[s].store(1); built_set = true;
                    }
                    rc = mono(ctx, *w, col[s], ns[s], hs[s], cv[s], ws[s], hh[s], D, prm, bcd_hip_scale_seed(prm->order_seed, s), s, out[s], lvp ? &lvp[s] : nullptr);
                    if (rc != BCD_HIP_OK) break;
                    t_done[s] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); // (mono ends with a stream synchronisation)
                    if (s < nb_scales - 1) {
                        if (await(done[s + 1]) < 0) { rc = BCD_HIP_EDEVICE; break; }
                        if (hipStreamWaitEvent(w->stream, ctx->extra[s + 1].ev_done, 0) != hipSuccess) { rc = BCD_HIP_EDEVICE; break; }
                        rc = merge_on(ctx, *w, out[s], ws[s], hh[s], out[s + 1], 3);
                        if (rc != BCD_HIP_OK) break;
                        if (lvp) rc = merge_layers_on(ctx, *w, w->lay_tmp_lo, lvp[s], ws[s], hh[s], lvp[s + 1]);
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
        for (int s = 1; s < nb_scales; ++s) threads[s].join();
        for (int s = 0; s < nb_scales; ++s) RCCHK(rcs[s]);
        if (lvp) HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream)); // (the last merge of the extra layers)
        if (nb_scales > 1 && t_done[0] > 0.0) {
            double last = 0.0;
            for (int s = 1; s < nb_scales; ++s) last = std::max(last, t_done[s]);
            const double frac = last / t_done[0];
            if (frac < 0.80) ctx->coarse_share = std::max(8, ctx->coarse_share - 2);
            else if (frac > 0.92) ctx->coarse_share = std::min(60, ctx->coarse_share + 6);
        }
        return BCD_HIP_OK;
    }
    for (int s = 1; s < nb_scales; ++s) {
        RCCHK(build_level(ctx, col[s - 1], ns[s - 1], hs[s - 1], cv[s - 1], ws[s - 1], hh[s - 1], D, ctx->pyr[s], ctx->stream));
        if (lvp) RCCHK(build_level_layers(ctx, lvp[s - 1], lvp[s], ns[s - 1], ws[s - 1], hh[s - 1], ctx->stream));
    }
    // ---- coarse to fine, one after the other
    for (int s = nb_scales - 1; s >= 0; --s) {
        RCCHK(mono(ctx, ctx->main, col[s], ns[s], hs[s], cv[s], ws[s], hh[s], D, prm, bcd_hip_scale_seed(prm->order_seed, s), s, out[s], lvp ? &lvp[s] : nullptr));
        if (s < nb_scales - 1) RCCHK(bcd_hip_merge(ctx, out[s], ws[s], hh[s], out[s + 1], 3));
        if (s < nb_scales - 1 && lvp) RCCHK(merge_layers_on(ctx, ctx->main, ctx->main.lay_tmp_lo, lvp[s], ws[s], hh[s], lvp[s + 1]));
    }
    if (lvp) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BCD_HIP_OK;
}

// the refusals a guide adds to a call; no device work: the kernel's LDS limit is a function attribute
int check_guide(bcd_hip_ctx *ctx, const bcd_hip_guide *g, int search_radius)
{
    if (!g) return bad(ctx, "null guide");
    if (g->nb_channels < 1 || g->nb_channels > BCD_HIP_GUIDE_MAX_CHANNELS) return bad(ctx, "the number of feature channels must be between 1 and 8 (BCD_HIP_GUIDE_MAX_CHANNELS)");
    if (!g->features) return bad(ctx, "null feature image");
    if (!g->floors) return bad(ctx, "null feature floors");
    bool counts = g->variances != nullptr;
    for (int k = 0; k < g->nb_channels; ++k) {
        if (!(g->floors[k] >= 0.f) || !std::isfinite(g->floors[k])) return bad(ctx, "a feature floor must be finite and not negative");
        counts = counts || g->floors[k] > 0.f;
    }
    if (!(g->threshold >= 0.f) || !std::isfinite(g->threshold)) return bad(ctx, "the feature threshold must be finite and not negative");
    if (!counts) return bad(ctx, "no feature channel can count: every floor is 0 and there are no variances");
    if (search_radius >= 0 && search_radius <= 15 && bcd_pairdist_guide_launchable(g->nb_channels, g->variances != nullptr, search_radius) != hipSuccess) {
        set_err(ctx, "the feature distance kernel cannot be launched for this number of channels and search radius (LDS)");
        return BCD_HIP_EUNSUPPORTED;
    }
    return BCD_HIP_OK;
}

// one level of a feature pyramid from the W x H level above it: the features are downscale_avg of the finer ones, the variances (d_var null: none)
// downscale_avg of the finer ones times 0.25f (the variance of a mean of four)
int guide_build_level(bcd_hip_ctx *ctx, const float *d_feat, const float *d_var, int W, int H, int F, float *d_feat_out, float *d_var_out, hipStream_t st)
{
    HIPCHK(ctx, bcd_launch_downscale(1, d_feat, W, H, F, d_feat_out, st));
    if (!d_var) return BCD_HIP_OK;
    HIPCHK(ctx, bcd_launch_downscale(1, d_var, W, H, F, d_var_out, st));
    HIPCHK(ctx, bcd_launch_scale_inplace(d_var_out, 0.25f, (int64_t)(W / 2) * (H / 2) * F, st));
    return BCD_HIP_OK;
}

// the levels of the guide's pyramid by guide_build_level; threshold and floors are those of level 0.  On the context's stream: every scale's stream waits for
// what that stream holds (ev_pyramid)
int guide_begin(bcd_hip_ctx *ctx, const bcd_hip_guide *g, const float *d_features, const float *d_variances, int W, int H, int nb_scales)
{
    const int F = g->nb_channels;
    auto &G = ctx->guide;
    G.on = false;
    G.F = F; G.tau = g->threshold;
    for (int k = 0; k < BCD_GUIDE_MAX_CHANNELS; ++k) G.floors[k] = k < F ? g->floors[k] : 0.f;
    for (int s = 0; s < MAX_SCALES; ++s) G.f[s] = G.v[s] = nullptr;
    G.f[0] = d_features; G.v[0] = d_variances;
    for (int s = 1, ws = W, hs = H; s < nb_scales && s < MAX_SCALES; ++s) {
        const size_t np = (size_t)(ws / 2) * (hs / 2);
        RCCHK(ensure(ctx, ctx->guide_pyr[s][0], np * F * sizeof(float)));
        if (d_variances) RCCHK(ensure(ctx, ctx->guide_pyr[s][1], np * F * sizeof(float)));
        RCCHK(guide_build_level(ctx, G.f[s - 1], G.v[s - 1], ws, hs, F, (float *)ctx->guide_pyr[s][0].p, (float *)ctx->guide_pyr[s][1].p, ctx->stream));
        G.f[s] = (const float *)ctx->guide_pyr[s][0].p;
        if (d_variances) G.v[s] = (const float *)ctx->guide_pyr[s][1].p;
        ws /= 2; hs /= 2;
    }
    G.on = true;
    return BCD_HIP_OK;
}

// the refusals of bcd_hip_denoise_layers (and of bcd_hip_denoise_layers_keep): everything is checked before any device work
// (no_hist: the call of bcd_hip_denoise_moments -- there is no histogram image, d_hist and D are not looked at)
int check_layers_call(bcd_hip_ctx *ctx, const float *d_ns, const float *d_hist, int W, int H, int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer *layers,
                      int nb_layers, bool no_hist)
{
    if (!d_ns || (!d_hist && !no_hist)) return bad(ctx, "null image pointer");
    if (!layers) return bad(ctx, "null layer list");
    if (nb_layers < 1 || nb_layers > BCD_HIP_MAX_LAYERS) return bad(ctx, "the number of layers must be between 1 and 16 (BCD_HIP_MAX_LAYERS)");
    for (int k = 0; k < nb_layers; ++k)
        if (!layers[k].d_colors || !layers[k].d_covariances || !layers[k].d_out) return bad(ctx, "null image pointer in a layer");
    RCCHK(check_params(ctx, W, H, no_hist ? 1 : D, prm));
    if (nb_scales < 1 || nb_scales > MAX_SCALES) return bad(ctx, "bad number of scales");
    for (int s = 1, ws = W, hs = H; s < nb_scales; ++s) {
        ws /= 2; hs /= 2;
        if (ws < 2 * prm->patch_radius + 1 || hs < 2 * prm->patch_radius + 1) return bad(ctx, "too many scales for this image size");
    }
    {
        const size_t f1 = (size_t)W * H * sizeof(float), no = 3 * f1; // (one float per pixel, an output)
        for (int k = 0; k < nb_layers; ++k) {
            const float *o = layers[k].d_out;
            if (bytes_overlap(o, no, d_ns, f1) || (!no_hist && bytes_overlap(o, no, d_hist, f1 * D))) return bad(ctx, "a layer's output overlaps the sample counts or the histograms");
            for (int j = 0; j < nb_layers; ++j) {
                if (bytes_overlap(o, no, layers[j].d_colors, 3 * f1) || bytes_overlap(o, no, layers[j].d_covariances, 6 * f1))
                    return bad(ctx, "a layer's output overlaps an input image");
                if (j != k && bytes_overlap(o, no, layers[j].d_out, no)) return bad(ctx, "two layers share (part of) an output image");
            }
        }
    }
    return BCD_HIP_OK;
}

extern "C" {

int bcd_hip_denoise(bcd_hip_ctx *ctx, const float *d_colors, const float *d_ns, const float *d_hist, const float *d_cov,
                    int W, int H, int D, int nb_scales, const bcd_hip_params *prm, float *d_out)
{
    return denoise_impl(ctx, d_colors, d_ns, d_hist, d_cov, W, H, D, nb_scales, prm, d_out, nullptr);
}

int bcd_hip_denoise_layers(bcd_hip_ctx *ctx, const float *d_ns, const float *d_hist, int W, int H, int D, int nb_scales, const bcd_hip_params *prm,
                           const bcd_hip_layer *layers, int nb_layers)
{
    if (!ctx) return BCD_HIP_EINVAL;
    RCCHK(check_layers_call(ctx, d_ns, d_hist, W, H, D, nb_scales, prm, layers, nb_layers)); // everything is checked before any device work
    return denoise_layers_checked(ctx, d_ns, d_hist, W, H, D, nb_scales, prm, layers, nb_layers);
}

} // extern "C"

// bcd_hip_denoise_layers behind its checks (bcd_hip_denoise_moments arrives here with checks of its own, ctx->moments set, no histograms and D = 0)
int denoise_layers_checked(bcd_hip_ctx *ctx, const float *d_ns, const float *d_hist, int W, int H, int D, int nb_scales, const bcd_hip_params *prm,
                           const bcd_hip_layer *layers, int nb_layers)
{
    LayerView lv;
    lv.n = nb_layers - 1;
    for (int k = 1; k < nb_layers; ++k) { lv.col[k - 1] = layers[k].d_colors; lv.cov[k - 1] = layers[k].d_covariances; lv.out[k - 1] = layers[k].d_out; }
    memset(ctx->layer_spectral, 0, sizeof(ctx->layer_spectral));
    ctx->layer_count = 0;
    RCCHK(denoise_impl(ctx, layers[0].d_colors, d_ns, d_hist, layers[0].d_covariances, W, H, D, nb_scales, prm, layers[0].d_out, &lv));
    if (lv.n == 0) for (int s = 0; s < nb_scales; ++s) ctx->layer_spectral[s][0] = ctx->stats[s].spectral_inverses;
    ctx->layer_count = nb_layers;
    return BCD_HIP_OK;
}

extern "C" {

int bcd_hip_layer_spectral_inverses(const bcd_hip_ctx *ctx, int scale, int layer, int32_t *count)
{
    if (!ctx || !count || scale < 0 || scale >= MAX_SCALES || layer < 0 || layer >= ctx->layer_count) return BCD_HIP_EINVAL;
    *count = ctx->layer_spectral[scale][layer];
    return BCD_HIP_OK;
}

int bcd_hip_denoise_begin(bcd_hip_ctx *ctx, const float *d_colors, const float *d_ns, const float *d_hist, const float *d_cov,
                          int W, int H, int D, int nb_scales, const bcd_hip_params *prm, float *d_out)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_colors || !d_ns || !d_hist || !d_cov || !d_out) return bad(ctx, "null image pointer");
    RCCHK(check_params(ctx, W, H, D, prm));
    if (nb_scales < 1 || nb_scales > MAX_SCALES) return bad(ctx, "bad number of scales");
    bcd_hip_ctx::Async &a = ctx->async;
    std::unique_lock<std::mutex> lk(a.mu);
    if (a.in_flight) return bad(ctx, "a frame of this context is already in flight: call bcd_hip_denoise_wait first");
    a.col = d_colors; a.ns = d_ns; a.hist = d_hist; a.cov = d_cov; a.out = d_out; a.W = W; a.H = H; a.D = D; a.S = nb_scales; a.prm = *prm;
    a.has_job = true; a.in_flight = true; a.rc = BCD_HIP_OK;
    if (!a.th.joinable())
        a.th = std::thread([ctx]() {
            bcd_hip_ctx::Async &j = ctx->async;
            std::unique_lock<std::mutex> l(j.mu);
            for (;;) {
                j.cv.wait(l, [&]() { return j.has_job || j.quit; });
                if (!j.has_job) return; // (quit)
                j.has_job = false;
                l.unlock();
                const int rc = bcd_hip_denoise(ctx, j.col, j.ns, j.hist, j.cov, j.W, j.H, j.D, j.S, &j.prm, j.out); // (synchronises the context's streams)
                l.lock();
                j.rc = rc;
                j.in_flight = false;
                j.cv.notify_all();
            }
        });
    lk.unlock();
    a.cv.notify_all();
    return BCD_HIP_OK;
}

int bcd_hip_denoise_wait(bcd_hip_ctx *ctx)
{
    if (!ctx) return BCD_HIP_EINVAL;
    bcd_hip_ctx::Async &a = ctx->async;
    std::unique_lock<std::mutex> lk(a.mu);
    a.cv.wait(lk, [&]() { return !a.in_flight; });
    return a.rc;
}

int bcd_hip_denoise_band(bcd_hip_ctx *ctx, const float *d_colors, const float *d_ns, const float *d_hist, const float *d_cov,
                         int W, int H, int D, int main_row_begin, int main_row_end, const bcd_hip_params *prm, uint32_t order_seed,
                         float *d_sum, int32_t *d_count)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_colors || !d_ns || !d_hist || !d_cov || !d_sum || !d_count) return bad(ctx, "null image pointer");
    RCCHK(check_params(ctx, W, H, D, prm));
    if (main_row_begin < 0 || main_row_end > H || main_row_begin > main_row_end) return bad(ctx, "bad main row range");
    DEVICE_GUARD(ctx);
    return mono_accumulate(ctx, ctx->main, d_colors, d_ns, d_hist, d_cov, W, H, D, main_row_begin, main_row_end, prm, order_seed, 0, d_sum, d_count);
}

int bcd_hip_denoise_bands(bcd_hip_ctx *ctx, const bcd_hip_band_job *jobs, int njobs, const bcd_hip_params *prm)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!jobs || njobs < 1 || njobs > MAX_SCALES) return bad(ctx, "bad job list");
    for (int i = 0; i < njobs; ++i) {
        const bcd_hip_band_job &j = jobs[i];
        if (!j.d_colors || !j.d_nsamples || !j.d_histograms || !j.d_covariances || !j.d_sum || !j.d_count) return bad(ctx, "null image pointer");
        RCCHK(check_params(ctx, j.W, j.H, j.D, prm));
        if (j.main_row_begin < 0 || j.main_row_end > j.H || j.main_row_begin > j.main_row_end) return bad(ctx, "bad main row range");
    }
    DEVICE_GUARD(ctx);
    if (!ctx->concurrent_scales || njobs == 1) {
        for (int i = 0; i < njobs; ++i) {
            const bcd_hip_band_job &j = jobs[i];
            RCCHK(mono_accumulate(ctx, ctx->main, j.d_colors, j.d_nsamples, j.d_histograms, j.d_covariances, j.W, j.H, j.D, j.main_row_begin,
                                  j.main_row_end, prm, j.order_seed, i, j.d_sum, j.d_count));
        }
        return BCD_HIP_OK;
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev_pyramid, ctx->stream)); // inputs were produced on the context's stream
    int rcs[MAX_SCALES];
    std::thread threads[MAX_SCALES];
    for (int i = 1; i < njobs; ++i) RCCHK(work_init(ctx, ctx->extra[i], nullptr));
    for (int i = njobs - 1; i >= 0; --i) {
        Work *w = i == 0 ? &ctx->main : &ctx->extra[i];
        const bcd_hip_band_job j = jobs[i];
        rcs[i] = BCD_HIP_OK;
        auto job = [=, &rcs]() {
            if (hipSetDevice(ctx->device) != hipSuccess) { rcs[i] = BCD_HIP_EDEVICE; return; }
            if (i != 0 && hipStreamWaitEvent(w->stream, ctx->ev_pyramid, 0) != hipSuccess) { rcs[i] = BCD_HIP_EDEVICE; return; }
            rcs[i] = mono_accumulate(ctx, *w, j.d_colors, j.d_nsamples, j.d_histograms, j.d_covariances, j.W, j.H, j.D, j.main_row_begin,
                                     j.main_row_end, prm, j.order_seed, i, j.d_sum, j.d_count);
            if (rcs[i] == BCD_HIP_OK && i != 0 && hipEventRecord(w->ev_done, w->stream) != hipSuccess) rcs[i] = BCD_HIP_EDEVICE;
        };
        if (i == 0) job(); else threads[i] = std::thread(job);
    }
    for (int i = 1; i < njobs; ++i) threads[i].join();
    for (int i = 0; i < njobs; ++i) RCCHK(rcs[i]);
    for (int i = 1; i < njobs; ++i) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->extra[i].ev_done, 0));
    return BCD_HIP_OK;
}

int bcd_hip_set_progress_callback(bcd_hip_ctx *ctx, bcd_hip_progress_fn fn, void *user)
{
    if (!ctx) return BCD_HIP_EINVAL;
    std::lock_guard<std::mutex> lock(ctx->progress_mutex);
    ctx->progress_fn = fn;
    ctx->progress_user = user;
    return BCD_HIP_OK;
}

// ---- stages -------------------------------------------------------------------------------------------
int bcd_hip_pixel_cov(bcd_hip_ctx *ctx, const float *d_cov, const float *d_ns, int W, int H, float *d_out)
{
    if (!ctx || !d_cov || !d_ns || !d_out || W <= 0 || H <= 0) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_pixel_cov(d_cov, d_ns, (int64_t)W * H, d_out, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_scale_begin(bcd_hip_ctx *ctx, const float *d_cov, const float *d_ns, int W, int H, float *d_pixcov, float *d_sum, int32_t *d_count)
{
    if (!ctx || !d_cov || !d_ns || !d_pixcov || !d_sum || !d_count || W <= 0 || H <= 0) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    Work &wk = ctx->main;
    constexpr size_t LINE_INTS = (size_t)BCD_CNT_LINES * BCD_CNT_STRIDE;
    RCCHK(ensure(ctx, wk.counters, sizeof(Counters)));
    RCCHK(ensure(ctx, wk.cnt_lines, ROUND_BATCH * LINE_INTS * sizeof(int)));
    RCCHK(ensure(ctx, wk.work_q, BCD_WORK_INTS * sizeof(int32_t)));
    HIPCHK(ctx, bcd_launch_pixel_cov_clear(d_cov, d_ns, (int64_t)W * H, d_pixcov, d_sum, d_count, wk.stream));
    HIPCHK(ctx, bcd_launch_scale_begin((int *)wk.counters.p, COUNTER_WORDS, -1, -1, (int *)wk.cnt_lines.p, (int)(ROUND_BATCH * LINE_INTS), (int *)wk.work_q.p, BCD_WORK_INTS, wk.stream));
    // ("clean" = zero because nobody has used it since: every user of these buffers takes the note and clears it)
    wk.clean_flags = wk.clean_lines = wk.clean_dc = wk.clean_wq = true;
    wk.planes.ready = false;
    return BCD_HIP_OK;
}

int bcd_hip_similarity_masks(bcd_hip_ctx *ctx, const float *d_hist, const float *d_ns, int W, int H, int D, int w, int b, float tau,
                             uint32_t *d_mask, int32_t *d_count)
{
    if (!ctx || !d_hist || !d_ns || !d_mask || !d_count) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    bcd_hip_params p; bcd_hip_default_params(&p); p.patch_radius = w; p.search_radius = b;
    RCCHK(check_params(ctx, W, H, D, &p));
    return similarity(ctx, ctx->main, d_hist, d_ns, W, H, D, w, b, tau, d_mask, d_count);
}

int bcd_hip_similarity_masks_deferred(bcd_hip_ctx *ctx, const float *d_hist, const float *d_ns, int W, int H, int D, int w, int b, float tau,
                                      uint32_t *d_mask, int32_t *d_count)
{
    if (!ctx || !d_hist || !d_ns || !d_mask || !d_count) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    bcd_hip_params p; bcd_hip_default_params(&p); p.patch_radius = w; p.search_radius = b;
    RCCHK(check_params(ctx, W, H, D, &p));
    return similarity(ctx, ctx->main, d_hist, d_ns, W, H, D, w, b, tau, d_mask, d_count, 2);
}

int bcd_hip_similarity_masks_verdict(bcd_hip_ctx *ctx, int *redo)
{
    if (!ctx || !redo) return BCD_HIP_EINVAL;
    *redo = similarity_redo_mode(ctx->main) != 0 ? 1 : 0; // (also keeps the workspace's memory of non-uniform sample counts)
    return BCD_HIP_OK;
}

int bcd_hip_similarity_masks_exact(bcd_hip_ctx *ctx, const float *d_hist, const float *d_ns, int W, int H, int D, int w, int b, float tau,
                                   uint32_t *d_mask, int32_t *d_count)
{
    if (!ctx || !d_hist || !d_ns || !d_mask || !d_count) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    bcd_hip_params p; bcd_hip_default_params(&p); p.patch_radius = w; p.search_radius = b;
    RCCHK(check_params(ctx, W, H, D, &p));
    return similarity(ctx, ctx->main, d_hist, d_ns, W, H, D, w, b, tau, d_mask, d_count, 1);
}

int bcd_hip_similarity_last_path(bcd_hip_ctx *ctx, int32_t *path, int32_t *borderline, int32_t *capacity)
{
    if (!ctx || !path || !borderline || !capacity) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    Work &wk = ctx->main;
    HIPCHK(ctx, hipStreamSynchronize(wk.stream)); // (the flags' copies are the last thing a deferred pass enqueues)
    const bool fast = wk.border_capacity > 0 && wk.h_counters;
    *path = fast ? (wk.ratio_used ? 2 : 1) : 0;
    *borderline = fast ? wk.h_counters->flags.borderline : 0;
    *capacity = fast ? wk.border_capacity : 0;
    return BCD_HIP_OK;
}

int bcd_hip_window_distances(bcd_hip_ctx *ctx, const float *d_hist, const float *d_ns, int W, int H, int D, int w, int b,
                             int line, int col, float *h_out)
{
    if (!ctx || !d_hist || !d_ns || !h_out) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    bcd_hip_params p; bcd_hip_default_params(&p); p.patch_radius = w; p.search_radius = b;
    RCCHK(check_params(ctx, W, H, D, &p));
    if (line < w || line > H - 1 - w || col < w || col > W - 1 - w) return bad(ctx, "not a main pixel");
    const size_t npix = (size_t)W * H;
    const int nd = bcd_delta_count(b), n = (2 * b + 1) * (2 * b + 1);
    RCCHK(ensure(ctx, ctx->main.T, npix * nd * sizeof(float)));
    RCCHK(ensure(ctx, ctx->main.Cn, npix * nd));
    RCCHK(ensure(ctx, ctx->tmp_lo, n * sizeof(float)));
    HIPCHK(ctx, bcd_launch_pairdist(d_hist, d_ns, W, H, D, b, (float *)ctx->main.T.p, (uint8_t *)ctx->main.Cn.p, 0, nullptr, 0.f, ctx->stream));
    HIPCHK(ctx, bcd_launch_window_distances((const float *)ctx->main.T.p, (const uint8_t *)ctx->main.Cn.p, W, H, w, b, line, col, (float *)ctx->tmp_lo.p, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(h_out, ctx->tmp_lo.p, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BCD_HIP_OK;
}

namespace {
// the refusals the two stage calls of the moment selection share
int check_moments_stage(bcd_hip_ctx *ctx, int W, int H, int w, int b, float var_floor)
{
    if (!(var_floor >= 0.f) || !std::isfinite(var_floor)) return bad(ctx, "the variance floor must be finite and not negative");
    bcd_hip_params p; bcd_hip_default_params(&p); p.patch_radius = w; p.search_radius = b;
    return check_params(ctx, W, H, 1, &p);
}
} // namespace

int bcd_hip_similarity_masks_moments(bcd_hip_ctx *ctx, const float *d_colors, const float *d_pixcov, int W, int H, int w, int b, float tau, float var_floor,
                                     uint32_t *d_mask, int32_t *d_count)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_colors || !d_pixcov || !d_mask || !d_count) return bad(ctx, "bad argument");
    RCCHK(check_moments_stage(ctx, W, H, w, b, var_floor));
    DEVICE_GUARD(ctx);
    return similarity_moments(ctx, ctx->main, d_colors, d_pixcov, W, H, w, b, tau, var_floor, d_mask, d_count);
}

int bcd_hip_window_distances_moments(bcd_hip_ctx *ctx, const float *d_colors, const float *d_pixcov, int W, int H, int w, int b, float var_floor, int line, int col,
                                     float *h_out)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_colors || !d_pixcov || !h_out) return bad(ctx, "bad argument");
    RCCHK(check_moments_stage(ctx, W, H, w, b, var_floor));
    if (line < w || line > H - 1 - w || col < w || col > W - 1 - w) return bad(ctx, "not a main pixel");
    DEVICE_GUARD(ctx);
    const size_t npix = (size_t)W * H;
    const int nd = bcd_delta_count(b), n = (2 * b + 1) * (2 * b + 1);
    RCCHK(ensure(ctx, ctx->main.T, npix * nd * sizeof(float)));
    RCCHK(ensure(ctx, ctx->main.Cn, count_plane_bytes(npix, nd)));
    RCCHK(ensure(ctx, ctx->tmp_lo, n * sizeof(float)));
    ctx->main.planes.ready = false; // (the workspace's planes are overwritten)
    HIPCHK(ctx, bcd_launch_pairdist_moments(d_colors, d_pixcov, W, H, b, var_floor, (float *)ctx->main.T.p, (uint8_t *)ctx->main.Cn.p, ctx->stream));
    HIPCHK(ctx, bcd_launch_window_distances((const float *)ctx->main.T.p, (const uint8_t *)ctx->main.Cn.p, W, H, w, b, line, col, (float *)ctx->tmp_lo.p, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(h_out, ctx->tmp_lo.p, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BCD_HIP_OK;
}

namespace {
// the refusals the stage calls of the feature gate share
static int check_guide_stage(bcd_hip_ctx *ctx, const bcd_hip_guide *g, int W, int H, int w, int b)
{
    bcd_hip_params p; bcd_hip_default_params(&p); p.patch_radius = w; p.search_radius = b;
    RCCHK(check_params(ctx, W, H, BCD_HIP_GUIDE_MAX_CHANNELS, &p)); // (indices of W*H*F floats stay below 2^31 for every F)
    return check_guide(ctx, g, b);
}
} // namespace

int bcd_hip_similarity_masks_guide(bcd_hip_ctx *ctx, const bcd_hip_guide *g, int W, int H, int w, int b, uint32_t *d_mask, int32_t *d_count)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_mask || !d_count) return bad(ctx, "bad argument");
    RCCHK(check_guide_stage(ctx, g, W, H, w, b));
    DEVICE_GUARD(ctx);
    return guide_masks(ctx, ctx->main, g->features, g->variances, g->nb_channels, g->floors, g->threshold, W, H, w, b, d_mask, d_count);
}

int bcd_hip_window_distances_guide(bcd_hip_ctx *ctx, const bcd_hip_guide *g, int W, int H, int w, int b, int line, int col, float *h_out)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!h_out) return bad(ctx, "bad argument");
    RCCHK(check_guide_stage(ctx, g, W, H, w, b));
    if (line < w || line > H - 1 - w || col < w || col > W - 1 - w) return bad(ctx, "not a main pixel");
    DEVICE_GUARD(ctx);
    const size_t npix = (size_t)W * H;
    const int nd = bcd_delta_count(b), n = (2 * b + 1) * (2 * b + 1);
    RCCHK(ensure(ctx, ctx->main.T, npix * nd * sizeof(float)));
    RCCHK(ensure(ctx, ctx->main.Cn, count_plane_bytes(npix, nd)));
    RCCHK(ensure(ctx, ctx->tmp_lo, n * sizeof(float)));
    ctx->main.planes.ready = false; // (the workspace's planes are overwritten)
    HIPCHK(ctx, bcd_launch_pairdist_guide(g->features, g->variances, g->nb_channels, g->floors, W, H, b, (float *)ctx->main.T.p, (uint8_t *)ctx->main.Cn.p, ctx->stream));
    HIPCHK(ctx, bcd_launch_window_distances((const float *)ctx->main.T.p, (const uint8_t *)ctx->main.Cn.p, W, H, w, b, line, col, (float *)ctx->tmp_lo.p, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(h_out, ctx->tmp_lo.p, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_gate_masks(bcd_hip_ctx *ctx, uint32_t *d_mask, int32_t *d_count, const uint32_t *d_gate, int W, int H, int b)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_mask || !d_count || !d_gate) return bad(ctx, "bad argument");
    if (W <= 0 || H <= 0 || (int64_t)W * H >= (1ll << 31)) return bad(ctx, "empty input image");
    if (b < 0) return bad(ctx, "negative radius");
    if (b > 15) { set_err(ctx, "search radius > 15 is not supported"); return BCD_HIP_EUNSUPPORTED; }
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_gate_masks(d_mask, d_gate, d_count, W, H, b, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_active_set(bcd_hip_ctx *ctx, const uint32_t *d_mask, const int32_t *d_count, int W, int H, int w, int b,
                       int main_row_begin, int main_row_end, float skip_probability, int random_order, uint32_t seed,
                       uint8_t *d_state, int32_t *rounds)
{
    if (!ctx || !d_mask || !d_count || !d_state) return bad(ctx, "bad argument");
    if (W <= 0 || H <= 0 || w < 0 || b < 0) return bad(ctx, "marking: empty image or negative radius"); // (before any launch: a grid of no blocks is a launch error)
    DEVICE_GUARD(ctx);
    return active_set(ctx, ctx->main, d_mask, d_count, W, H, w, b, main_row_begin, main_row_end, skip_probability, random_order, seed, d_state, rounds);
}

int bcd_hip_active_init(bcd_hip_ctx *ctx, const int32_t *d_count, int W, int H, int w, int main_row_begin, int main_row_end,
                        float skip_probability, uint32_t seed, int row_offset, uint8_t *d_state)
{
    if (!ctx || !d_count || !d_state) return bad(ctx, "bad argument");
    if (W <= 0 || H <= 0 || w < 0) return bad(ctx, "marking: empty image or negative radius");
    DEVICE_GUARD(ctx);
    // (ctx->stream IS ctx->main.stream -- work_init(ctx, ctx->main, ctx->stream) in bcd_hip_ctx_create --: the steps that follow are ordered behind this launch)
    HIPCHK(ctx, bcd_launch_active_init(d_count, W, H, w, main_row_begin, main_row_end, skip_probability, seed, row_offset, d_state, ctx->stream));
    ctx->main.dep_ready = false;
    return BCD_HIP_OK;
}

int bcd_hip_active_step(bcd_hip_ctx *ctx, const uint32_t *d_mask, const int32_t *d_count, int W, int H, int w, int b, int main_row_begin,
                        int main_row_end, int random_order, uint32_t seed, int row_offset, int first_pass, uint8_t *d_state, int32_t *undecided)
{
    if (!ctx || !d_mask || !d_count || !d_state || !undecided) return bad(ctx, "bad argument");
    if (W <= 0 || H <= 0 || w < 0 || b < 0) return bad(ctx, "marking: empty image or negative radius");
    DEVICE_GUARD(ctx);
    int u = 0;
    // the dependency lists extracted by the first step after bcd_hip_active_init stay valid for the following steps of the same
    // marking problem on the same buffers (masks and counts do not change; a pixel that is still undecided keeps its list)
    RCCHK(active_step(ctx, ctx->main, d_mask, d_count, W, H, w, b, main_row_begin, main_row_end, random_order, seed, row_offset, first_pass != 0,
                      d_state, &u, nullptr));
    *undecided = u;
    return BCD_HIP_OK;
}

int bcd_hip_active_step_enqueue(bcd_hip_ctx *ctx, const uint32_t *d_mask, const int32_t *d_count, int W, int H, int w, int b, int main_row_begin,
                                int main_row_end, int random_order, uint32_t seed, int row_offset, uint8_t *d_state, int64_t *d_total, int with_verdict)
{
    if (!ctx || !d_mask || !d_count || !d_state) return bad(ctx, "bad argument");
    if (W <= 0 || H <= 0 || w < 0 || b < 0) return bad(ctx, "marking: empty image or negative radius");
    DEVICE_GUARD(ctx);
    static_assert(sizeof(long long) == sizeof(int64_t), "64-bit counters");
    return active_step_enqueue(ctx, ctx->main, d_mask, d_count, W, H, w, b, main_row_begin, main_row_end, random_order, seed, row_offset, d_state,
                               reinterpret_cast<long long *>(d_total), with_verdict != 0);
}

int bcd_hip_active_step_collect(bcd_hip_ctx *ctx, int32_t *undecided, int32_t *launches)
{
    if (!ctx || !undecided) return BCD_HIP_EINVAL;
    int u = 0, n = 0;
    active_step_collect(ctx->main, &u, &n);
    *undecided = u;
    if (launches) *launches = n;
    return BCD_HIP_OK;
}

int bcd_hip_bayes_accumulate(bcd_hip_ctx *ctx, const float *d_colors, const float *d_pixcov, const uint32_t *d_mask,
                             const int32_t *d_nsim, const uint8_t *d_state, int W, int H, int w, int b, float min_eig,
                             float *d_sum, int32_t *d_count)
{
    if (!ctx || !d_colors || !d_pixcov || !d_mask || !d_nsim || !d_state || !d_sum || !d_count) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    return bayes(ctx, ctx->main, d_colors, d_pixcov, d_mask, d_nsim, d_state, W, H, w, b, min_eig, d_sum, d_count);
}

int bcd_hip_bayes_accumulate_layers(bcd_hip_ctx *ctx, const bcd_hip_stage_layer *layers, int nb_layers, const uint32_t *d_mask, const int32_t *d_nsim,
                                    const uint8_t *d_state, int W, int H, int w, int b, float min_eig, int32_t *d_count, int32_t *h_redo)
{
    if (!ctx) return BCD_HIP_EINVAL;
    // ---- everything is checked before any device work (as bcd_hip_denoise_layers)
    if (!d_mask || !d_nsim || !d_state || !d_count) return bad(ctx, "null image pointer");
    if (!layers) return bad(ctx, "null layer list");
    if (nb_layers < 1 || nb_layers > BCD_HIP_MAX_LAYERS) return bad(ctx, "the number of layers must be between 1 and 16 (BCD_HIP_MAX_LAYERS)");
    for (int k = 0; k < nb_layers; ++k)
        if (!layers[k].d_colors || !layers[k].d_pixel_cov || !layers[k].d_sum) return bad(ctx, "null image pointer in a layer");
    bcd_hip_params p; bcd_hip_default_params(&p); p.patch_radius = w; p.search_radius = b;
    RCCHK(check_params(ctx, W, H, 1, &p));
    {
        const size_t npix = (size_t)W * H;
        const size_t words = ((size_t)(2 * b + 1) * (2 * b + 1) + 31) / 32;
        for (int k = 0; k < nb_layers; ++k) {
            const float *o = layers[k].d_sum;
            const size_t no = npix * 3 * sizeof(float);
            if (bytes_overlap(o, no, d_mask, npix * words * 4) || bytes_overlap(o, no, d_nsim, npix * 4) || bytes_overlap(o, no, d_state, npix) ||
                bytes_overlap(o, no, d_count, npix * 4))
                return bad(ctx, "a layer's sum image overlaps the selection or the count image");
            for (int j = 0; j < nb_layers; ++j) {
                if (bytes_overlap(o, no, layers[j].d_colors, npix * 3 * sizeof(float)) || bytes_overlap(o, no, layers[j].d_pixel_cov, npix * 6 * sizeof(float)))
                    return bad(ctx, "a layer's sum image overlaps an input image");
                if (j != k && bytes_overlap(o, no, layers[j].d_sum, no)) return bad(ctx, "two layers share (part of) a sum image");
            }
        }
    }
    DEVICE_GUARD(ctx);
    Work &wk = ctx->main;
    RCCHK(bayes(ctx, wk, layers[0].d_colors, layers[0].d_pixel_cov, d_mask, d_nsim, d_state, W, H, w, b, min_eig, layers[0].d_sum, d_count));
    HIPCHK(ctx, hipStreamSynchronize(wk.stream)); // (the list lengths and the first layer's redo counter are on the host: what mono_accumulate hands over)
    int32_t spectral[BCD_MAX_LAYERS] = { wk.h_counters->lists.spectral };
    if (nb_layers > 1) {
        LayerView lv;
        lv.n = nb_layers - 1;
        const float *pixcov[BCD_MAX_LAYERS];
        float *sum[BCD_MAX_LAYERS];
        for (int k = 1; k < nb_layers; ++k) { lv.col[k - 1] = layers[k].d_colors; lv.cov[k - 1] = nullptr; lv.out[k - 1] = nullptr; pixcov[k - 1] = layers[k].d_pixel_cov; sum[k - 1] = layers[k].d_sum; }
        RCCHK(layers_follow(ctx, wk, lv, d_mask, d_nsim, d_state, pixcov, sum, W, H, w, b, min_eig, d_count, spectral));
    }
    if (h_redo) for (int k = 0; k < nb_layers; ++k) h_redo[k] = spectral[k];
    return BCD_HIP_OK;
}

namespace {
int layer_list_ok(bcd_hip_ctx *ctx, const void *const *a, const void *const *b, int nb_layers)
{
    if (!a || !b) return bad(ctx, "null layer list");
    if (nb_layers < 1 || nb_layers > BCD_HIP_MAX_LAYERS) return bad(ctx, "the number of layers must be between 1 and 16 (BCD_HIP_MAX_LAYERS)");
    for (int k = 0; k < nb_layers; ++k)
        if (!a[k] || !b[k]) return bad(ctx, "null image pointer in a layer");
    return BCD_HIP_OK;
}
} // namespace

int bcd_hip_layers_pixel_cov(bcd_hip_ctx *ctx, const float *const *d_cov, int nb_layers, const float *d_ns, int W, int H, float *d_pixcov, float *d_sum)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_ns || !d_pixcov || !d_sum || W <= 0 || H <= 0) return bad(ctx, "bad argument");
    RCCHK(layer_list_ok(ctx, (const void *const *)d_cov, (const void *const *)d_cov, nb_layers));
    DEVICE_GUARD(ctx);
    BcdLayerTable t = {};
    for (int k = 0; k < nb_layers; ++k) t.a[k] = d_cov[k];
    HIPCHK(ctx, bcd_launch_layers_pixel_cov_clear(t, nb_layers, d_ns, (int64_t)W * H, d_pixcov, d_sum, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_layers_finalize(bcd_hip_ctx *ctx, const float *const *d_sum, float *const *d_out, int nb_layers, const int32_t *d_count, int64_t npix)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_count || npix <= 0) return bad(ctx, "bad argument");
    RCCHK(layer_list_ok(ctx, (const void *const *)d_sum, (const void *const *)d_out, nb_layers));
    DEVICE_GUARD(ctx);
    BcdLayerTable t = {};
    for (int k = 0; k < nb_layers; ++k) { t.a[k] = d_sum[k]; t.o[k] = d_out[k]; }
    HIPCHK(ctx, bcd_launch_layers_finalize(t, nb_layers, d_count, npix, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_layers_downscale_avg(bcd_hip_ctx *ctx, const float *const *d_in, float *const *d_out, int nb_layers, int W, int H)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (W < 2 || H < 2) return bad(ctx, "bad argument");
    RCCHK(layer_list_ok(ctx, (const void *const *)d_in, (const void *const *)d_out, nb_layers));
    DEVICE_GUARD(ctx);
    BcdLayerTable t = {};
    for (int k = 0; k < nb_layers; ++k) { t.a[k] = d_in[k]; t.o[k] = d_out[k]; }
    HIPCHK(ctx, bcd_launch_layers_downscale_avg(t, nb_layers, W, H, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_layers_downscale_cov(bcd_hip_ctx *ctx, const float *const *d_cov, float *const *d_out, int nb_layers, const float *d_ns, int W, int H)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_ns || W < 2 || H < 2) return bad(ctx, "bad argument");
    RCCHK(layer_list_ok(ctx, (const void *const *)d_cov, (const void *const *)d_out, nb_layers));
    DEVICE_GUARD(ctx);
    BcdLayerTable t = {};
    for (int k = 0; k < nb_layers; ++k) { t.a[k] = d_cov[k]; t.o[k] = d_out[k]; }
    HIPCHK(ctx, bcd_launch_layers_downscale_cov(t, nb_layers, d_ns, W, H, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_layers_merge(bcd_hip_ctx *ctx, float *const *d_hi, const float *const *d_lo, int nb_layers, int W, int H)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (W < 2 || H < 2) return bad(ctx, "bad argument");
    RCCHK(layer_list_ok(ctx, (const void *const *)d_hi, (const void *const *)d_lo, nb_layers));
    DEVICE_GUARD(ctx);
    LayerView hi, lo;
    hi.n = lo.n = nb_layers;
    for (int k = 0; k < nb_layers; ++k) { hi.out[k] = d_hi[k]; lo.out[k] = const_cast<float *>(d_lo[k]); }
    return merge_layers_on(ctx, ctx->main, ctx->main.lay_tmp_lo, hi, W, H, lo); // (the frame's own two launches)
}

int bcd_hip_bayes_last_redo_count(bcd_hip_ctx *ctx, int32_t *count)
{
    if (!ctx || !count) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream)); // (the counter's copy is the last thing bayes() enqueues)
    *count = ctx->main.h_counters->lists.spectral;
    return BCD_HIP_OK;
}

int bcd_hip_bayes_accumulate_rows(bcd_hip_ctx *ctx, const float *d_colors, const float *d_pixcov, const uint32_t *d_mask,
                                  const int32_t *d_nsim, const uint8_t *d_state, int W, int H, int w, int b, float min_eig,
                                  float *d_sum, int32_t *d_count, int row_begin, int row_end, const int64_t *d_skip_if, const int64_t *h_skip_if, int *skipped)
{
    if (!ctx || !d_colors || !d_pixcov || !d_mask || !d_nsim || !d_state || !d_sum || !d_count) return bad(ctx, "bad argument");
    if (d_skip_if && (!h_skip_if || !skipped)) return bad(ctx, "a speculative estimate needs the host copy of its word and a place for the verdict");
    DEVICE_GUARD(ctx);
    bool sk = false;
    const int rc = bayes(ctx, ctx->main, d_colors, d_pixcov, d_mask, d_nsim, d_state, W, H, w, b, min_eig, d_sum, d_count, false, row_begin, row_end,
                         reinterpret_cast<const long long *>(d_skip_if), reinterpret_cast<const long long *>(h_skip_if), d_skip_if ? &sk : nullptr);
    if (skipped) *skipped = sk ? 1 : 0;
    return rc;
}

int bcd_hip_finalize(bcd_hip_ctx *ctx, const float *d_sum, const int32_t *d_count, int64_t npix, float *d_out)
{
    if (!ctx || !d_sum || !d_count || !d_out || npix <= 0) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_finalize(d_sum, d_count, npix, d_out, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_finalize_band(bcd_hip_ctx *ctx, const float *d_sum, const int32_t *d_count, int W, int rows, int halo, const float *d_up_sum,
                          const int32_t *d_up_count, const float *d_down_sum, const int32_t *d_down_count, float *d_out)
{
    if (!ctx || !d_sum || !d_count || !d_out || W <= 0 || rows <= 0 || halo < 0) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    if ((d_up_sum == nullptr) != (d_up_count == nullptr) || (d_down_sum == nullptr) != (d_down_count == nullptr)) return bad(ctx, "halo sum without count");
    if ((d_up_sum || d_down_sum) && halo > rows) return bad(ctx, "halo larger than the band");
    HIPCHK(ctx, bcd_launch_finalize_band(d_sum, d_count, W, rows, halo, d_up_sum, d_up_count, d_down_sum, d_down_count, d_out, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_downscale_sum(bcd_hip_ctx *ctx, const float *d_in, int W, int H, int D, float *d_out)
{
    if (!ctx || !d_in || !d_out || W < 2 || H < 2 || D <= 0) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_downscale(0, d_in, W, H, D, d_out, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_downscale_avg(bcd_hip_ctx *ctx, const float *d_in, int W, int H, int D, float *d_out)
{
    if (!ctx || !d_in || !d_out || W < 2 || H < 2 || D <= 0) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_downscale(1, d_in, W, H, D, d_out, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_downscale_cov(bcd_hip_ctx *ctx, const float *d_cov, const float *d_ns, int W, int H, float *d_out)
{
    if (!ctx || !d_cov || !d_ns || !d_out || W < 2 || H < 2) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_downscale_cov(d_cov, d_ns, W, H, d_out, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_interpolate(bcd_hip_ctx *ctx, const float *d_lo, int w, int h, int D, float *d_hi, int W, int H)
{
    if (!ctx || !d_lo || !d_hi || w != W / 2 || h != H / 2 || w <= 0 || h <= 0 || D <= 0) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_interpolate(0, d_lo, w, h, D, d_hi, W, H, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_merge(bcd_hip_ctx *ctx, float *d_hi, int W, int H, const float *d_lo, int D)
{
    if (!ctx || !d_hi || !d_lo || W < 2 || H < 2 || D <= 0) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    return merge_on(ctx, ctx->main, d_hi, W, H, d_lo, D);
}

int bcd_hip_spike_filter(bcd_hip_ctx *ctx, const float *d_col, const float *d_ns, const float *d_hist, const float *d_cov, int W, int H,
                         int D, float factor, float *o_col, float *o_ns, float *o_hist, float *o_cov)
{
    if (!ctx || !d_col || !d_ns || !d_hist || !d_cov || !o_col || !o_ns || !o_hist || !o_cov) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    if (W < 3 || H < 3 || D <= 0) return bad(ctx, "image smaller than 3x3");
    HIPCHK(ctx, bcd_launch_spike(d_col, d_ns, d_hist, d_cov, W, H, D, factor, o_col, o_ns, o_hist, o_cov, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_accumulate_samples(bcd_hip_ctx *ctx, const float *d_samples, const float *d_weights, int W, int H, int spp, int nb_bins,
                               float gamma, float max_value, float *d_nsamples, float *d_mean, float *d_cov, float *d_hist)
{
    if (!ctx || !d_samples || !d_nsamples || !d_mean || !d_cov || !d_hist) return bad(ctx, "null pointer");
    DEVICE_GUARD(ctx);
    // (2 bins: nb_bins - 2 = 0 puts every value in the saturation branch, bins 0 and 1 -- in bounds; the minimum of bcd_hip_accum_create)
    if (W <= 0 || H <= 0 || spp <= 0 || nb_bins < 2) return bad(ctx, "bad size");
    if ((size_t)3 * nb_bins * 64 * sizeof(float) > 160 * 1024) { set_err(ctx, "more than 213 bins per channel are not supported"); return BCD_HIP_EUNSUPPORTED; }
    HIPCHK(ctx, bcd_launch_accumulate_samples(d_samples, d_weights, (int64_t)W * H, spp, nb_bins, gamma, max_value, d_nsamples, d_mean, d_cov, d_hist, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_zero_bad_values(bcd_hip_ctx *ctx, float *d_img, int64_t n)
{
    if (!ctx || !d_img || n <= 0) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_zero_bad(d_img, n, ctx->stream));
    return BCD_HIP_OK;
}

// ---- host utilities -------------------------------------------------------------------------------------
uint32_t bcd_hip_scale_seed(uint32_t seed0, int scale) { return seed0 + (uint32_t)scale; }

uint32_t bcd_hip_strip_order_seed(int W, int H, int patch_radius, int search_radius) { return bcd_strip_order_seed(W, H, patch_radius, search_radius); }

int bcd_hip_visit_order(int W, int H, int w, int random_order, uint32_t seed, int32_t *h_order)
{
    if (!h_order || W < 2 * w + 1 || H < 2 * w + 1 || w < 0) return BCD_HIP_EINVAL;
    std::vector<uint64_t> keys;
    keys.reserve((size_t)(W - 2 * w) * (H - 2 * w));
    for (int l = w; l <= H - 1 - w; ++l)
        for (int c = w; c <= W - 1 - w; ++c) keys.push_back(bcd_order_key((uint32_t)(l * W + c), random_order, seed));
    std::sort(keys.begin(), keys.end());
    for (size_t i = 0; i < keys.size(); ++i) h_order[i] = (int32_t)(keys[i] & 0xffffffffu);
    return BCD_HIP_OK;
}

} // extern "C"
