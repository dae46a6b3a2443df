// bcd_host.hip -- the host-buffer entry points of the C ABI (bcd_hip_denoise_host*, bcd_hip_denoise_layers_host): the frame is uploaded -- streamed in
// row chunks, the histograms without their zeros -- denoised by the drivers of bcd_api.hip and copied back.
#include "bcd_ctx.h"

#include <algorithm>
#include <thread>

// the upload stream and the sparse uploader of the host-buffer entry points, created on first use
int host_upload_stream(bcd_hip_ctx *ctx)
{
    if (!ctx->upload_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->upload_stream, hipStreamNonBlocking));
    return BCD_HIP_OK;
}

int host_sparse_uploader(bcd_hip_ctx *ctx)
{
    if (!ctx->sparse && !(ctx->sparse = bcd_sparse_create())) { set_err(ctx, "out of host memory"); return BCD_HIP_ENOMEM; }
    return BCD_HIP_OK;
}

// The streamed upload of a frame (bcd_hip_denoise_host_ex on frames of >= 256 lines, and bcd_hip_selftest_host_stream): the four host images h_src
// (colours, sample counts, histograms, covariances) go to the device copies d[0..3]; d[5..8] are the prefiltered copies (== d[0..3] without the prefilter).
// Returns with everything enqueued: the main stream waits for what the upload streams carry.  stop_after_chunks >= 0: only that many row chunks are
// uploaded and scheduled; poison: see below (both for the self-test; the host path passes -1 and false).
int host_stream_frame(bcd_hip_ctx *ctx, const float *const h_src[4], float *const d[9], int W, int H, int D, int b, float tau, bool prefilter, float spike_factor,
                      int stop_after_chunks, bool poison, HostStreamProgress *out, bool margin)
{
    Work &wk = ctx->main;
    RCCHK(host_upload_stream(ctx));
    const size_t np = (size_t)W * H;
    const size_t sz[4] = { np * 3, np, np * D, np * 6 };
    const int nd = bcd_delta_count(b), tile = bcd_pairdist_rw_tile_lines();
    // (the sizes similarity() will ask for: a larger request there would REALLOCATE the planes computed here)
    RCCHK(ensure(ctx, wk.T, half_plane_bytes(np, nd)));
    RCCHK(ensure(ctx, wk.Cn, count_plane_bytes(np, nd)));
    RCCHK(ensure(ctx, wk.counters, sizeof(Counters)));
    Counters::Flags *d_flag = &wk.d_counters()->flags;
    HIPCHK(ctx, hipMemsetAsync(d_flag, 0, sizeof(*d_flag), ctx->stream));
    // uniform power-of-two sample count: taken from the first pixel; the distance kernel checks every pixel against it and raises the
    // flag that sends the scale to the exact kernels if the guess was wrong (k_pairdist_rw, range_flag bit 1)
    // (a strided sample of 1024 pixels settles the usual non-uniform case -- adaptive sampling -- on the host at no cost)
    float uni_n = 0.f;
    {
        const float *h_ns = h_src[1];
        const float n0 = h_ns[0];
        if (is_pow2_sample_count(n0)) uni_n = n0;
        const size_t stride = std::max<size_t>(1, np / 1024);
        for (size_t i = 0; i < np && uni_n > 0.f; i += stride)
            if (h_ns[i] != n0) uni_n = 0.f;
    }
    // general sample counts: the RATIO form of the kernel, as similarity() chooses it for a resident frame, unless this workspace has seen it decline
    // on frames of this size.  Its statistics are cleared here and judged behind the last tile row (the verdict needs the whole frame).
    const bool ratio = uni_n == 0.f && !wk.ratio_is_declined(W, H);
    if (ratio) {
        RCCHK(ensure(ctx, wk.ratio_stats, 128 * sizeof(unsigned int)));
        HIPCHK(ctx, bcd_launch_ratio_begin((unsigned int *)wk.ratio_stats.p, ctx->stream));
    }
    margin = margin && !ratio; // (the RATIO form keeps T / C planes)
    const float margin_tau = margin ? tau : 0.f; // the margin plane is a function of the threshold: known here, before the first launch
    const int chunk = std::max(64, ((H + 7) / 8 + tile - 1) / tile * tile); // ~8 chunks, whole tile rows
    const int tile_rows = (H + tile - 1) / tile;
    int filtered = 0, tiles_done = 0, k = 0;
    if (poison) { // (self-test) whatever this function reads or writes holds 0xFF bytes before the first transfer: a line that is read before it has arrived shows
        for (int i = 0; i < 4; ++i) {
            HIPCHK(ctx, hipMemsetAsync(d[i], 0xFF, sz[i] * sizeof(float), ctx->stream));
            if (d[5 + i] != d[i]) HIPCHK(ctx, hipMemsetAsync(d[5 + i], 0xFF, sz[i] * sizeof(float), ctx->stream));
        }
        HIPCHK(ctx, hipMemsetAsync(wk.T.p, 0xFF, half_plane_bytes(np, nd), ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(wk.Cn.p, 0xFF, count_plane_bytes(np, nd), ctx->stream));
    }
    // the upload stream must not overwrite device copies an earlier frame's kernels may still read
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // colours, sample counts and covariances first, whole (83 MB at 1080p; the prefilter and the distance kernel need them with the
    // first histogram lines), then the histograms -- 87 % of the bytes -- in row chunks
    // Without the prefilter only the sample counts are needed with the first histogram lines (the distance kernel); colours and covariances
    // are first read by the pyramid and the estimate stage.  Their (pageable, host-blocking) copies then run on a helper thread and a
    // stream of their own beside the histogram pieces, whose pace is set by the host-side packing and leaves the link half idle (round 4).
    std::thread side_copy;
    hipError_t side_rc = hipSuccess;
    struct SideJoin { std::thread &t; ~SideJoin() { if (t.joinable()) t.join(); } } side_join{ side_copy };
    const bool side = !prefilter && ctx->sparse_uploads && (D & 3) == 0;
    if (side) {
        if (!ctx->upload_stream2) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->upload_stream2, hipStreamNonBlocking));
        if (!ctx->ev_upload2) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_upload2, hipEventDisableTiming));
        HIPCHK(ctx, hipMemcpyAsync(d[1], h_src[1], sz[1] * sizeof(float), hipMemcpyHostToDevice, ctx->upload_stream));
        const int dev = ctx->device;
        hipStream_t s2 = ctx->upload_stream2;
        hipEvent_t e2 = ctx->ev_upload2;
        float *dc = d[0], *dv = d[3];
        const float *hc = h_src[0], *hv = h_src[3];
        const size_t nc = sz[0] * sizeof(float), nv = sz[3] * sizeof(float);
        side_copy = std::thread([=, &side_rc]() {
            hipError_t e = hipSetDevice(dev);
            if (e == hipSuccess) e = hipMemcpyAsync(dc, hc, nc, hipMemcpyHostToDevice, s2);
            if (e == hipSuccess) e = hipMemcpyAsync(dv, hv, nv, hipMemcpyHostToDevice, s2);
            if (e == hipSuccess) e = hipEventRecord(e2, s2);
            side_rc = e;
        });
    } else
        for (int i : { 0, 1, 3 }) HIPCHK(ctx, hipMemcpyAsync(d[i], h_src[i], sz[i] * sizeof(float), hipMemcpyHostToDevice, ctx->upload_stream));
    const bool sparse = ctx->sparse_uploads && (D & 3) == 0;
    if (sparse) {
        RCCHK(host_sparse_uploader(ctx));
        bcd_sparse_frame_begin(ctx->sparse);
    }
    ctx->upload_raw_bytes = ctx->upload_sent_bytes = (long long)sz[2] * 4;
    for (int r0 = 0; r0 < H && (stop_after_chunks < 0 || k < stop_after_chunks); r0 += chunk, ++k) {
        const int r1 = std::min(H, r0 + chunk);
        {
            const size_t off = (size_t)r0 * W * D, n = (size_t)(r1 - r0) * W * D;
            if (sparse) HIPCHK(ctx, bcd_sparse_upload(ctx->sparse, d[2] + off, h_src[2] + off, n, ctx->upload_stream)); // (off % 4 == 0: D % 4 == 0 on this path)
            else HIPCHK(ctx, hipMemcpyAsync(d[2] + off, h_src[2] + off, n * sizeof(float), hipMemcpyHostToDevice, ctx->upload_stream));
        }
        if ((int)ctx->ev_upload.size() <= k) {
            hipEvent_t ev;
            HIPCHK(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            ctx->ev_upload.push_back(ev);
        }
        HIPCHK(ctx, hipEventRecord(ctx->ev_upload[k], ctx->upload_stream));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_upload[k], 0));
        int avail = r1;
        if (prefilter) { // a filtered line reads its own and the two adjacent input lines (clamped inward at the frame border)
            const int upto = r1 == H ? H : std::max(0, r1 - 1);
            HIPCHK(ctx, bcd_launch_spike_rows(d[0], d[1], d[2], d[3], W, H, D, spike_factor, d[5], d[6], d[7], d[8], filtered, upto, ctx->stream));
            filtered = std::max(filtered, upto);
            avail = filtered;
        }
        // a tile row reads its own lines and the b lines below them
        const int t_end = avail == H ? tile_rows : std::max(0, (avail - b) / tile);
        if (t_end > tiles_done) {
            if (ratio) HIPCHK(ctx, bcd_launch_pairdist_rw_ratio_rows(d[7], d[6], W, H, D, b, wk.T.p, (uint8_t *)wk.Cn.p, &d_flag->range, (unsigned int *)wk.ratio_stats.p, tiles_done, t_end, ctx->stream));
            else HIPCHK(ctx, bcd_launch_pairdist_rw_rows(d[7], d[6], W, H, D, b, wk.T.p, (uint8_t *)wk.Cn.p, &d_flag->range, uni_n, tiles_done, t_end, ctx->stream, margin_tau));
            tiles_done = t_end;
            if (ratio && tiles_done == tile_rows) HIPCHK(ctx, bcd_launch_ratio_verdict((const unsigned int *)wk.ratio_stats.p, tau, &d_flag->range, ctx->stream));
        }
    }
    if (sparse) bcd_sparse_frame_bytes(ctx->sparse, &ctx->upload_raw_bytes, &ctx->upload_sent_bytes);
    if (side) { // colours and covariances have been enqueued by now (the helper thread is joined), the frame's kernels wait for their arrival
        side_copy.join();
        HIPCHK(ctx, side_rc);
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_upload2, 0));
    }
    out->chunk_lines = chunk; out->chunks = k; out->rows_filtered = filtered; out->tile_rows_done = tiles_done; out->uni_n = uni_n; out->ratio = ratio; out->margin = margin;
    return BCD_HIP_OK;
}

// bcd_hip_denoise_host_ex, and -- with `extra`: host images of further colour layers -- bcd_hip_denoise_layers_host: the primary inputs travel as they always
// did (streamed, the histograms without their zeros), the extra layers as plain copies behind them.  filter_layers (bcd_hip_denoise_layers_host_ex): the
// prefilter covers the extra layers too -- gathered on the device through the source map of the primary colours
static int denoise_host_impl(bcd_hip_ctx *ctx, const float *h_colors, const float *h_ns, const float *h_hist, const float *h_cov,
                             int W, int H, int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_host_options *opt, float *h_out,
                             const bcd_hip_host_layer *extra, int nb_extra, bool filter_layers = false)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!h_colors || !h_ns || !h_hist || !h_cov || !h_out) return bad(ctx, "null image pointer");
    RCCHK(check_params(ctx, W, H, D, prm));
    DEVICE_GUARD(ctx);
    const size_t np = (size_t)W * H;
    const size_t sz[5] = { np * 3, np, np * D, np * 6, np * 3 };
    const float *src[4] = { h_colors, h_ns, h_hist, h_cov };
    const bool prefilter = opt && opt->spike_factor > 0.f;
    if (prefilter && (W < 3 || H < 3)) return bad(ctx, "image smaller than 3x3");
    // device copies live in the context (grow-only): a sequence of frames pays for the allocations once
    float *d[9];
    for (int i = 0; i < 5; ++i) { RCCHK(ensure(ctx, ctx->host_stage[i], sz[i] * sizeof(float))); d[i] = (float *)ctx->host_stage[i].p; }
    for (int i = 0; i < 4; ++i) {
        d[5 + i] = d[i];
        if (prefilter) { RCCHK(ensure(ctx, ctx->host_stage[5 + i], sz[i] * sizeof(float))); d[5 + i] = (float *)ctx->host_stage[5 + i].p; }
    }
    // The frame arrives in row chunks on an upload stream; the lines that have arrived are prefiltered (SpikeRemovalFilter::filter,
    // src/cli/main.cpp:428-441, on the device copies: no second trip over PCIe) and the finest scale's approximate distance planes -- the
    // largest single kernel of the frame, and a function of the histograms alone -- are computed for them while the next chunk travels.
    // Everything else needs the whole frame (pyramid, the marking order) and follows the last chunk.
    const int b = prm->search_radius;
    const bool stream_in = host_frame_streams(ctx, H, D, prm);
    if (!stream_in) {
        for (int i = 0; i < 4; ++i) HIPCHK(ctx, hipMemcpyAsync(d[i], src[i], sz[i] * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        if (prefilter) HIPCHK(ctx, bcd_launch_spike(d[0], d[1], d[2], d[3], W, H, D, opt->spike_factor, d[5], d[6], d[7], d[8], ctx->stream));
    } else {
        HostStreamProgress done;
        RCCHK(host_stream_frame(ctx, src, d, W, H, D, b, prm->hist_dist_threshold, prefilter, prefilter ? opt->spike_factor : 0.f, -1, false, &done, ctx->margin_planes));
        Work &wk = ctx->main;
        wk.planes.ready = true; wk.planes.hist = d[7]; wk.planes.ns = d[6]; wk.planes.W = W; wk.planes.H = H; wk.planes.D = D; wk.planes.b = b;
        wk.planes.tau = prm->hist_dist_threshold; wk.planes.uni_n = done.uni_n; wk.planes.ratio = done.ratio; wk.planes.margin = done.margin;
    }
    LayerView lv;
    if (nb_extra > 0) { // device copies of the extra layers: colours | covariances | outputs, one slice per layer
        auto fail = [&](int rc) { ctx->main.planes.ready = false; return rc; };
        for (int i = 0; i < 3; ++i)
            if (ensure(ctx, ctx->lay_host[i], (size_t)nb_extra * np * (i == 1 ? 6 : 3) * sizeof(float)) != BCD_HIP_OK) return fail(BCD_HIP_ENOMEM);
        lv.n = nb_extra;
        for (int k = 0; k < nb_extra; ++k) {
            float *dc = (float *)ctx->lay_host[0].p + k * np * 3, *dv = (float *)ctx->lay_host[1].p + k * np * 6;
            lv.col[k] = dc; lv.cov[k] = dv; lv.out[k] = (float *)ctx->lay_host[2].p + k * np * 3;
            if (hipMemcpyAsync(dc, extra[k].h_colors, np * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
                hipMemcpyAsync(dv, extra[k].h_covariances, np * 6 * sizeof(float), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
                set_err(ctx, "upload of a colour layer failed");
                return fail(BCD_HIP_EDEVICE);
            }
        }
        if (prefilter && filter_layers) {
            // The primary layer has been filtered above, line by line as it arrived.  The decision behind it is a function of the UNFILTERED primary colours,
            // which are still resident (d[0]): it is taken once more as a source map (k_spike_map: 108 B read and 4 B written per pixel) and every extra
            // layer's colours and covariances are gathered through it into a second set of slices, which the frame then reads.  No second trip over
            // PCIe, and nothing in the upload schedule of the primary layer moves.
            if (ensure(ctx, ctx->spike_map, np * sizeof(int32_t)) != BCD_HIP_OK) return fail(BCD_HIP_ENOMEM);
            for (int i = 0; i < 2; ++i)
                if (ensure(ctx, ctx->lay_host_f[i], (size_t)nb_extra * np * (i == 1 ? 6 : 3) * sizeof(float)) != BCD_HIP_OK) return fail(BCD_HIP_ENOMEM);
            int32_t *d_map = (int32_t *)ctx->spike_map.p;
            BcdSpikeTable tc = {}, tv = {};
            for (int k = 0; k < nb_extra; ++k) {
                tc.src[k] = lv.col[k]; tc.dst[k] = (float *)ctx->lay_host_f[0].p + k * np * 3;
                tv.src[k] = lv.cov[k]; tv.dst[k] = (float *)ctx->lay_host_f[1].p + k * np * 6;
                lv.col[k] = tc.dst[k]; lv.cov[k] = tv.dst[k];
            }
            if (bcd_launch_spike_map(d[0], W, H, opt->spike_factor, d_map, nullptr, ctx->stream) != hipSuccess ||
                bcd_launch_spike_apply(tc, nb_extra, d_map, W, H, 3, ctx->stream) != hipSuccess ||
                bcd_launch_spike_apply(tv, nb_extra, d_map, W, H, 6, ctx->stream) != hipSuccess) {
                set_err(ctx, "the spike prefilter of the colour layers failed to launch");
                return fail(BCD_HIP_EDEVICE);
            }
        }
    }
    {
        const int rc = denoise_impl(ctx, d[5], d[6], d[7], d[8], W, H, D, nb_scales, prm, d[4], nb_extra > 0 ? &lv : nullptr);
        ctx->main.planes.ready = false; // (consumed by the finest scale's similarity stage; never left behind by a call that failed earlier)
        if (rc != BCD_HIP_OK) return rc;
    }
    // checkAndPutToZeroNegativeInfNaNValues (src/cli/main.cpp:389-420, 470)
    if (opt && opt->zero_bad_values) HIPCHK(ctx, bcd_launch_zero_bad(d[4], (int64_t)np * 3, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(h_out, d[4], sz[4] * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (nb_extra > 0) {
        if (opt && opt->zero_bad_values) HIPCHK(ctx, bcd_launch_zero_bad(lv.out[0], (int64_t)nb_extra * np * 3, ctx->stream)); // (the outputs lie one behind the other)
        for (int k = 0; k < nb_extra; ++k) HIPCHK(ctx, hipMemcpyAsync(extra[k].h_out, lv.out[k], np * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BCD_HIP_OK;
}

extern "C" {

int bcd_hip_denoise_host_ex(bcd_hip_ctx *ctx, const float *h_colors, const float *h_ns, const float *h_hist, const float *h_cov,
                            int W, int H, int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_host_options *opt, float *h_out)
{
    return denoise_host_impl(ctx, h_colors, h_ns, h_hist, h_cov, W, H, D, nb_scales, prm, opt, h_out, nullptr, 0);
}

int bcd_hip_denoise_layers_host(bcd_hip_ctx *ctx, const float *h_ns, const float *h_hist, int W, int H, int D, int nb_scales, const bcd_hip_params *prm,
                                const bcd_hip_host_options *opt, const bcd_hip_host_layer *layers, int nb_layers)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!h_ns || !h_hist) return bad(ctx, "null image pointer");
    if (!layers) return bad(ctx, "null layer list");
    if (nb_layers < 1 || nb_layers > BCD_HIP_MAX_LAYERS) return bad(ctx, "the number of layers must be between 1 and 16 (BCD_HIP_MAX_LAYERS)");
    for (int k = 0; k < nb_layers; ++k) {
        if (!layers[k].h_colors || !layers[k].h_covariances || !layers[k].h_out) return bad(ctx, "null image pointer in a layer");
        for (int j = 0; j < k; ++j) if (layers[j].h_out == layers[k].h_out) return bad(ctx, "two layers share an output image");
    }
    if (nb_layers > 1 && opt && opt->spike_factor > 0.f) {
        set_err(ctx, "the spike prefilter moves whole pixels by the first layer's colours: it is not available with several layers");
        return BCD_HIP_EUNSUPPORTED;
    }
    return denoise_host_impl(ctx, layers[0].h_colors, h_ns, h_hist, layers[0].h_covariances, W, H, D, nb_scales, prm, opt, layers[0].h_out, layers + 1, nb_layers - 1);
}

int bcd_hip_denoise_layers_host_ex(bcd_hip_ctx *ctx, const float *h_ns, const float *h_hist, int W, int H, int D, int nb_scales, const bcd_hip_params *prm,
                                   const bcd_hip_layers_host_options *opt, const bcd_hip_host_layer *layers, int nb_layers)
{
    if (!ctx) return BCD_HIP_EINVAL;
    bcd_hip_host_options o = { 0.f, 0 };
    if (opt) { o.spike_factor = opt->spike_factor; o.zero_bad_values = opt->zero_bad_values; }
    if (!opt || !opt->filter_layers || nb_layers < 2 || !(o.spike_factor > 0.f)) // nothing for the switch to do: the old call, with its refusal
        return bcd_hip_denoise_layers_host(ctx, h_ns, h_hist, W, H, D, nb_scales, prm, &o, layers, nb_layers);
    if (!h_ns || !h_hist) return bad(ctx, "null image pointer");
    if (!layers) return bad(ctx, "null layer list");
    if (nb_layers > BCD_HIP_MAX_LAYERS) return bad(ctx, "the number of layers must be between 1 and 16 (BCD_HIP_MAX_LAYERS)");
    for (int k = 0; k < nb_layers; ++k) {
        if (!layers[k].h_colors || !layers[k].h_covariances || !layers[k].h_out) return bad(ctx, "null image pointer in a layer");
        for (int j = 0; j < k; ++j) if (layers[j].h_out == layers[k].h_out) return bad(ctx, "two layers share an output image");
    }
    return denoise_host_impl(ctx, layers[0].h_colors, h_ns, h_hist, layers[0].h_covariances, W, H, D, nb_scales, prm, &o, layers[0].h_out, layers + 1, nb_layers - 1, true);
}

// bcd_hip_denoise_moments for host images: plain uploads into the context's grow-only device copies, the resident call, downloads.  Nothing is streamed in:
// 24 + 36 L bytes per pixel travel instead of the histogram image.
int bcd_hip_denoise_moments_host(bcd_hip_ctx *ctx, const float *h_ns, int W, int H, int nb_scales, const bcd_hip_params *prm, const bcd_hip_layers_host_options *opt,
                                 float var_floor, const bcd_hip_host_layer *layers, int nb_layers)
{
    if (!ctx) return BCD_HIP_EINVAL;
    // ---- everything is checked before any device work
    if (!h_ns) return bad(ctx, "null image pointer");
    if (!layers) return bad(ctx, "null layer list");
    if (nb_layers < 1 || nb_layers > BCD_HIP_MAX_LAYERS) return bad(ctx, "the number of layers must be between 1 and 16 (BCD_HIP_MAX_LAYERS)");
    for (int k = 0; k < nb_layers; ++k) {
        if (!layers[k].h_colors || !layers[k].h_covariances || !layers[k].h_out) return bad(ctx, "null image pointer in a layer");
        for (int j = 0; j < k; ++j) if (layers[j].h_out == layers[k].h_out) return bad(ctx, "two layers share an output image");
    }
    if (!(var_floor >= 0.f) || !std::isfinite(var_floor)) return bad(ctx, "the variance floor must be finite and not negative");
    const bool prefilter = opt && opt->spike_factor > 0.f;
    if (prefilter && nb_layers > 1 && !opt->filter_layers) {
        set_err(ctx, "the spike prefilter moves whole pixels by the first layer's colours: it is not available with several layers");
        return BCD_HIP_EUNSUPPORTED;
    }
    RCCHK(check_params(ctx, W, H, 1, prm));
    if (nb_scales < 1 || nb_scales > MAX_SCALES) return bad(ctx, "bad number of scales");
    for (int s = 1, ws = W, hs = H; s < nb_scales; ++s) {
        ws /= 2; hs /= 2;
        if (ws < 2 * prm->patch_radius + 1 || hs < 2 * prm->patch_radius + 1) return bad(ctx, "too many scales for this image size");
    }
    if (prefilter && (W < 3 || H < 3)) return bad(ctx, "image smaller than 3x3");
    DEVICE_GUARD(ctx);
    const size_t np = (size_t)W * H, f = sizeof(float);
    const int L = nb_layers;
    RCCHK(ensure(ctx, ctx->host_stage[1], np * f));
    for (int i = 0; i < 3; ++i) RCCHK(ensure(ctx, ctx->lay_host[i], (size_t)L * np * (i == 1 ? 6 : 3) * f));
    const float *d_ns = (const float *)ctx->host_stage[1].p;
    bcd_hip_layer dl[BCD_HIP_MAX_LAYERS];
    HIPCHK(ctx, hipMemcpyAsync(ctx->host_stage[1].p, h_ns, np * f, hipMemcpyHostToDevice, ctx->stream));
    for (int k = 0; k < L; ++k) {
        float *dc = (float *)ctx->lay_host[0].p + k * np * 3, *dv = (float *)ctx->lay_host[1].p + k * np * 6;
        HIPCHK(ctx, hipMemcpyAsync(dc, layers[k].h_colors, np * 3 * f, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(dv, layers[k].h_covariances, np * 6 * f, hipMemcpyHostToDevice, ctx->stream));
        dl[k].d_colors = dc; dl[k].d_covariances = dv; dl[k].d_out = (float *)ctx->lay_host[2].p + k * np * 3;
    }
    if (prefilter) { // the source map of the first layer's colours moves the sample counts and every layer on the resident copies: no histogram to move
        RCCHK(ensure(ctx, ctx->host_stage[6], np * f));
        for (int i = 0; i < 2; ++i) RCCHK(ensure(ctx, ctx->lay_host_f[i], (size_t)L * np * (i == 1 ? 6 : 3) * f));
        bcd_hip_spike_layer sl[BCD_HIP_MAX_LAYERS];
        for (int k = 0; k < L; ++k) {
            sl[k].d_colors = dl[k].d_colors; sl[k].d_covariances = dl[k].d_covariances;
            sl[k].d_colors_out = (float *)ctx->lay_host_f[0].p + k * np * 3; sl[k].d_covariances_out = (float *)ctx->lay_host_f[1].p + k * np * 6;
            dl[k].d_colors = sl[k].d_colors_out; dl[k].d_covariances = sl[k].d_covariances_out;
        }
        RCCHK(bcd_hip_spike_filter_layers(ctx, d_ns, nullptr, W, H, 0, opt->spike_factor, (float *)ctx->host_stage[6].p, nullptr, sl, L, nullptr, nullptr));
        d_ns = (const float *)ctx->host_stage[6].p;
    }
    RCCHK(bcd_hip_denoise_moments(ctx, d_ns, W, H, nb_scales, prm, var_floor, dl, L, nullptr));
    if (opt && opt->zero_bad_values) HIPCHK(ctx, bcd_launch_zero_bad(dl[0].d_out, (int64_t)L * np * 3, ctx->stream)); // (the outputs lie one behind the other)
    for (int k = 0; k < L; ++k) HIPCHK(ctx, hipMemcpyAsync(layers[k].h_out, dl[k].d_out, np * 3 * f, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BCD_HIP_OK;
}

// bcd_hip_denoise_guided for host images: plain uploads of the features and their variances into the context's grow-only device copies and their pyramid on
// the context's stream, then -- with ctx->guide set -- the host call of the layers (histograms: streamed in as ever, the planes computed ahead are consumed
// by the selection pass before the gate takes the workspace's planes) or of the moment selection.  Every refusal of those calls is made here first, so that
// none follows device work.
int bcd_hip_denoise_guided_host(bcd_hip_ctx *ctx, const float *h_ns, const float *h_hist, int W, int H, int D, int nb_scales, const bcd_hip_params *prm,
                                const bcd_hip_layers_host_options *opt, float var_floor, const bcd_hip_host_layer *layers, int nb_layers, const bcd_hip_guide *guide)
{
    if (!ctx) return BCD_HIP_EINVAL;
    const bool moments = h_hist == nullptr;
    if (!h_ns) return bad(ctx, "null image pointer");
    if (!layers) return bad(ctx, "null layer list");
    if (nb_layers < 1 || nb_layers > BCD_HIP_MAX_LAYERS) return bad(ctx, "the number of layers must be between 1 and 16 (BCD_HIP_MAX_LAYERS)");
    for (int k = 0; k < nb_layers; ++k) {
        if (!layers[k].h_colors || !layers[k].h_covariances || !layers[k].h_out) return bad(ctx, "null image pointer in a layer");
        for (int j = 0; j < k; ++j) if (layers[j].h_out == layers[k].h_out) return bad(ctx, "two layers share an output image");
    }
    if (moments && (!(var_floor >= 0.f) || !std::isfinite(var_floor))) return bad(ctx, "the variance floor must be finite and not negative");
    const bool prefilter = opt && opt->spike_factor > 0.f;
    if (prefilter && nb_layers > 1 && !opt->filter_layers) {
        set_err(ctx, "the spike prefilter moves whole pixels by the first layer's colours: it is not available with several layers");
        return BCD_HIP_EUNSUPPORTED;
    }
    RCCHK(check_params(ctx, W, H, moments ? 1 : D, prm));
    if (nb_scales < 1 || nb_scales > MAX_SCALES) return bad(ctx, "bad number of scales");
    for (int s = 1, ws = W, hs = H; s < nb_scales; ++s) {
        ws /= 2; hs /= 2;
        if (ws < 2 * prm->patch_radius + 1 || hs < 2 * prm->patch_radius + 1) return bad(ctx, "too many scales for this image size");
    }
    if (prefilter && (W < 3 || H < 3)) return bad(ctx, "image smaller than 3x3");
    if ((int64_t)W * H >= (1ll << 31) / BCD_HIP_GUIDE_MAX_CHANNELS) return bad(ctx, "image too large for 32-bit DeepImage indices");
    RCCHK(check_guide(ctx, guide, prm->search_radius));
    {
        DEVICE_GUARD(ctx);
        const size_t bytes = (size_t)W * H * guide->nb_channels * sizeof(float);
        RCCHK(ensure(ctx, ctx->guide_host[0], bytes));
        HIPCHK(ctx, hipMemcpyAsync(ctx->guide_host[0].p, guide->features, bytes, hipMemcpyHostToDevice, ctx->stream));
        if (guide->variances) {
            RCCHK(ensure(ctx, ctx->guide_host[1], bytes));
            HIPCHK(ctx, hipMemcpyAsync(ctx->guide_host[1].p, guide->variances, bytes, hipMemcpyHostToDevice, ctx->stream));
        }
        RCCHK(guide_begin(ctx, guide, (const float *)ctx->guide_host[0].p, guide->variances ? (const float *)ctx->guide_host[1].p : nullptr, W, H, nb_scales));
    }
    const int rc = moments ? bcd_hip_denoise_moments_host(ctx, h_ns, W, H, nb_scales, prm, opt, var_floor, layers, nb_layers)
                           : bcd_hip_denoise_layers_host_ex(ctx, h_ns, h_hist, W, H, D, nb_scales, prm, opt, layers, nb_layers);
    guide_end(ctx);
    return rc;
}

int bcd_hip_last_upload_bytes(const bcd_hip_ctx *ctx, int64_t *hist_bytes, int64_t *hist_bytes_sent)
{
    if (!ctx || !hist_bytes || !hist_bytes_sent) return BCD_HIP_EINVAL;
    *hist_bytes = ctx->upload_raw_bytes;
    *hist_bytes_sent = ctx->upload_sent_bytes;
    return BCD_HIP_OK;
}

int bcd_hip_denoise_host(bcd_hip_ctx *ctx, const float *h_colors, const float *h_ns, const float *h_hist, const float *h_cov,
                         int W, int H, int D, int nb_scales, const bcd_hip_params *prm, float *h_out)
{
    return bcd_hip_denoise_host_ex(ctx, h_colors, h_ns, h_hist, h_cov, W, H, D, nb_scales, prm, nullptr, h_out);
}

} // extern "C"
