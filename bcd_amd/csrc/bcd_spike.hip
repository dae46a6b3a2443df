// bcd_spike.hip -- the spike prefilter through a source map (bcd_hip_spike_map, bcd_hip_spike_apply, bcd_hip_spike_filter_layers): every argument is
// checked before any device work, everything is enqueued on the context's stream, no call synchronises -- but the in-place forms
// (bcd_hip_spike_apply_inplace, bcd_hip_spike_filter_layers_inplace; spike_gather_inplace below, which the animation paths call too), which read the
// number of moved pixels back once to size their list and staging buffer.
#include "bcd_ctx.h"

#include <vector>

namespace {

struct Range {
    const void *p;
    size_t bytes;
    Range(const void *p_, size_t n) : p(p_), bytes(n) {}
    bool overlaps(const Range &o) const { return bytes_overlap(p, bytes, o.p, o.bytes); }
};

// no output may be (or overlap) an input or another output
bool outputs_are_apart(const std::vector<Range> &in, const std::vector<Range> &out)
{
    for (size_t k = 0; k < out.size(); ++k) {
        for (const Range &r : in) if (out[k].overlaps(r)) return false;
        for (size_t j = 0; j < k; ++j) if (out[k].overlaps(out[j])) return false;
    }
    return true;
}

int check_frame(bcd_hip_ctx *ctx, int W, int H)
{
    if (W < 3 || H < 3) return bad(ctx, "image smaller than 3x3");
    if ((int64_t)W * H >= (1ll << 31)) return bad(ctx, "image too large: pixel indices must fit 31 bits");
    return BCD_HIP_OK;
}

// no two of them share a byte
bool all_apart(const std::vector<Range> &r)
{
    for (size_t k = 0; k < r.size(); ++k)
        for (size_t j = 0; j < k; ++j) if (r[k].overlaps(r[j])) return false;
    return true;
}

} // namespace

// The in-place gather of t's n images (t.img, t.depth) through d_map on the context's stream.  k_spike_moved_count counts the moved pixels (one atomic per
// workgroup of 4096 pixels -- the counter of bcd_launch_spike_map, one atomic per wavefront on one word, costs more than the map itself); the count is read
// back -- the one synchronisation -- and sizes the list and the staging buffer; with no moved pixel nothing further is launched.  No argument is checked here
int spike_gather_inplace(bcd_hip_ctx *ctx, const int32_t *d_map, size_t npix, BcdSpikeInplaceTable &t, int n, int32_t *h_moved)
{
    RCCHK(ensure(ctx, ctx->spike_count, 2 * sizeof(int32_t)));
    int32_t *d_cnt = (int32_t *)ctx->spike_count.p;
    HIPCHK(ctx, bcd_launch_spike_moved_count(d_map, (uint32_t)npix, d_cnt, ctx->stream));
    int32_t moved = 0;
    HIPCHK(ctx, hipMemcpyAsync(&moved, d_cnt, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (h_moved) *h_moved = moved;
    if (moved <= 0) return BCD_HIP_OK;
    const size_t floats = bcd_spike_stage_floats(t, n, (uint32_t)moved);
    RCCHK(ensure(ctx, ctx->spike_list, (size_t)moved * sizeof(int2)));
    RCCHK(ensure(ctx, ctx->spike_stage, floats * sizeof(float)));
    HIPCHK(ctx, bcd_launch_spike_compact(d_map, (uint32_t)npix, d_cnt + 1, (int2 *)ctx->spike_list.p, (uint32_t)moved, ctx->stream));
    HIPCHK(ctx, bcd_launch_spike_stage(t, n, (const int2 *)ctx->spike_list.p, (uint32_t)moved, (float *)ctx->spike_stage.p, ctx->stream));
    return BCD_HIP_OK;
}

// The spike prefilter of one resident frame in place: the map of d_col[0] into d_map (null: the context's scratch map), then one in-place gather of the
// sample counts, the histograms (null: none) and the colours and covariances of the L layers.  Synchronises once.  No argument is checked here
int spike_filter_frame_inplace(bcd_hip_ctx *ctx, float *d_ns, float *d_hist, int W, int H, int D, float factor, float *const *d_col, float *const *d_cov, int L,
                               int32_t *d_map, int32_t *h_moved)
{
    const size_t np = (size_t)W * H;
    if (!d_map) {
        RCCHK(ensure(ctx, ctx->spike_map, np * sizeof(int32_t)));
        d_map = (int32_t *)ctx->spike_map.p;
    }
    HIPCHK(ctx, bcd_launch_spike_map(d_col[0], W, H, factor, d_map, nullptr, ctx->stream));
    BcdSpikeInplaceTable t = {};
    int n = 0;
    t.img[n] = d_ns; t.depth[n++] = 1;
    if (d_hist) { t.img[n] = d_hist; t.depth[n++] = D; }
    for (int k = 0; k < L; ++k) { t.img[n] = d_col[k]; t.depth[n++] = 3; }
    for (int k = 0; k < L; ++k) { t.img[n] = d_cov[k]; t.depth[n++] = 6; }
    return spike_gather_inplace(ctx, d_map, np, t, n, h_moved);
}

extern "C" {

int bcd_hip_spike_map(bcd_hip_ctx *ctx, const float *d_colors, int W, int H, float factor, int32_t *d_map, int32_t *d_moved)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_colors || !d_map) return bad(ctx, "null image pointer");
    RCCHK(check_frame(ctx, W, H));
    const size_t np = (size_t)W * H;
    {
        std::vector<Range> in{ Range(d_colors, np * 3 * sizeof(float)) }, out{ Range(d_map, np * sizeof(int32_t)) };
        if (d_moved) out.push_back(Range(d_moved, sizeof(int32_t)));
        if (!outputs_are_apart(in, out)) return bad(ctx, "the map or the moved count overlaps the colours or each other");
    }
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_spike_map(d_colors, W, H, factor, d_map, d_moved, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_spike_apply(bcd_hip_ctx *ctx, const int32_t *d_map, int W, int H, int depth, const float *const *d_src, float *const *d_dst, int nb_images)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_map) return bad(ctx, "null map pointer");
    if (!d_src || !d_dst) return bad(ctx, "null image list");
    RCCHK(check_frame(ctx, W, H));
    if (depth < 1) return bad(ctx, "the depth must be at least 1");
    if (nb_images < 1 || nb_images > BCD_SPIKE_MAX_IMAGES) return bad(ctx, "the number of images must be between 1 and 32");
    const size_t np = (size_t)W * H, bytes = np * (size_t)depth * sizeof(float);
    BcdSpikeTable t = {};
    {
        std::vector<Range> in{ Range(d_map, np * sizeof(int32_t)) }, out;
        for (int k = 0; k < nb_images; ++k) {
            if (!d_src[k] || !d_dst[k]) return bad(ctx, "null image pointer in a list");
            t.src[k] = d_src[k]; t.dst[k] = d_dst[k];
            in.push_back(Range(d_src[k], bytes));
            out.push_back(Range(d_dst[k], bytes));
        }
        if (!outputs_are_apart(in, out)) return bad(ctx, "an output overlaps an input, the map or another output (the gather is out of place)");
    }
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_spike_apply(t, nb_images, d_map, W, H, depth, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_spike_filter_layers(bcd_hip_ctx *ctx, const float *d_nsamples, const float *d_histograms, int W, int H, int D, float factor, float *o_nsamples,
                                float *o_histograms, const bcd_hip_spike_layer *layers, int nb_layers, int32_t *d_map, int32_t *d_moved)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_nsamples || !o_nsamples) return bad(ctx, "null image pointer");
    if ((d_histograms == nullptr) != (o_histograms == nullptr)) return bad(ctx, "the histograms and their output must both be given or both be null");
    if (!layers) return bad(ctx, "null layer list");
    if (nb_layers < 1 || nb_layers > BCD_HIP_MAX_LAYERS) return bad(ctx, "the number of layers must be between 1 and 16 (BCD_HIP_MAX_LAYERS)");
    for (int k = 0; k < nb_layers; ++k)
        if (!layers[k].d_colors || !layers[k].d_covariances || !layers[k].d_colors_out || !layers[k].d_covariances_out) return bad(ctx, "null image pointer in a layer");
    RCCHK(check_frame(ctx, W, H));
    if (d_histograms && D < 1) return bad(ctx, "the depth must be at least 1");
    const size_t np = (size_t)W * H, f = sizeof(float);
    {
        std::vector<Range> in{ Range(d_nsamples, np * f) }, out{ Range(o_nsamples, np * f) };
        if (d_histograms) { in.push_back(Range(d_histograms, np * D * f)); out.push_back(Range(o_histograms, np * D * f)); }
        for (int k = 0; k < nb_layers; ++k) {
            in.push_back(Range(layers[k].d_colors, np * 3 * f));
            in.push_back(Range(layers[k].d_covariances, np * 6 * f));
            out.push_back(Range(layers[k].d_colors_out, np * 3 * f));
            out.push_back(Range(layers[k].d_covariances_out, np * 6 * f));
        }
        if (d_map) out.push_back(Range(d_map, np * sizeof(int32_t))); // (written by the first launch, read by the others: apart from every image)
        if (d_moved) out.push_back(Range(d_moved, sizeof(int32_t)));
        if (!outputs_are_apart(in, out)) return bad(ctx, "an output overlaps an input, the map or another output (the gather is out of place)");
    }
    DEVICE_GUARD(ctx);
    if (!d_map) {
        RCCHK(ensure(ctx, ctx->spike_map, np * sizeof(int32_t)));
        d_map = (int32_t *)ctx->spike_map.p;
    }
    HIPCHK(ctx, bcd_launch_spike_map(layers[0].d_colors, W, H, factor, d_map, d_moved, ctx->stream));
    BcdSpikeTable t = {};
    t.src[0] = d_nsamples; t.dst[0] = o_nsamples;
    HIPCHK(ctx, bcd_launch_spike_apply(t, 1, d_map, W, H, 1, ctx->stream));
    if (d_histograms) {
        t.src[0] = d_histograms; t.dst[0] = o_histograms;
        HIPCHK(ctx, bcd_launch_spike_apply(t, 1, d_map, W, H, D, ctx->stream));
    }
    for (int k = 0; k < nb_layers; ++k) { t.src[k] = layers[k].d_colors; t.dst[k] = layers[k].d_colors_out; }
    HIPCHK(ctx, bcd_launch_spike_apply(t, nb_layers, d_map, W, H, 3, ctx->stream));
    for (int k = 0; k < nb_layers; ++k) { t.src[k] = layers[k].d_covariances; t.dst[k] = layers[k].d_covariances_out; }
    HIPCHK(ctx, bcd_launch_spike_apply(t, nb_layers, d_map, W, H, 6, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_spike_apply_inplace(bcd_hip_ctx *ctx, const int32_t *d_map, int W, int H, const int32_t *depths, float *const *d_images, int nb_images, int32_t *h_moved)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_map) return bad(ctx, "null map pointer");
    if (!depths || !d_images) return bad(ctx, "null image or depth list");
    RCCHK(check_frame(ctx, W, H));
    if (nb_images < 1 || nb_images > BCD_SPIKE_MAX_IMAGES) return bad(ctx, "the number of images must be between 1 and 32");
    const size_t np = (size_t)W * H;
    BcdSpikeInplaceTable t = {};
    {
        std::vector<Range> r{ Range(d_map, np * sizeof(int32_t)) };
        for (int k = 0; k < nb_images; ++k) {
            if (!d_images[k]) return bad(ctx, "null image pointer in a list");
            if (depths[k] < 1) return bad(ctx, "the depth must be at least 1");
            if (depths[k] > BCD_SPIKE_INPLACE_MAX_DEPTH) return bad(ctx, "the depth must be at most 2^24");
            t.img[k] = d_images[k]; t.depth[k] = depths[k];
            r.push_back(Range(d_images[k], np * (size_t)depths[k] * sizeof(float)));
        }
        if (!all_apart(r)) return bad(ctx, "two images overlap, or an image overlaps the map");
    }
    DEVICE_GUARD(ctx);
    return spike_gather_inplace(ctx, d_map, np, t, nb_images, h_moved);
}

int bcd_hip_spike_filter_layers_inplace(bcd_hip_ctx *ctx, float *d_nsamples, float *d_histograms, int W, int H, int D, float factor,
                                        const bcd_hip_spike_layer_inplace *layers, int nb_layers, int32_t *d_map, int32_t *h_moved)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_nsamples) return bad(ctx, "null image pointer");
    if (!layers) return bad(ctx, "null layer list");
    if (nb_layers < 1 || nb_layers > BCD_HIP_MAX_LAYERS) return bad(ctx, "the number of layers must be between 1 and 16 (BCD_HIP_MAX_LAYERS)");
    for (int k = 0; k < nb_layers; ++k)
        if (!layers[k].d_colors || !layers[k].d_covariances) return bad(ctx, "null image pointer in a layer");
    RCCHK(check_frame(ctx, W, H));
    if (d_histograms && D < 1) return bad(ctx, "the depth must be at least 1");
    if (d_histograms && D > BCD_SPIKE_INPLACE_MAX_DEPTH) return bad(ctx, "the depth must be at most 2^24");
    const size_t np = (size_t)W * H, f = sizeof(float);
    float *col[BCD_HIP_MAX_LAYERS], *cov[BCD_HIP_MAX_LAYERS];
    {
        std::vector<Range> r{ Range(d_nsamples, np * f) };
        if (d_histograms) r.push_back(Range(d_histograms, np * D * f));
        for (int k = 0; k < nb_layers; ++k) {
            col[k] = layers[k].d_colors; cov[k] = layers[k].d_covariances;
            r.push_back(Range(col[k], np * 3 * f));
            r.push_back(Range(cov[k], np * 6 * f));
        }
        if (d_map) r.push_back(Range(d_map, np * sizeof(int32_t)));
        if (!all_apart(r)) return bad(ctx, "two images overlap, or an image overlaps the map");
    }
    DEVICE_GUARD(ctx);
    return spike_filter_frame_inplace(ctx, d_nsamples, d_histograms, W, H, D, factor, col, cov, nb_layers, d_map, h_moved);
}

} // extern "C"
