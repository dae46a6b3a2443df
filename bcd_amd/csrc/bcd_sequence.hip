// bcd_sequence.hip -- a sequence denoised through a sliding window that reuses cross masks (bcd_hip_sequence_*, bcd_hip_transpose_masks_cross; DESIGN.md
// section 16, "Sequences").  The frame calls of bcd_temporal.hip denoise one frame and forget everything; called once per frame of an animation they search
// every pair of frames twice, build every frame's pyramid 2R + 1 times and (through the host entry points) upload every frame 2R + 1 times.  The sequence
// keeps the last 2R + 1 frames in a ring of slots -- a push copies the frame once and builds its pyramid levels and their per-pixel covariances once -- and
// the cross masks of every pair (a, b), a < b <= a + R, from the pop of frame a until the pop of frame b, which takes them through k_masks_transpose
// (k_masks_transpose.hip) instead of a second cross pass.  A pop runs the scales coarse to fine through the code of the frame call: temporal_select (with the
// sequence's members of TemporalSelFrame), bayes_temporal, the finalisation, bcd_hip_merge.
#include "bcd_ctx.h"

#include <algorithm>
#include <cstring>
#include <new>

#pragma GCC visibility push(hidden)
constexpr int SEQ_MAX_RADIUS = BCD_HIP_MAX_NEIGHBOURS / 2;
constexpr int SEQ_MAX_SLOTS = 2 * SEQ_MAX_RADIUS + 1;

struct SeqSlot {
    DevBuf lv[MAX_SCALES][4]; // per level: colours, sample counts, histograms, covariances ([0]: the copy of the pushed frame)
    DevBuf pixcov[MAX_SCALES]; // per level: the per-pixel covariances
    DevBuf pair[SEQ_MAX_RADIUS][MAX_SCALES]; // [d - 1]: the cross masks of (this frame -> this frame + d) at every level
    int64_t pair_frame[SEQ_MAX_RADIUS];      // ... valid for this frame index (-1: not kept)
};
#pragma GCC visibility pop

struct bcd_hip_sequence {
    bcd_hip_ctx *ctx = nullptr;
    int W = 0, H = 0, D = 0, S = 0, R = 0, N = 0;
    bcd_hip_params prm;
    bool reuse = true, ended = false;
    int64_t pushed = 0, popped = 0;
    int ws[MAX_SCALES], hs[MAX_SCALES];
    SeqSlot slot[SEQ_MAX_SLOTS];
    DevBuf out[MAX_SCALES];                  // the outputs of the levels 1..
    DevBuf self[MAX_SCALES];                 // the in-frame masks of the last pop, per level (bcd_hip_sequence_last_masks)
    DevBuf low[SEQ_MAX_RADIUS][MAX_SCALES];  // the masks of its neighbours below it, per level
    DevBuf host_out;                         // bcd_hip_sequence_pop_host: the frame before its download
    int64_t last_frame = -1;                 // the last pop: its frame index, its neighbours in ascending order
    int last_nb = 0;
    int64_t last_nbs[BCD_HIP_MAX_NEIGHBOURS];
    int64_t held = 0, uploaded = 0, pyramids = 0, computed = 0, transposed = 0;
};

namespace {

size_t mask_bytes(size_t npix, int b) { return npix * (((size_t)(2 * b + 1) * (2 * b + 1) + 31) / 32) * sizeof(uint32_t); }

// ensure() on a buffer of the sequence, with the bytes held kept up to date
int seq_ensure(bcd_hip_sequence *q, DevBuf &b, size_t bytes)
{
    const size_t before = b.bytes;
    const int rc = ensure(q->ctx, b, bytes);
    q->held += (int64_t)b.bytes - (int64_t)before;
    return rc;
}

void forget(bcd_hip_sequence *q)
{
    q->pushed = q->popped = 0;
    q->ended = false;
    q->last_frame = -1; q->last_nb = 0;
    q->uploaded = q->pyramids = q->computed = q->transposed = 0;
    for (SeqSlot &s : q->slot) for (int64_t &f : s.pair_frame) f = -1;
}

// the frames that can be popped now
int64_t ready_count(const bcd_hip_sequence *q)
{
    return q->ended ? q->pushed - q->popped : std::max<int64_t>(0, q->pushed - q->R - q->popped);
}

// a push: the four images into the frame's slot (kind: device to device, or host to device), its pyramid levels by the reducers of temporal_run, the per-pixel
// covariances of every level; synchronised, so the caller's buffers are free when it returns
int push(bcd_hip_sequence *q, const float *col, const float *ns, const float *hist, const float *cov, hipMemcpyKind kind)
{
    if (!q) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = q->ctx;
    if (!col || !ns || !hist || !cov) return bad(ctx, "null image pointer");
    if (q->ended) return bad(ctx, "the sequence has ended: no further frame can be pushed (bcd_hip_sequence_reset starts another)");
    if (q->pushed > q->popped + q->R) return bad(ctx, "pop first: the ring holds every frame the next pop needs");
    DEVICE_GUARD(ctx);
    hipStream_t st = ctx->main.stream;
    SeqSlot &sl = q->slot[q->pushed % q->N];
    const int D = q->D;
    const float *src[4] = { col, ns, hist, cov };
    for (int s = 0; s < q->S; ++s) {
        const size_t np = (size_t)q->ws[s] * q->hs[s], bytes[4] = { np * 3 * sizeof(float), np * sizeof(float), np * D * sizeof(float), np * 6 * sizeof(float) };
        for (int k = 0; k < 4; ++k) RCCHK(seq_ensure(q, sl.lv[s][k], bytes[k]));
        RCCHK(seq_ensure(q, sl.pixcov[s], bytes[3]));
        float *l[4] = { (float *)sl.lv[s][0].p, (float *)sl.lv[s][1].p, (float *)sl.lv[s][2].p, (float *)sl.lv[s][3].p };
        if (s == 0) {
            for (int k = 0; k < 4; ++k) HIPCHK(ctx, hipMemcpyAsync(l[k], src[k], bytes[k], kind, st));
            if (kind == hipMemcpyHostToDevice) q->uploaded += (int64_t)(bytes[0] + bytes[1] + bytes[2] + bytes[3]);
        } else {
            const float *fine[4] = { (const float *)sl.lv[s - 1][0].p, (const float *)sl.lv[s - 1][1].p, (const float *)sl.lv[s - 1][2].p, (const float *)sl.lv[s - 1][3].p };
            HIPCHK(ctx, bcd_launch_downscale(1, fine[0], q->ws[s - 1], q->hs[s - 1], 3, l[0], st));
            HIPCHK(ctx, bcd_launch_downscale(0, fine[1], q->ws[s - 1], q->hs[s - 1], 1, l[1], st));
            HIPCHK(ctx, bcd_launch_downscale(0, fine[2], q->ws[s - 1], q->hs[s - 1], D, l[2], st));
            HIPCHK(ctx, bcd_launch_downscale_cov(fine[3], fine[1], q->ws[s - 1], q->hs[s - 1], l[3], st));
        }
        HIPCHK(ctx, bcd_launch_pixel_cov(l[3], l[1], (int64_t)np, (float *)sl.pixcov[s].p, st));
    }
    for (int64_t &f : sl.pair_frame) f = -1; // (the slot's earlier frame: its pairs were consumed R pops ago)
    HIPCHK(ctx, hipStreamSynchronize(st));
    ++q->pushed;
    ++q->pyramids;
    return BCD_HIP_OK;
}

// one scale of a pop: frame t with the neighbours nbs[0 .. nn) in ascending order
int pop_scale(bcd_hip_sequence *q, int64_t t, const int64_t *nbs, int nn, int s, float *d_out)
{
    bcd_hip_ctx *ctx = q->ctx;
    Work &wk = ctx->main;
    const int W = q->ws[s], H = q->hs[s], b = q->prm.search_radius, nf = nn + 1;
    const size_t npix = (size_t)W * H, mb = mask_bytes(npix, b);
    RCCHK(ensure(ctx, wk.sum, npix * 3 * sizeof(float)));
    RCCHK(seq_ensure(q, q->self[s], mb));
    const SeqSlot *fr[BCD_HIP_MAX_NEIGHBOURS + 1];
    TemporalSelFrame sel[BCD_HIP_MAX_NEIGHBOURS + 1];
    SeqSlot &me = q->slot[t % q->N];
    fr[0] = &me;
    sel[0] = { (const float *)me.lv[s][1].p, (const float *)me.lv[s][2].p, nullptr };
    for (int i = 1, below = 0; i < nf; ++i) {
        const int64_t f = nbs[i - 1];
        SeqSlot &nb = q->slot[f % q->N];
        fr[i] = &nb;
        sel[i] = { (const float *)nb.lv[s][1].p, (const float *)nb.lv[s][2].p, nullptr };
        if (f > t) { // searched as the frame call searches it; the masks stay with the pair (t, f)
            DevBuf &keep = me.pair[f - t - 1][s];
            RCCHK(seq_ensure(q, keep, mb));
            sel[i].mask_dst = (uint32_t *)keep.p;
        } else {     // the pair (f, t) was searched by the pop of f
            DevBuf &dst = q->low[below++][s];
            RCCHK(seq_ensure(q, dst, mb));
            sel[i].mask_dst = (uint32_t *)dst.p;
            if (q->reuse && nb.pair_frame[t - f - 1] == f) sel[i].transpose_from = (const uint32_t *)nb.pair[t - f - 1][s].p;
        }
    }
    TemporalPath path;
    RCCHK(temporal_select(ctx, sel, nf, W, H, q->D, &q->prm, s, []() -> int { return BCD_HIP_OK; } /* (computed by the pushes) */, &path));
    HIPCHK(ctx, hipMemcpyAsync(q->self[s].p, wk.mask.p, mb, hipMemcpyDeviceToDevice, wk.stream));
    BcdFrameTable tb = {};
    tb.n = nf;
    for (int i = 0; i < nf; ++i) {
        tb.col[i] = (const float *)fr[i]->lv[s][0].p;
        tb.pixcov[i] = (const float *)fr[i]->pixcov[s].p;
        tb.mask[i] = i == 0 ? (const uint32_t *)wk.mask.p : sel[i].mask_dst;
    }
    HIPCHK(ctx, hipMemsetAsync(wk.sum.p, 0, npix * 3 * sizeof(float), wk.stream));
    HIPCHK(ctx, hipMemsetAsync(wk.cnt.p, 0, npix * sizeof(int32_t), wk.stream));
    RCCHK(bayes_temporal(ctx, wk, tb, (const int32_t *)wk.nsim.p, (const uint8_t *)wk.state.p, W, H, b, q->prm.min_eigen_value, (float *)wk.sum.p, (int32_t *)wk.cnt.p));
    if (ctx->profiling) HIPCHK(ctx, hipEventRecord(wk.ev_stage[3], wk.stream));
    HIPCHK(ctx, bcd_launch_finalize((const float *)wk.sum.p, (const int32_t *)wk.cnt.p, (int64_t)npix, d_out, wk.stream));
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    temporal_stats_tail(ctx, s, path);
    return BCD_HIP_OK;
}

// the next frame into d_out (device memory)
int pop(bcd_hip_sequence *q, float *d_out, int64_t *frame_index)
{
    bcd_hip_ctx *ctx = q->ctx;
    const int64_t t = q->popped, last = q->pushed - 1;
    int64_t nbs[BCD_HIP_MAX_NEIGHBOURS];
    int nn = 0;
    for (int64_t f = std::max<int64_t>(0, t - q->R); f <= std::min(last, t + q->R); ++f) if (f != t) nbs[nn++] = f;
    SeqSlot &me = q->slot[t % q->N];
    if (nn == 0) { // a sequence of one frame: the plain call on the slot's copy
        RCCHK(bcd_hip_denoise(ctx, (const float *)me.lv[0][0].p, (const float *)me.lv[0][1].p, (const float *)me.lv[0][2].p, (const float *)me.lv[0][3].p, q->W, q->H, q->D,
                              q->S, &q->prm, d_out));
    } else {
        DEVICE_GUARD(ctx);
        for (int s = 1; s < q->S; ++s) RCCHK(seq_ensure(q, q->out[s], (size_t)q->ws[s] * q->hs[s] * 3 * sizeof(float)));
        for (int s = q->S - 1; s >= 0; --s) { // coarse to fine, merged as in bcd_hip_denoise_temporal
            float *out = s == 0 ? d_out : (float *)q->out[s].p;
            RCCHK(pop_scale(q, t, nbs, nn, s, out));
            if (s < q->S - 1) RCCHK(bcd_hip_merge(ctx, out, q->ws[s], q->hs[s], (const float *)q->out[s + 1].p, 3));
        }
        HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
        for (int i = 0; i < nn; ++i) {
            const int64_t f = nbs[i];
            if (f > t) { me.pair_frame[f - t - 1] = t; ++q->computed; continue; }
            int64_t &kept = q->slot[f % q->N].pair_frame[t - f - 1];
            if (q->reuse && kept == f) ++q->transposed; else ++q->computed;
            kept = -1; // (no later frame needs the pair)
        }
    }
    q->last_frame = t; q->last_nb = nn;
    for (int i = 0; i < nn; ++i) q->last_nbs[i] = nbs[i];
    if (frame_index) *frame_index = t;
    ++q->popped;
    return BCD_HIP_OK;
}

int check_pop(bcd_hip_sequence *q, const void *out)
{
    if (!out) return bad(q->ctx, "null output pointer");
    if (ready_count(q) < 1)
        return bad(q->ctx, q->popped == q->pushed ? "not ready: every pushed frame has been popped"
                                                  : "not ready: the next frame needs its later neighbours (push them, or call bcd_hip_sequence_end)");
    return BCD_HIP_OK;
}

} // namespace

extern "C" {

int bcd_hip_transpose_masks_cross(bcd_hip_ctx *ctx, const uint32_t *d_mask_in, int W, int H, int b, uint32_t *d_mask_out, int32_t *d_count_out)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_mask_in || !d_mask_out) return bad(ctx, "null mask pointer");
    if (W <= 0 || H <= 0) return bad(ctx, "empty image");
    if (b < 1) return bad(ctx, "the search radius must be at least 1");
    if (b > 6) { set_err(ctx, "the mask transposition supports search radius 1 to 6 (neighbour frames exist at search radius 6 only)"); return BCD_HIP_EUNSUPPORTED; }
    if ((int64_t)W * H >= (1ll << 31) / 6) return bad(ctx, "image too large for 32-bit DeepImage indices");
    const size_t npix = (size_t)W * H, mb = mask_bytes(npix, b);
    if (bytes_overlap(d_mask_out, mb, d_mask_in, mb)) return bad(ctx, "the output masks overlap the input masks (the transposition is not done in place)");
    if (d_count_out && (bytes_overlap(d_count_out, npix * 4, d_mask_in, mb) || bytes_overlap(d_count_out, npix * 4, d_mask_out, mb)))
        return bad(ctx, "the counts overlap the masks");
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_masks_transpose(d_mask_in, W, H, b, d_mask_out, d_count_out, ctx->main.stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
    return BCD_HIP_OK;
}

int bcd_hip_sequence_create(bcd_hip_ctx *ctx, int W, int H, int D, int nb_scales, int radius, const bcd_hip_params *prm, void **out)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!out) return bad(ctx, "null handle pointer");
    *out = nullptr;
    RCCHK(check_params(ctx, W, H, D, prm));
    if (nb_scales < 1 || nb_scales > MAX_SCALES) return bad(ctx, "bad number of scales");
    if (radius < 1 || radius > SEQ_MAX_RADIUS) return bad(ctx, "the temporal radius of a sequence must be 1 or 2 (2 radius <= BCD_HIP_MAX_NEIGHBOURS)");
    if (prm->patch_radius != 1 || prm->search_radius != 6) {
        set_err(ctx, "neighbour frames are supported with patch radius 1 and search radius 6");
        return BCD_HIP_EUNSUPPORTED;
    }
    for (int s = 1, ws = W, hs = H; s < nb_scales; ++s) {
        ws /= 2; hs /= 2;
        if (ws < 2 * prm->patch_radius + 1 || hs < 2 * prm->patch_radius + 1) return bad(ctx, "too many scales for this image size");
    }
    bcd_hip_sequence *q = new (std::nothrow) bcd_hip_sequence;
    if (!q) { set_err(ctx, "out of host memory"); return BCD_HIP_ENOMEM; }
    q->ctx = ctx;
    q->W = W; q->H = H; q->D = D; q->S = nb_scales; q->R = radius; q->N = 2 * radius + 1;
    q->prm = *prm;
    for (int s = 0; s < MAX_SCALES; ++s) { q->ws[s] = s ? q->ws[s - 1] / 2 : W; q->hs[s] = s ? q->hs[s - 1] / 2 : H; }
    forget(q);
    *out = q;
    return BCD_HIP_OK;
}

int bcd_hip_sequence_push(void *seq, const float *d_colors, const float *d_nsamples, const float *d_histograms, const float *d_covariances)
{
    return push((bcd_hip_sequence *)seq, d_colors, d_nsamples, d_histograms, d_covariances, hipMemcpyDeviceToDevice);
}

int bcd_hip_sequence_push_host(void *seq, const float *h_colors, const float *h_nsamples, const float *h_histograms, const float *h_covariances)
{
    return push((bcd_hip_sequence *)seq, h_colors, h_nsamples, h_histograms, h_covariances, hipMemcpyHostToDevice);
}

int bcd_hip_sequence_end(void *seq)
{
    bcd_hip_sequence *q = (bcd_hip_sequence *)seq;
    if (!q) return BCD_HIP_EINVAL;
    q->ended = true;
    return BCD_HIP_OK;
}

int bcd_hip_sequence_ready(void *seq)
{
    const bcd_hip_sequence *q = (const bcd_hip_sequence *)seq;
    return q ? (int)ready_count(q) : 0;
}

int bcd_hip_sequence_pop(void *seq, float *d_out, int64_t *frame_index)
{
    bcd_hip_sequence *q = (bcd_hip_sequence *)seq;
    if (!q) return BCD_HIP_EINVAL;
    RCCHK(check_pop(q, d_out));
    return pop(q, d_out, frame_index);
}

int bcd_hip_sequence_pop_host(void *seq, float *h_out, int64_t *frame_index)
{
    bcd_hip_sequence *q = (bcd_hip_sequence *)seq;
    if (!q) return BCD_HIP_EINVAL;
    RCCHK(check_pop(q, h_out));
    bcd_hip_ctx *ctx = q->ctx;
    DEVICE_GUARD(ctx);
    const size_t bytes = (size_t)q->W * q->H * 3 * sizeof(float);
    RCCHK(seq_ensure(q, q->host_out, bytes));
    RCCHK(pop(q, (float *)q->host_out.p, frame_index));
    HIPCHK(ctx, hipMemcpyAsync(h_out, q->host_out.p, bytes, hipMemcpyDeviceToHost, ctx->main.stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
    return BCD_HIP_OK;
}

int bcd_hip_sequence_set_reuse(void *seq, int on)
{
    bcd_hip_sequence *q = (bcd_hip_sequence *)seq;
    if (!q) return BCD_HIP_EINVAL;
    q->reuse = on != 0;
    return BCD_HIP_OK;
}

int bcd_hip_sequence_last_masks(void *seq, int neighbour, int scale, uint32_t *d_mask, int32_t *d_count)
{
    bcd_hip_sequence *q = (bcd_hip_sequence *)seq;
    if (!q) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = q->ctx;
    if (!d_mask) return bad(ctx, "null mask pointer");
    if (q->last_frame < 0) return bad(ctx, "no frame has been popped");
    if (q->last_nb == 0) return bad(ctx, "the last frame had no neighbour: it went through bcd_hip_denoise, which keeps no masks");
    if (neighbour < 0 || neighbour > q->last_nb) return bad(ctx, "no such neighbour of the last frame");
    if (scale < 0 || scale >= q->S) return bad(ctx, "no such scale");
    const int64_t t = q->last_frame;
    const DevBuf *src = &q->self[scale];
    if (neighbour > 0) {
        const int64_t f = q->last_nbs[neighbour - 1];
        src = f > t ? &q->slot[t % q->N].pair[f - t - 1][scale] : &q->low[neighbour - 1][scale]; // (the neighbours below come first)
    }
    const size_t npix = (size_t)q->ws[scale] * q->hs[scale], mb = mask_bytes(npix, q->prm.search_radius);
    if (d_count && bytes_overlap(d_count, npix * 4, d_mask, mb)) return bad(ctx, "the counts overlap the masks");
    DEVICE_GUARD(ctx);
    hipStream_t st = ctx->main.stream;
    HIPCHK(ctx, hipMemcpyAsync(d_mask, src->p, mb, hipMemcpyDeviceToDevice, st));
    if (d_count) HIPCHK(ctx, bcd_launch_mask_popcount((const uint32_t *)src->p, (int64_t)npix, (int)(mb / npix / sizeof(uint32_t)), d_count, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return BCD_HIP_OK;
}

int bcd_hip_sequence_info(void *seq, struct bcd_hip_sequence_info *info)
{
    const bcd_hip_sequence *q = (const bcd_hip_sequence *)seq;
    if (!q) return BCD_HIP_EINVAL;
    if (!info) return bad(q->ctx, "null info pointer");
    info->frames_pushed = q->pushed; info->frames_popped = q->popped;
    info->device_bytes = q->held;
    info->bytes_uploaded = q->uploaded;
    info->pyramids_built = q->pyramids;
    info->cross_computed = q->computed;
    info->cross_transposed = q->transposed;
    return BCD_HIP_OK;
}

int bcd_hip_sequence_reset(void *seq)
{
    bcd_hip_sequence *q = (bcd_hip_sequence *)seq;
    if (!q) return BCD_HIP_EINVAL;
    forget(q);
    return BCD_HIP_OK;
}

void bcd_hip_sequence_destroy(void *seq)
{
    bcd_hip_sequence *q = (bcd_hip_sequence *)seq;
    if (!q) return;
    {
        DeviceGuard guard(q->ctx);
        auto drop = [](DevBuf &b) { if (b.p) (void)hipFree(b.p); };
        for (SeqSlot &s : q->slot) {
            for (auto &level : s.lv) for (DevBuf &b : level) drop(b);
            for (DevBuf &b : s.pixcov) drop(b);
            for (auto &d : s.pair) for (DevBuf &b : d) drop(b);
        }
        for (DevBuf &b : q->out) drop(b);
        for (DevBuf &b : q->self) drop(b);
        for (auto &l : q->low) for (DevBuf &b : l) drop(b);
        drop(q->host_out);
    }
    delete q;
}

} // extern "C"
