// bcd_sequence.hip -- a sequence denoised through a sliding window that reuses cross masks (bcd_hip_sequence_*, bcd_hip_transpose_masks_cross; DESIGN.md
// section 16, "Sequences").  The frame calls of bcd_temporal.hip denoise one frame and forget everything; called once per frame of an animation they search
// every pair of frames twice, build every frame's pyramid 2R + 1 times and (through the host entry points) upload every frame 2R + 1 times.  The sequence
// keeps the last 2R + 1 frames in a ring of slots -- a push copies the frame once and builds its pyramid levels and their per-pixel covariances once -- and
// the cross masks of every pair (a, b), a < b <= a + R, from the pop of frame a until the pop of frame b, which takes them through k_masks_transpose
// (k_masks_transpose.hip) instead of a second cross pass.  A push builds the levels with the reducers of the frame calls (temporal_build_level,
// guide_build_level); a pop runs the scales coarse to fine through the scale stage of the frame calls (temporal_scale, bcd_temporal.hip) with the slots'
// images, the pushes' per-pixel covariances and the sequence's members of TemporalSelFrame in its table, and merges them as the matching frame call does.
// A sequence in a mode (bcd_hip_sequence_create_mode; section 16, "Modes") holds L colour layers per slot, no histogram when it selects from means and
// covariances, and the levels of the feature pyramid when it gates: the moment and the feature cross distances are symmetric as the histogram distance is, the
// transposition distributes over the AND of the gate, so the kept (gated) masks are transposed as they are and a transposed neighbour runs neither a cross pass
// nor temporal_guide_gate.  There is one push, one pop and one construction: a sequence of bcd_hip_sequence_create is the mode of one layer, histograms and
// no gate; L > 1 or moments take the layered estimate (bayes_temporal_layers), one layer of histograms, gated or not, bayes_temporal.
// A frame may be pushed with its two step motion fields (bcd_hip_sequence_push_frame_motion; section 16, "Sequences with motion"): a pop then warps every
// neighbour whose direction has a field from its slot, as the motion frame calls warp it (pop_motion, warp_slot), composing the field of a neighbour two frames
// away from the steps (bcd_hip_compose_motion, k_motion_compose.hip); a pair is kept and transposed only when neither of its directions has a field.
#include "bcd_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#pragma GCC visibility push(hidden)
constexpr int SEQ_MAX_RADIUS = BCD_HIP_MAX_NEIGHBOURS / 2;
constexpr int SEQ_MAX_SLOTS = 2 * SEQ_MAX_RADIUS + 1;

struct SeqSlot {
    DevBuf lv[MAX_SCALES][4]; // per level: colours, sample counts, histograms, covariances ([0]: the copy of the pushed frame)
    DevBuf pixcov[MAX_SCALES]; // per level: the per-pixel covariances
    // ("Modes": colours, covariances and per-pixel covariances hold one slice per layer, [2] stays empty in a moments sequence)
    DevBuf guide[MAX_SCALES][2]; // per level, with the feature gate: the features and their variances
    DevBuf pair[SEQ_MAX_RADIUS][MAX_SCALES]; // [d - 1]: the cross masks of (this frame -> this frame + d) at every level
    int64_t pair_frame[SEQ_MAX_RADIUS];      // ... valid for this frame index (-1: not kept)
    DevBuf motion[2];                        // "Sequences with motion": the pushed step fields, [0] this frame -> the one before it, [1] -> the one after it
    bool has_motion[2] = { false, false };   // ... of the slot's frame (false: NULL was pushed, zero motion); the buffers exist from the first field on
};
// a neighbour of the pop in progress that has a field: its warped levels (in the buffers of ctx->temporal that the motion calls use) and their validity bytes
struct SeqWarped {
    bool on = false;
    TemporalFrame lv[MAX_SCALES];
    const uint8_t *valid[MAX_SCALES];
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
    // ---- the mode (bcd_hip_sequence_create_mode; DESIGN.md section 16, "Modes").  A sequence of bcd_hip_sequence_create is L = 1, histograms, no gate
    bool by_mode = false;                    // created by bcd_hip_sequence_create_mode: the _frame / _layers calls are open
    int L = 1, F = 0;                        // colour layers; feature channels (0: no gate)
    bool moments = false, fvar = false;      // selection from means and covariances (D = 0, no histogram stored); every frame brings feature variances
    float var_floor = 0.f, floors[BCD_GUIDE_MAX_CHANNELS] = {}, ftau = 0.f;
    int64_t feature_passes = 0;              // cross feature passes its pops launched
    // ---- the spike prefilter (bcd_hip_sequence_set_prefilter; DESIGN.md section 16, "Prefilter"): every frame is filtered once, in place in its slot, by its push
    float prefilter = 0.f;                   // the factor (0: off)
    int64_t filtered = 0, moved = 0;         // frames filtered, pixels they moved
    // ---- motion (bcd_hip_sequence_push_frame_motion; DESIGN.md section 16, "Sequences with motion"): a neighbour whose direction has a field is warped per pop
    DevBuf composed[2];                      // the fields frame t -> t - 2 and t -> t + 2 of the pop in progress, where both of their steps have a field
    SeqWarped warped[BCD_HIP_MAX_NEIGHBOURS + 1]; // [1..]: the neighbours of the pop in progress
    int64_t nb_warped = 0, nb_composed = 0;  // neighbours warped, fields composed by the pops
    bool plain() const { return L == 1 && !moments && F == 0; }   // what bcd_hip_sequence_create builds: its entry points, and it reports no layers
    bool layered() const { return moments || L > 1; }             // the estimate of bcd_temporal_layers.hip (one layer of histograms: that of bcd_temporal.hip)
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
    q->uploaded = q->pyramids = q->computed = q->transposed = q->feature_passes = q->filtered = q->moved = q->nb_warped = q->nb_composed = 0;
    for (SeqSlot &s : q->slot) for (int64_t &f : s.pair_frame) f = -1;
}

// the frames that can be popped now
int64_t ready_count(const bcd_hip_sequence *q)
{
    return q->ended ? q->pushed - q->popped : std::max<int64_t>(0, q->pushed - q->R - q->popped);
}

// slot sl at level s as temporal_build_level and temporal_scale see it: every image the mode stores, the layers as slices of the slot's buffers
TemporalFrame slot_level(const bcd_hip_sequence *q, const SeqSlot &sl, int s)
{
    const size_t np = (size_t)q->ws[s] * q->hs[s];
    TemporalFrame f;
    f.sel.ns = (const float *)sl.lv[s][1].p;
    f.sel.hist = q->moments ? nullptr : (const float *)sl.lv[s][2].p;
    if (q->F) { f.sel.feat = (const float *)sl.guide[s][0].p; f.sel.var = q->fvar ? (const float *)sl.guide[s][1].p : nullptr; }
    for (int k = 0; k < q->L; ++k) { f.col[k] = (const float *)sl.lv[s][0].p + k * np * 3; f.cov[k] = (const float *)sl.lv[s][3].p + k * np * 6; }
    f.pixcov = (float *)sl.pixcov[s].p;
    return f;
}

// a push, behind the refusals of its entry point: the frame's images into its slot (kind: device to device, or host to device), every pyramid level by the
// reducers of the matching frame call (temporal_build_level, guide_build_level), the per-pixel covariances of all layers of a level in one launch;
// synchronised, so the caller's buffers are free when it returns.  motion[0], motion[1]: null, or the step fields towards the frame before and after it, which
// are copied as they are (the prefilter does not move them)
int push_frame(bcd_hip_sequence *q, const bcd_hip_sequence_frame *fm, const float *const *motion, hipMemcpyKind kind)
{
    bcd_hip_ctx *ctx = q->ctx;
    if (q->ended) return bad(ctx, "the sequence has ended: no further frame can be pushed (bcd_hip_sequence_reset starts another)");
    if (q->pushed > q->popped + q->R) return bad(ctx, "pop first: the ring holds every frame the next pop needs");
    DEVICE_GUARD(ctx);
    hipStream_t st = ctx->main.stream;
    SeqSlot &sl = q->slot[q->pushed % q->N];
    const int D = q->D, L = q->L, F = q->F;
    const size_t f4 = sizeof(float);
    for (int s = 0; s < q->S; ++s) {
        const size_t np = (size_t)q->ws[s] * q->hs[s];
        RCCHK(seq_ensure(q, sl.lv[s][0], L * np * 3 * f4));
        RCCHK(seq_ensure(q, sl.lv[s][1], np * f4));
        if (!q->moments) RCCHK(seq_ensure(q, sl.lv[s][2], np * D * f4));
        RCCHK(seq_ensure(q, sl.lv[s][3], L * np * 6 * f4));
        RCCHK(seq_ensure(q, sl.pixcov[s], L * np * 6 * f4));
        if (F) RCCHK(seq_ensure(q, sl.guide[s][0], np * F * f4));
        if (F && q->fvar) RCCHK(seq_ensure(q, sl.guide[s][1], np * F * f4));
        const TemporalFrame l = slot_level(q, sl, s);
        if (s == 0) {
            int64_t bytes = (int64_t)(np * f4);
            HIPCHK(ctx, hipMemcpyAsync(sl.lv[0][1].p, fm->nsamples, np * f4, kind, st));
            if (!q->moments) { HIPCHK(ctx, hipMemcpyAsync(sl.lv[0][2].p, fm->histograms, np * D * f4, kind, st)); bytes += (int64_t)(np * D * f4); }
            for (int k = 0; k < L; ++k) {
                HIPCHK(ctx, hipMemcpyAsync(const_cast<float *>(l.col[k]), fm->layers[k].d_colors, np * 3 * f4, kind, st));
                HIPCHK(ctx, hipMemcpyAsync(const_cast<float *>(l.cov[k]), fm->layers[k].d_covariances, np * 6 * f4, kind, st));
                bytes += (int64_t)(np * 9 * f4);
            }
            if (F) { HIPCHK(ctx, hipMemcpyAsync(sl.guide[0][0].p, fm->features, np * F * f4, kind, st)); bytes += (int64_t)(np * F * f4); }
            if (F && q->fvar) { HIPCHK(ctx, hipMemcpyAsync(sl.guide[0][1].p, fm->variances, np * F * f4, kind, st)); bytes += (int64_t)(np * F * f4); }
            if (kind == hipMemcpyHostToDevice) q->uploaded += bytes;
            if (q->prefilter > 0.f) { // the frame's own decision, in place: the pyramid and the per-pixel covariances below come from the filtered level 0
                float *col[BCD_MAX_LAYERS], *cov[BCD_MAX_LAYERS];
                for (int k = 0; k < L; ++k) { col[k] = const_cast<float *>(l.col[k]); cov[k] = const_cast<float *>(l.cov[k]); }
                int32_t moved = 0;
                RCCHK(spike_filter_frame_inplace(ctx, (float *)sl.lv[0][1].p, q->moments ? nullptr : (float *)sl.lv[0][2].p, q->W, q->H, D, q->prefilter, col, cov, L, nullptr,
                                                 &moved));
                ++q->filtered;
                q->moved += moved;
            }
        } else {
            const TemporalFrame fine = slot_level(q, sl, s - 1);
            RCCHK(temporal_build_level(ctx, fine, l, L, q->layered(), q->ws[s - 1], q->hs[s - 1], D, st));
            if (F) RCCHK(guide_build_level(ctx, fine.sel.feat, fine.sel.var, q->ws[s - 1], q->hs[s - 1], F, (float *)sl.guide[s][0].p, (float *)sl.guide[s][1].p, st));
        }
        if (q->layered()) {
            BcdLayerTable t = {};
            for (int k = 0; k < L; ++k) t.a[k] = l.cov[k];
            HIPCHK(ctx, bcd_launch_layers_pixel_cov(t, L, l.sel.ns, (int64_t)np, l.pixcov, st));
        } else {
            HIPCHK(ctx, bcd_launch_pixel_cov(l.cov[0], l.sel.ns, (int64_t)np, l.pixcov, st));
        }
    }
    for (int64_t &f : sl.pair_frame) f = -1; // (the slot's earlier frame: its pairs were consumed R pops ago)
    for (int d = 0; d < 2; ++d) {
        const size_t bytes = (size_t)q->W * q->H * 2 * f4;
        sl.has_motion[d] = motion[d] != nullptr;
        if (!motion[d]) continue;
        RCCHK(seq_ensure(q, sl.motion[d], bytes));
        HIPCHK(ctx, hipMemcpyAsync(sl.motion[d].p, motion[d], bytes, kind, st));
        if (kind == hipMemcpyHostToDevice) q->uploaded += (int64_t)bytes;
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    ++q->pushed;
    ++q->pyramids;
    return BCD_HIP_OK;
}

// bcd_hip_sequence_push[_host]: its refusals, then the push of a frame of one layer
int push_images(bcd_hip_sequence *q, const float *col, const float *ns, const float *hist, const float *cov, hipMemcpyKind kind)
{
    if (!q) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = q->ctx;
    if (!q->plain()) return bad(ctx, "this sequence was created in a mode (bcd_hip_sequence_create_mode): its frames are pushed by bcd_hip_sequence_push_frame");
    if (!col || !ns || !hist || !cov) return bad(ctx, "null image pointer");
    const bcd_hip_frame_layer layer = { col, cov };
    const bcd_hip_sequence_frame fm = { ns, hist, &layer, nullptr, nullptr, nullptr };
    const float *const still[2] = { nullptr, nullptr };
    return push_frame(q, &fm, still, kind);
}

// bcd_hip_sequence_push_frame[_motion][_host]: its refusals, then the push (a push without fields is one with both fields NULL)
int push_mode_frame(bcd_hip_sequence *q, const bcd_hip_sequence_frame *fm, const float *motion_prev, const float *motion_next, hipMemcpyKind kind)
{
    if (!q) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = q->ctx;
    if (!q->by_mode) return bad(ctx, "this sequence was created by bcd_hip_sequence_create: its frames are pushed by bcd_hip_sequence_push");
    if (!fm) return bad(ctx, "null frame");
    if (fm->reserved) return bad(ctx, "the reserved pointer of a frame must be NULL");
    if (!fm->nsamples) return bad(ctx, "null image pointer");
    if (q->moments && fm->histograms) return bad(ctx, "a moments sequence takes no histograms: the frame's histograms must be NULL");
    if (!q->moments && !fm->histograms) return bad(ctx, "a histogram sequence needs the frame's histograms");
    if (!fm->layers) return bad(ctx, "null layer list");
    for (int k = 0; k < q->L; ++k) if (!fm->layers[k].d_colors || !fm->layers[k].d_covariances) return bad(ctx, "null image pointer in a layer");
    if (q->F == 0 && (fm->features || fm->variances)) return bad(ctx, "the sequence has no feature gate: the frame's features and variances must be NULL");
    if (q->F > 0 && !fm->features) return bad(ctx, "null feature image");
    if (q->F > 0 && (fm->variances != nullptr) != q->fvar) return bad(ctx, "feature variances must be given for every frame or for none, as the mode says");
    const float *const motion[2] = { motion_prev, motion_next };
    return push_frame(q, fm, motion, kind);
}

// One scale of a pop, frame t with the neighbours nbs[0 .. nn) in ascending order: the table of temporal_scale on the slots.  The per-pixel covariances are
// the pushes'; a neighbour above t is searched as the frame call searches it and its (gated) masks stay with the pair (t, f); one below takes the kept masks
// of (f, t) through the transposition; the in-frame masks are copied to self[s]
int pop_scale(bcd_hip_sequence *q, int64_t t, const int64_t *nbs, int nn, int s, const LayerView &out)
{
    bcd_hip_ctx *ctx = q->ctx;
    const int W = q->ws[s], H = q->hs[s], L = q->L;
    const size_t npix = (size_t)W * H, mb = mask_bytes(npix, q->prm.search_radius);
    TemporalScale sc;
    sc.nf = nn + 1; sc.L = L; sc.layered = q->layered(); sc.pixcov_ready = true;
    DevBuf &sum = sc.layered ? ctx->temporal.lay_sum : ctx->main.sum;
    RCCHK(ensure(ctx, sum, (size_t)L * npix * 3 * sizeof(float)));
    RCCHK(seq_ensure(q, q->self[s], mb));
    sc.sum = (float *)sum.p;
    sc.self_copy = (uint32_t *)q->self[s].p;
    for (int k = 0; k < L; ++k) sc.out[k] = out.out[k];
    SeqSlot &me = q->slot[t % q->N];
    sc.fr[0] = slot_level(q, me, s);
    for (int i = 1, below = 0; i <= nn; ++i) {
        const int64_t f = nbs[i - 1];
        SeqSlot &nb = q->slot[f % q->N];
        sc.fr[i] = slot_level(q, nb, s);
        const SeqWarped &wn = q->warped[i];
        if (wn.on) { // ("Sequences with motion": the warped level, its per-pixel covariances as the frame call computes them, the validity bytes for the gate)
            auto &tp = ctx->temporal;
            sc.fr[i] = wn.lv[s];
            DevBuf &pc = sc.layered ? tp.lay_pixcov[i] : tp.pixcov[i];
            RCCHK(ensure(ctx, pc, (size_t)L * npix * 6 * sizeof(float)));
            sc.fr[i].pixcov = (float *)pc.p;
            sc.fr[i].sel.valid = wn.valid[s];
            if (sc.layered) {
                BcdLayerTable lt = {};
                for (int k = 0; k < L; ++k) lt.a[k] = sc.fr[i].cov[k];
                HIPCHK(ctx, bcd_launch_layers_pixel_cov(lt, L, sc.fr[i].sel.ns, (int64_t)npix, sc.fr[i].pixcov, ctx->main.stream));
            } else {
                HIPCHK(ctx, bcd_launch_pixel_cov(sc.fr[i].cov[0], sc.fr[i].sel.ns, (int64_t)npix, sc.fr[i].pixcov, ctx->main.stream));
            }
        }
        DevBuf &dst = f > t ? me.pair[f - t - 1][s] : q->low[below++][s];
        RCCHK(seq_ensure(q, dst, mb));
        sc.fr[i].sel.mask_dst = (uint32_t *)dst.p;
        if (!wn.on && f < t && q->reuse && nb.pair_frame[t - f - 1] == f) sc.fr[i].sel.transpose_from = (const uint32_t *)nb.pair[t - f - 1][s].p;
    }
    return temporal_scale(ctx, sc, W, H, q->D, &q->prm, s);
}

// a frame without neighbours: the matching single-frame call on the slot's copies (a sequence of bcd_hip_sequence_create: the plain call, which reports no layers)
int pop_single(bcd_hip_sequence *q, const SeqSlot &me, float *const *d_out)
{
    bcd_hip_ctx *ctx = q->ctx;
    const size_t npix = (size_t)q->W * q->H;
    bcd_hip_layer lay[BCD_HIP_MAX_LAYERS];
    for (int k = 0; k < q->L; ++k) lay[k] = { (const float *)me.lv[0][0].p + k * npix * 3, (const float *)me.lv[0][3].p + k * npix * 6, d_out[k] };
    const float *ns = (const float *)me.lv[0][1].p, *hist = q->moments ? nullptr : (const float *)me.lv[0][2].p;
    if (q->plain()) return bcd_hip_denoise(ctx, lay[0].d_colors, ns, hist, lay[0].d_covariances, q->W, q->H, q->D, q->S, &q->prm, d_out[0]);
    if (q->F) {
        const bcd_hip_guide g = { (const float *)me.guide[0][0].p, q->fvar ? (const float *)me.guide[0][1].p : nullptr, q->F, q->floors, q->ftau };
        return bcd_hip_denoise_guided(ctx, ns, hist, q->W, q->H, q->D, q->S, &q->prm, q->var_floor, lay, q->L, &g, nullptr);
    }
    if (q->moments) return bcd_hip_denoise_moments(ctx, ns, q->W, q->H, q->S, &q->prm, q->var_floor, lay, q->L, nullptr);
    return bcd_hip_denoise_layers(ctx, ns, hist, q->W, q->H, q->D, q->S, &q->prm, lay, q->L);
}

// the scales of a pop, coarse to fine: the context carries the mode as it does inside the matching frame call (the moment selection, the guide's channels,
// floors and threshold) while they run.  A sequence in a mode reports its layers as the layered frame call does; one of bcd_hip_sequence_create, like
// bcd_hip_denoise_temporal, leaves ctx->layer_spectral and ctx->layer_count alone
int pop_scales(bcd_hip_sequence *q, int64_t t, const int64_t *nbs, int nn, float *const *d_out)
{
    bcd_hip_ctx *ctx = q->ctx;
    const int L = q->L, S = q->S;
    const bool layered = q->layered(), report_layers = !q->plain();
    auto &tp = ctx->temporal;
    struct ModeOn {
        bcd_hip_ctx *c;
        ModeOn(bcd_hip_ctx *ctx, const bcd_hip_sequence *q) : c(ctx)
        {
            if (q->F) {
                auto &G = c->guide;
                G.on = false; G.F = q->F; G.tau = q->ftau;
                for (int k = 0; k < BCD_GUIDE_MAX_CHANNELS; ++k) G.floors[k] = k < q->F ? q->floors[k] : 0.f;
            }
            c->temporal.guide.on = false; // (the slots' levels travel in TemporalSelFrame)
            c->moments.on = q->moments; c->moments.var_floor = q->var_floor;
        }
        ~ModeOn() { c->moments.on = false; }
    } mode_on(ctx, q);
    const int64_t passes = tp.guide_cross_passes;
    if (report_layers) {
        memset(ctx->layer_spectral, 0, sizeof(ctx->layer_spectral));
        ctx->layer_count = 0;
    }
    for (int s = 1; s < S; ++s) RCCHK(seq_ensure(q, q->out[s], (size_t)L * q->ws[s] * q->hs[s] * 3 * sizeof(float)));
    LayerView outs[MAX_SCALES];
    for (int s = 0; s < S; ++s) {
        outs[s].n = L;
        for (int k = 0; k < L; ++k) outs[s].out[k] = s == 0 ? d_out[k] : (float *)q->out[s].p + (size_t)k * q->ws[s] * q->hs[s] * 3;
    }
    int rc = BCD_HIP_OK;
    for (int s = S - 1; s >= 0 && rc == BCD_HIP_OK; --s) { // merged as in the matching frame call: the layers in one pair of launches, one layer of histograms by bcd_hip_merge
        rc = pop_scale(q, t, nbs, nn, s, outs[s]);
        if (rc != BCD_HIP_OK || s == S - 1) continue;
        rc = layered ? merge_layers_on(ctx, ctx->main, tp.lay_tmp_lo, outs[s], q->ws[s], q->hs[s], outs[s + 1])
                     : bcd_hip_merge(ctx, outs[s].out[0], q->ws[s], q->hs[s], outs[s + 1].out[0], 3);
    }
    q->feature_passes += tp.guide_cross_passes - passes;
    RCCHK(rc);
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
    if (!report_layers) return BCD_HIP_OK;
    if (!layered) for (int s = 0; s < S; ++s) ctx->layer_spectral[s][0] = ctx->stats[s].spectral_inverses; // (as the frame call of one layer reports it)
    ctx->layer_count = L;
    return BCD_HIP_OK;
}

// "Sequences with motion": the step fields whose composition is the field frame `from` -> frame `to` (1 or 2 frames apart, both in the ring): *a, then *b in the
// pixel order of the frame between them (null: zero motion; one step: *b is null)
void direction(const bcd_hip_sequence *q, int64_t from, int64_t to, const float **a, const float **b)
{
    const int d = to > from ? 1 : 0;
    const int64_t mid = to > from ? from + 1 : from - 1;
    auto step = [&](int64_t f) { const SeqSlot &s = q->slot[f % q->N]; return s.has_motion[d] ? (const float *)s.motion[d].p : nullptr; };
    *a = step(from);
    *b = mid == to ? nullptr : step(mid);
}

bool still(const bcd_hip_sequence *q, int64_t from, int64_t to)
{
    const float *a, *b;
    direction(q, from, to, &a, &b);
    return !a && !b;
}

// neighbour i (1..) of a pop with nf frames, in slot `nb`, reprojected by `field` as the matching frame call reprojects it: level 0 by temporal_warp_neighbour
// (further layers by k_warp_layers), the slot's features by bcd_launch_warp_features, the levels 1.. by the reducers of the frame calls
int warp_slot(bcd_hip_sequence *q, int i, int nf, const SeqSlot &nb, const float *field)
{
    bcd_hip_ctx *ctx = q->ctx;
    auto &tp = ctx->temporal;
    hipStream_t st = ctx->main.stream;
    const int W = q->W, H = q->H, D = q->D, S = q->S, L = q->L, F = q->F;
    const size_t npix = (size_t)W * H, f4 = sizeof(float);
    const bool layered = q->layered();
    SeqWarped &wn = q->warped[i];
    const TemporalFrame src = slot_level(q, nb, 0);
    BcdWarpLayerTable t = {};
    if (L > 1) {
        DevBuf(&lw)[2] = tp.lay_warp[i];
        RCCHK(ensure(ctx, lw[0], (size_t)(L - 1) * npix * 3 * f4));
        RCCHK(ensure(ctx, lw[1], (size_t)(L - 1) * npix * 6 * f4));
        for (int k = 1; k < L; ++k) {
            t.col[k - 1] = src.col[k]; t.cov[k - 1] = src.cov[k];
            t.ocol[k - 1] = (float *)lw[0].p + (size_t)(k - 1) * npix * 3; t.ocov[k - 1] = (float *)lw[1].p + (size_t)(k - 1) * npix * 6;
        }
    }
    TemporalFrame &l0 = wn.lv[0] = TemporalFrame();
    if (F) { // (the validity bytes it writes are written again below)
        DevBuf(&gw)[2] = tp.guide_warp[i];
        RCCHK(ensure(ctx, gw[0], npix * F * f4));
        if (q->fvar) RCCHK(ensure(ctx, gw[1], npix * F * f4));
        RCCHK(ensure(ctx, tp.valid[i][0], npix));
        HIPCHK(ctx, bcd_launch_warp_features(src.sel.feat, src.sel.var, F, field, W, H, (float *)gw[0].p, q->fvar ? (float *)gw[1].p : nullptr, (uint8_t *)tp.valid[i][0].p, st));
        l0.sel.feat = (const float *)gw[0].p;
        l0.sel.var = q->fvar ? (const float *)gw[1].p : nullptr;
    }
    const uint8_t *valid[MAX_SCALES * (BCD_HIP_MAX_NEIGHBOURS + 1)] = {};
    const float *wp[4];
    RCCHK(temporal_warp_neighbour(ctx, i, nf, src.col[0], src.sel.ns, src.sel.hist, src.cov[0], field, W, H, D, S, L > 1 ? &t : nullptr, L - 1, valid, wp));
    l0.col[0] = wp[0]; l0.sel.ns = wp[1]; l0.sel.hist = q->moments ? nullptr : wp[2]; l0.cov[0] = wp[3];
    for (int k = 1; k < L; ++k) { l0.col[k] = t.ocol[k - 1]; l0.cov[k] = t.ocov[k - 1]; }
    for (int s = 0; s < S; ++s) wn.valid[s] = valid[(size_t)s * nf + i];
    for (int s = 1; s < S; ++s) {
        const size_t np = (size_t)q->ws[s] * q->hs[s];
        DevBuf(&l)[4] = tp.pyr[i][s];
        TemporalFrame &coarse = wn.lv[s] = TemporalFrame();
        RCCHK(ensure(ctx, l[1], np * f4));
        if (!q->moments) RCCHK(ensure(ctx, l[2], np * D * f4));
        coarse.sel.ns = (const float *)l[1].p; coarse.sel.hist = q->moments ? nullptr : (const float *)l[2].p;
        if (layered) {
            DevBuf(&ll)[2] = tp.lay_pyr[i][s];
            RCCHK(ensure(ctx, ll[0], (size_t)L * np * 3 * f4));
            RCCHK(ensure(ctx, ll[1], (size_t)L * np * 6 * f4));
            for (int k = 0; k < L; ++k) { coarse.col[k] = (const float *)ll[0].p + (size_t)k * np * 3; coarse.cov[k] = (const float *)ll[1].p + (size_t)k * np * 6; }
        } else {
            RCCHK(ensure(ctx, l[0], np * 3 * f4));
            RCCHK(ensure(ctx, l[3], np * 6 * f4));
            coarse.col[0] = (const float *)l[0].p; coarse.cov[0] = (const float *)l[3].p;
        }
        RCCHK(temporal_build_level(ctx, wn.lv[s - 1], coarse, L, layered, q->ws[s - 1], q->hs[s - 1], D, st));
        if (F) {
            DevBuf(&g)[2] = tp.guide_pyr[i][s];
            RCCHK(ensure(ctx, g[0], np * F * f4));
            if (q->fvar) RCCHK(ensure(ctx, g[1], np * F * f4));
            RCCHK(guide_build_level(ctx, wn.lv[s - 1].sel.feat, wn.lv[s - 1].sel.var, q->ws[s - 1], q->hs[s - 1], F, (float *)g[0].p, (float *)g[1].p, st));
            coarse.sel.feat = (const float *)g[0].p;
            coarse.sel.var = q->fvar ? (const float *)g[1].p : nullptr;
        }
    }
    wn.on = true;
    ++q->nb_warped;
    return BCD_HIP_OK;
}

// the motion set-up of a pop: per neighbour the field of its direction -- a step field, or two of them composed -- and, where there is one, the warped neighbour
int pop_motion(bcd_hip_sequence *q, int64_t t, const int64_t *nbs, int nn)
{
    bcd_hip_ctx *ctx = q->ctx;
    for (SeqWarped &w : q->warped) w.on = false;
    for (int i = 1; i <= nn; ++i) {
        const int64_t f = nbs[i - 1];
        const float *a, *b;
        direction(q, t, f, &a, &b);
        const float *field = a ? a : b;
        if (a && b) {
            DevBuf &dst = q->composed[f > t ? 1 : 0];
            RCCHK(seq_ensure(q, dst, (size_t)q->W * q->H * 2 * sizeof(float)));
            HIPCHK(ctx, bcd_launch_motion_compose(a, b, q->W, q->H, (float *)dst.p, ctx->main.stream));
            ++q->nb_composed;
            field = (const float *)dst.p;
        }
        if (field) RCCHK(warp_slot(q, i, nn + 1, q->slot[f % q->N], field));
    }
    return BCD_HIP_OK;
}

// the next frame into d_out[0 .. L) (device memory)
int pop(bcd_hip_sequence *q, float *const *d_out, int64_t *frame_index)
{
    bcd_hip_ctx *ctx = q->ctx;
    const int64_t t = q->popped, last = q->pushed - 1;
    int64_t nbs[BCD_HIP_MAX_NEIGHBOURS];
    int nn = 0;
    for (int64_t f = std::max<int64_t>(0, t - q->R); f <= std::min(last, t + q->R); ++f) if (f != t) nbs[nn++] = f;
    SeqSlot &me = q->slot[t % q->N];
    if (nn == 0) {
        RCCHK(pop_single(q, me, d_out));
    } else {
        DEVICE_GUARD(ctx);
        RCCHK(pop_motion(q, t, nbs, nn));
        RCCHK(pop_scales(q, t, nbs, nn, d_out));
        for (int i = 0; i < nn; ++i) {
            const int64_t f = nbs[i];
            // (a pair is kept for the transposition exactly when neither of its directions has a field: frame f is in the ring, so both are known)
            if (f > t) { if (still(q, t, f) && still(q, f, t)) me.pair_frame[f - t - 1] = t; ++q->computed; continue; }
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

// what the two create calls share behind their own refusals of the mode: the refusals of the parameters, of the geometry and of the guide, then the sequence
int create(bcd_hip_ctx *ctx, int W, int H, int D, int nb_scales, int radius, const bcd_hip_params *prm, const bcd_hip_sequence_mode &mode, bool by_mode, void **out)
{
    const int L = mode.nb_layers, F = mode.nb_features;
    const bool moments = mode.moments == 1, fvar = mode.feature_variances == 1;
    RCCHK(check_params(ctx, W, H, moments ? 1 : D, prm)); // ("Moments": no histogram, D is not looked at)
    RCCHK(check_temporal_geometry(ctx, W, H, nb_scales, prm, true, &radius));
    if (F > 0) { // what bcd_hip_denoise_temporal_guided refuses of a guide (the images come with the frames: any address stands for them here)
        static const float present = 0.f;
        const bcd_hip_guide g = { &present, fvar ? &present : nullptr, F, mode.feature_floors, mode.feature_threshold };
        if ((int64_t)W * H >= (1ll << 31) / BCD_HIP_GUIDE_MAX_CHANNELS) return bad(ctx, "image too large for 32-bit DeepImage indices");
        RCCHK(check_guide(ctx, &g, prm->search_radius));
        if (bcd_pairdist_guide_cross_band(F, fvar, prm->search_radius) < 1) {
            set_err(ctx, "the cross feature distance kernel cannot be launched for this number of channels and search radius (LDS)");
            return BCD_HIP_EUNSUPPORTED;
        }
    }
    bcd_hip_sequence *q = new (std::nothrow) bcd_hip_sequence;
    if (!q) { set_err(ctx, "out of host memory"); return BCD_HIP_ENOMEM; }
    q->ctx = ctx;
    q->W = W; q->H = H; q->D = moments ? 0 : D; q->S = nb_scales; q->R = radius; q->N = 2 * radius + 1;
    q->prm = *prm;
    for (int s = 0; s < MAX_SCALES; ++s) { q->ws[s] = s ? q->ws[s - 1] / 2 : W; q->hs[s] = s ? q->hs[s - 1] / 2 : H; }
    q->by_mode = by_mode;
    q->L = L; q->F = F; q->moments = moments; q->fvar = fvar;
    q->var_floor = moments ? mode.var_floor : 0.f;
    for (int k = 0; k < F; ++k) q->floors[k] = mode.feature_floors[k];
    q->ftau = F ? mode.feature_threshold : 0.f;
    forget(q);
    *out = q;
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
    const bcd_hip_sequence_mode one_histogram_layer = { 1, 0, 0.f, 0, 0, nullptr, 0.f, nullptr };
    return create(ctx, W, H, D, nb_scales, radius, prm, one_histogram_layer, false, out);
}

int bcd_hip_sequence_push(void *seq, const float *d_colors, const float *d_nsamples, const float *d_histograms, const float *d_covariances)
{
    return push_images((bcd_hip_sequence *)seq, d_colors, d_nsamples, d_histograms, d_covariances, hipMemcpyDeviceToDevice);
}

int bcd_hip_sequence_push_host(void *seq, const float *h_colors, const float *h_nsamples, const float *h_histograms, const float *h_covariances)
{
    return push_images((bcd_hip_sequence *)seq, h_colors, h_nsamples, h_histograms, h_covariances, hipMemcpyHostToDevice);
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
    if (!q->plain()) return bad(q->ctx, "this sequence was created in a mode (bcd_hip_sequence_create_mode): its frames are popped by bcd_hip_sequence_pop_layers");
    RCCHK(check_pop(q, d_out));
    return pop(q, &d_out, frame_index);
}

// the layers of the next frame through the sequence's own device copy to host memory
static int pop_to_host(bcd_hip_sequence *q, float *const *h_out, int64_t *frame_index)
{
    bcd_hip_ctx *ctx = q->ctx;
    DEVICE_GUARD(ctx);
    const size_t bytes = (size_t)q->W * q->H * 3 * sizeof(float);
    RCCHK(seq_ensure(q, q->host_out, q->L * bytes));
    float *dev[BCD_HIP_MAX_LAYERS];
    for (int k = 0; k < q->L; ++k) dev[k] = (float *)q->host_out.p + (size_t)k * q->W * q->H * 3;
    RCCHK(pop(q, dev, frame_index));
    for (int k = 0; k < q->L; ++k) HIPCHK(ctx, hipMemcpyAsync(h_out[k], dev[k], bytes, hipMemcpyDeviceToHost, ctx->main.stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
    return BCD_HIP_OK;
}

int bcd_hip_sequence_pop_host(void *seq, float *h_out, int64_t *frame_index)
{
    bcd_hip_sequence *q = (bcd_hip_sequence *)seq;
    if (!q) return BCD_HIP_EINVAL;
    if (!q->plain()) return bad(q->ctx, "this sequence was created in a mode (bcd_hip_sequence_create_mode): its frames are popped by bcd_hip_sequence_pop_layers_host");
    RCCHK(check_pop(q, h_out));
    return pop_to_host(q, &h_out, frame_index);
}

// ---- "Modes": colour layers, the moment selection, the feature gate -------------------------------------------------------------
int bcd_hip_sequence_create_mode(bcd_hip_ctx *ctx, int W, int H, int D, int nb_scales, int radius, const bcd_hip_params *prm, const bcd_hip_sequence_mode *mode, void **out)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!out) return bad(ctx, "null handle pointer");
    *out = nullptr;
    if (!mode) return bad(ctx, "null mode");
    if (mode->reserved) return bad(ctx, "the reserved pointer of a mode must be NULL");
    const int L = mode->nb_layers, F = mode->nb_features;
    if (L < 1 || L > BCD_HIP_MAX_LAYERS) return bad(ctx, "the number of layers must be between 1 and 16 (BCD_HIP_MAX_LAYERS)");
    if (F < 0 || F > BCD_HIP_GUIDE_MAX_CHANNELS) return bad(ctx, "the number of feature channels must be between 1 and 8 (BCD_HIP_GUIDE_MAX_CHANNELS), or 0 for no feature gate");
    if ((mode->moments != 0 && mode->moments != 1) || (mode->feature_variances != 0 && mode->feature_variances != 1)) return bad(ctx, "the flags of a mode must be 0 or 1");
    const bool moments = mode->moments == 1, fvar = mode->feature_variances == 1;
    if (moments && (!(mode->var_floor >= 0.f) || !std::isfinite(mode->var_floor))) return bad(ctx, "the variance floor must be finite and not negative");
    if (F == 0 && fvar) return bad(ctx, "feature variances without feature channels");
    return create(ctx, W, H, D, nb_scales, radius, prm, *mode, true, out);
}

int bcd_hip_sequence_push_frame(void *seq, const bcd_hip_sequence_frame *frame) { return push_mode_frame((bcd_hip_sequence *)seq, frame, nullptr, nullptr, hipMemcpyDeviceToDevice); }

int bcd_hip_sequence_push_frame_host(void *seq, const bcd_hip_sequence_frame *frame) { return push_mode_frame((bcd_hip_sequence *)seq, frame, nullptr, nullptr, hipMemcpyHostToDevice); }

static int check_pop_layers(bcd_hip_sequence *q, float *const *outs, int nb_layers)
{
    bcd_hip_ctx *ctx = q->ctx;
    if (!q->by_mode) return bad(ctx, "this sequence was created by bcd_hip_sequence_create: its frames are popped by bcd_hip_sequence_pop");
    if (!outs) return bad(ctx, "null output list");
    if (nb_layers != q->L) return bad(ctx, "the number of outputs is not the number of layers of the sequence");
    for (int k = 0; k < nb_layers; ++k) {
        if (!outs[k]) return bad(ctx, "null output pointer");
        for (int j = 0; j < k; ++j)
            if (bytes_overlap(outs[k], (size_t)q->W * q->H * 3 * sizeof(float), outs[j], (size_t)q->W * q->H * 3 * sizeof(float))) return bad(ctx, "two layers share (part of) an output image");
    }
    return check_pop(q, outs[0]);
}

int bcd_hip_sequence_pop_layers(void *seq, float *const *d_outs, int nb_layers, int64_t *frame_index)
{
    bcd_hip_sequence *q = (bcd_hip_sequence *)seq;
    if (!q) return BCD_HIP_EINVAL;
    RCCHK(check_pop_layers(q, d_outs, nb_layers));
    return pop(q, d_outs, frame_index);
}

int bcd_hip_sequence_pop_layers_host(void *seq, float *const *h_outs, int nb_layers, int64_t *frame_index)
{
    bcd_hip_sequence *q = (bcd_hip_sequence *)seq;
    if (!q) return BCD_HIP_EINVAL;
    RCCHK(check_pop_layers(q, h_outs, nb_layers));
    return pop_to_host(q, h_outs, frame_index);
}

int bcd_hip_sequence_mode_info(void *seq, struct bcd_hip_sequence_mode_info *info)
{
    const bcd_hip_sequence *q = (const bcd_hip_sequence *)seq;
    if (!q) return BCD_HIP_EINVAL;
    if (!info) return bad(q->ctx, "null info pointer");
    info->nb_layers = q->L; info->moments = q->moments; info->nb_features = q->F; info->feature_variances = q->fvar;
    info->cross_feature_passes = q->feature_passes;
    info->reserved = 0;
    return BCD_HIP_OK;
}

int bcd_hip_sequence_set_reuse(void *seq, int on)
{
    bcd_hip_sequence *q = (bcd_hip_sequence *)seq;
    if (!q) return BCD_HIP_EINVAL;
    q->reuse = on != 0;
    return BCD_HIP_OK;
}

int bcd_hip_sequence_set_prefilter(void *seq, float factor)
{
    bcd_hip_sequence *q = (bcd_hip_sequence *)seq;
    if (!q) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = q->ctx;
    if (!std::isfinite(factor)) return bad(ctx, "the spike factor must be finite");
    if (q->pushed > 0) return bad(ctx, "the prefilter is set while the sequence holds no frame: after its creation or bcd_hip_sequence_reset");
    if (factor > 0.f && (q->W < 3 || q->H < 3)) return bad(ctx, "image smaller than 3x3");
    q->prefilter = factor > 0.f ? factor : 0.f;
    return BCD_HIP_OK;
}

int bcd_hip_sequence_prefilter_info(void *seq, int64_t *frames_filtered, int64_t *pixels_moved)
{
    const bcd_hip_sequence *q = (const bcd_hip_sequence *)seq;
    if (!q) return BCD_HIP_EINVAL;
    if (!frames_filtered || !pixels_moved) return bad(q->ctx, "null info pointer");
    *frames_filtered = q->filtered;
    *pixels_moved = q->moved;
    return BCD_HIP_OK;
}

// ---- "Sequences with motion"  --------------------------------------------------------------------------------------------------
int bcd_hip_compose_motion(bcd_hip_ctx *ctx, const float *d_a, const float *d_b, int W, int H, float *d_out)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!d_a || !d_b || !d_out) return bad(ctx, "null motion field pointer");
    if (W <= 0 || H <= 0) return bad(ctx, "empty image");
    if ((int64_t)W * H >= (1ll << 30)) return bad(ctx, "image too large for 32-bit DeepImage indices");
    const size_t bytes = (size_t)W * H * 2 * sizeof(float);
    if (bytes_overlap(d_out, bytes, d_a, bytes) || bytes_overlap(d_out, bytes, d_b, bytes)) return bad(ctx, "the composed field overlaps an input field (the composition is not done in place)");
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_motion_compose(d_a, d_b, W, H, d_out, ctx->main.stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
    return BCD_HIP_OK;
}

int bcd_hip_sequence_push_frame_motion(void *seq, const bcd_hip_sequence_frame *frame, const float *d_motion_prev, const float *d_motion_next)
{
    return push_mode_frame((bcd_hip_sequence *)seq, frame, d_motion_prev, d_motion_next, hipMemcpyDeviceToDevice);
}

int bcd_hip_sequence_push_frame_motion_host(void *seq, const bcd_hip_sequence_frame *frame, const float *h_motion_prev, const float *h_motion_next)
{
    return push_mode_frame((bcd_hip_sequence *)seq, frame, h_motion_prev, h_motion_next, hipMemcpyHostToDevice);
}

int bcd_hip_sequence_motion_info(void *seq, int64_t *neighbours_warped, int64_t *fields_composed)
{
    const bcd_hip_sequence *q = (const bcd_hip_sequence *)seq;
    if (!q) return BCD_HIP_EINVAL;
    if (!neighbours_warped || !fields_composed) return bad(q->ctx, "null info pointer");
    *neighbours_warped = q->nb_warped;
    *fields_composed = q->nb_composed;
    return BCD_HIP_OK;
}

int bcd_hip_sequence_last_masks(void *seq, int neighbour, int scale, uint32_t *d_mask, int32_t *d_count)
{
    bcd_hip_sequence *q = (bcd_hip_sequence *)seq;
    if (!q) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = q->ctx;
    if (!d_mask) return bad(ctx, "null mask pointer");
    if (q->last_frame < 0) return bad(ctx, "no frame has been popped");
    if (q->last_nb == 0)
        return bad(ctx, q->plain() ? "the last frame had no neighbour: it went through bcd_hip_denoise, which keeps no masks"
                                   : "the last frame had no neighbour: it went through the single-frame call of its mode, which keeps no masks");
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
        for (SeqSlot &s : q->slot) {
            free_bufs(s.lv, sizeof s.lv);
            free_bufs(s.pixcov, sizeof s.pixcov);
            free_bufs(s.guide, sizeof s.guide);
            free_bufs(s.pair, sizeof s.pair);
            free_bufs(s.motion, sizeof s.motion);
        }
        free_bufs(q->out, sizeof q->out);
        free_bufs(q->self, sizeof q->self);
        free_bufs(q->low, sizeof q->low);
        free_bufs(q->composed, sizeof q->composed);
        free_bufs(&q->host_out, sizeof q->host_out);
    }
    delete q;
}

} // extern "C"
