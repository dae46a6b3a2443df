// bcd_accum.hip -- the persistent device SamplesAccumulator of the C ABI (bcd_hip_accum_*): its own handle type, which uses the context it was
// created on for the device, the stream and the error string only.
#include "bcd_ctx.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

extern "C" {

// ---- persistent device SamplesAccumulator (k_accumulate.hip) ----------------------------------------------------
struct bcd_hip_accum {
    bcd_hip_ctx *ctx = nullptr;
    int W = 0, H = 0, nbins = 0;
    float gamma = 0.f, maxval = 0.f;
    int64_t N = 0;
    DevBuf state;                  // (11 + 3 nbins) planes of N floats
    int nlayers = 0;               // extra colour layers (bcd_hip_accum_create_layers)
    DevBuf layers;                 // nlayers x 9 planes of N floats: 3 colour sums, 6 second moments, layer after layer
    int nfeat = 0;                 // auxiliary feature channels (bcd_hip_accum_create_features)
    DevBuf features;               // nfeat x 2 planes of N floats: the weighted sum and the weighted sum of squares, channel after channel
    DevBuf dropped;                // unsigned long long: scattered samples with an index outside [0, N)
    DevBuf keys[2], vals[2], sort; // scattered-add scratch (grow-only)
    int64_t capacity = 0;          // > 0: samples per sorted chunk, scratch allocated at create time
    int64_t submitted = 0;         // samples handed to add_* since the last reset
    DevBuf plan_red, plan_c, plan_ends, plan_err, plan_cnt, plan_tmp; // adaptive-plan scratch (allocated once per accumulator)
    bool plan_ready = false;       // the plan scratch is allocated (N is fixed, so it is never resized)
    // states (export / import / merge): two pinned staging chunks and two device chunks of at most STATE_CHUNK bytes, allocated on first
    // use; stage_busy[i]: a copy out of stage[i] may still be in flight (stage_ev[i] marks its end)
    void *stage[2] = { nullptr, nullptr };
    void *chunk[2] = { nullptr, nullptr };
    hipEvent_t stage_ev[2] = { nullptr, nullptr };
    bool stage_busy[2] = { false, false };
    size_t chunk_bytes = 0;
    hipEvent_t ev_merge = nullptr; // recorded on the context's stream around a merge (the source's work so far / the destination's reads)
    // reconstruction filter of the splatted add (bcd_hip_accum_set_filter): the parameters are kernel arguments, the table lives on the
    // device and is replaced in stream order through a pinned staging copy (filter_ev: that copy has left the staging buffer)
    bool has_filter = false;
    float filter_f[4] = { 0.f, 0.f, 0.f, 0.f }; // rx, ry, inv_rx, inv_ry
    int filter_g[5] = { 0, 0, 0, 0, 0 };        // table size, kx, ky, nx, ny
    DevBuf table, cells;                        // the table (64 x 64 floats at most); the runs of the extended frame's cells (grow-only)
    float *table_stage = nullptr;
    hipEvent_t filter_ev = nullptr;
    bool filter_busy = false;
};

namespace {

size_t accum_state_bytes(const bcd_hip_accum *a) { return (size_t)(11 + 3 * a->nbins) * (size_t)a->N * sizeof(float); }
size_t accum_layer_bytes(const bcd_hip_accum *a) { return (size_t)(9 * a->nlayers) * (size_t)a->N * sizeof(float); }
size_t accum_feature_bytes(const bcd_hip_accum *a) { return (size_t)(2 * a->nfeat) * (size_t)a->N * sizeof(float); }

// scratch of the scattered path for chunks of n samples
int accum_scratch(bcd_hip_accum *a, int64_t n)
{
    bcd_hip_ctx *ctx = a->ctx;
    for (int i = 0; i < 2; ++i) {
        RCCHK(ensure(ctx, a->keys[i], (size_t)n * sizeof(uint32_t)));
        RCCHK(ensure(ctx, a->vals[i], (size_t)n * sizeof(uint32_t)));
    }
    size_t bytes = 0;
    const int end_bit = 64 - __builtin_clzll((unsigned long long)a->N); // keys are <= N (N = dropped)
    HIPCHK(ctx, bcd_accum_sort(nullptr, &bytes, nullptr, nullptr, nullptr, nullptr, n, end_bit, ctx->stream));
    RCCHK(ensure(ctx, a->sort, bytes));
    return BCD_HIP_OK;
}

// scratch of the adaptive plan: reductions, C (uint64), ends (int32), the error and counts images used when the caller passes none, and
// the scans' temporary storage; the frame size is fixed, so this sizes and allocates once (a failed attempt is retried by the next plan)
int accum_plan_scratch(bcd_hip_accum *a)
{
    if (a->plan_ready) return BCD_HIP_OK;
    bcd_hip_ctx *ctx = a->ctx;
    const size_t N = (size_t)a->N;
    size_t tmp = 0;
    HIPCHK(ctx, bcd_plan_scan_bytes(a->N, &tmp));
    RCCHK(ensure(ctx, a->plan_red, bcd_plan_red_bytes()));
    RCCHK(ensure(ctx, a->plan_c, N * sizeof(uint64_t)));
    RCCHK(ensure(ctx, a->plan_ends, N * sizeof(int32_t)));
    RCCHK(ensure(ctx, a->plan_err, N * sizeof(float)));
    RCCHK(ensure(ctx, a->plan_cnt, N * sizeof(int32_t)));
    RCCHK(ensure(ctx, a->plan_tmp, tmp));
    a->plan_ready = true;
    return BCD_HIP_OK;
}

// cells of the frame extended by (kx, ky) on each side (the key space of the splatted add)
#define SPLAT_MAX_K 4
int64_t accum_extended_cells(const bcd_hip_accum *a, int kx, int ky) { return ((int64_t)a->W + 2 * kx) * ((int64_t)a->H + 2 * ky); }

// scratch of the splatted add for any filter, beside accum_scratch's: the cell runs and the sort's storage for the wider keys
int accum_splat_scratch(bcd_hip_accum *a)
{
    bcd_hip_ctx *ctx = a->ctx;
    const int64_t NE = accum_extended_cells(a, SPLAT_MAX_K, SPLAT_MAX_K);
    if (NE >= ((int64_t)1 << 32) - 1) return BCD_HIP_OK; // (set_filter refuses such frames)
    RCCHK(ensure(ctx, a->cells, (size_t)NE * 2 * sizeof(uint32_t)));
    size_t bytes = 0;
    HIPCHK(ctx, bcd_accum_sort(nullptr, &bytes, nullptr, nullptr, nullptr, nullptr, a->capacity, 64 - __builtin_clzll((unsigned long long)NE), ctx->stream));
    if (bytes > a->sort.bytes) RCCHK(ensure(ctx, a->sort, bytes));
    return BCD_HIP_OK;
}

} // namespace

// create, create_layers and create_features (nb_layers = 0: no layer planes; nb_features = 0: no feature planes)
static int accum_create(bcd_hip_ctx *ctx, int W, int H, int nb_bins, float gamma, float max_value, int64_t max_batch_samples, int nb_layers,
                        int nb_features, bcd_hip_accum **acc)
{
    if (W <= 0 || H <= 0 || (int64_t)W * H >= ((int64_t)1 << 31)) return bad(ctx, "frame size must be positive and below 2^31 pixels");
    if (nb_bins < 2) return bad(ctx, "nb_bins must be >= 2");
    if (bcd_accum_snapshot_lds(3 * nb_bins) > 64 * 1024) { set_err(ctx, "more than 85 bins per channel are not supported"); return BCD_HIP_EUNSUPPORTED; }
    if (max_batch_samples < 0 || max_batch_samples >= ((int64_t)1 << 31)) return bad(ctx, "max_batch_samples must be in [0, 2^31)");
    DEVICE_GUARD(ctx);
    bcd_hip_accum *a = new (std::nothrow) bcd_hip_accum();
    if (!a) { set_err(ctx, "out of host memory"); return BCD_HIP_ENOMEM; }
    a->ctx = ctx; a->W = W; a->H = H; a->nbins = nb_bins; a->gamma = gamma; a->maxval = max_value;
    a->N = (int64_t)W * H;
    a->capacity = max_batch_samples;
    a->nlayers = nb_layers;
    a->nfeat = nb_features;
    int rc = ensure(ctx, a->state, accum_state_bytes(a));
    if (rc == BCD_HIP_OK && nb_layers > 0) rc = ensure(ctx, a->layers, accum_layer_bytes(a));
    if (rc == BCD_HIP_OK && nb_features > 0) rc = ensure(ctx, a->features, accum_feature_bytes(a));
    if (rc == BCD_HIP_OK) rc = ensure(ctx, a->dropped, sizeof(unsigned long long));
    if (rc == BCD_HIP_OK && hipEventCreateWithFlags(&a->ev_merge, hipEventDisableTiming) != hipSuccess) {
        a->ev_merge = nullptr;
        set_err(ctx, "hipEventCreateWithFlags failed");
        rc = BCD_HIP_EDEVICE;
    }
    if (rc == BCD_HIP_OK && a->capacity > 0) rc = accum_scratch(a, a->capacity);
    if (rc == BCD_HIP_OK && a->capacity > 0) rc = accum_plan_scratch(a);
    if (rc == BCD_HIP_OK && a->capacity > 0) rc = accum_splat_scratch(a);
    if (rc == BCD_HIP_OK) rc = bcd_hip_accum_reset(a);
    if (rc != BCD_HIP_OK) { bcd_hip_accum_destroy(a); return rc; }
    *acc = a;
    return BCD_HIP_OK;
}

int bcd_hip_accum_create(bcd_hip_ctx *ctx, int W, int H, int nb_bins, float gamma, float max_value, int64_t max_batch_samples, bcd_hip_accum **acc)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!acc) return bad(ctx, "null accumulator handle");
    *acc = nullptr;
    return accum_create(ctx, W, H, nb_bins, gamma, max_value, max_batch_samples, 0, 0, acc);
}

int bcd_hip_accum_create_layers(bcd_hip_ctx *ctx, int W, int H, int nb_bins, float gamma, float max_value, int64_t max_batch_samples, int nb_layers,
                                bcd_hip_accum **acc)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!acc) return bad(ctx, "null accumulator handle");
    *acc = nullptr;
    if (nb_layers < 1 || nb_layers > BCD_HIP_ACCUM_MAX_LAYERS) return bad(ctx, "nb_layers must be in [1, 15]");
    return accum_create(ctx, W, H, nb_bins, gamma, max_value, max_batch_samples, nb_layers, 0, acc);
}

int bcd_hip_accum_create_features(bcd_hip_ctx *ctx, int W, int H, int nb_bins, float gamma, float max_value, int64_t max_batch_samples, int nb_layers,
                                  int nb_features, bcd_hip_accum **acc)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!acc) return bad(ctx, "null accumulator handle");
    *acc = nullptr;
    if (nb_layers < 0 || nb_layers > BCD_HIP_ACCUM_MAX_LAYERS) return bad(ctx, "nb_layers must be in [0, 15]");
    if (nb_features < 1 || nb_features > BCD_HIP_ACCUM_MAX_FEATURES) return bad(ctx, "nb_features must be in [1, 8]");
    return accum_create(ctx, W, H, nb_bins, gamma, max_value, max_batch_samples, nb_layers, nb_features, acc);
}

int bcd_hip_accum_nb_features(bcd_hip_accum *acc, int *nb_features)
{
    if (!acc) return BCD_HIP_EINVAL;
    if (!nb_features) return bad(acc->ctx, "null feature count");
    *nb_features = acc->nfeat;
    return BCD_HIP_OK;
}

int bcd_hip_accum_nb_layers(bcd_hip_accum *acc, int *nb_layers)
{
    if (!acc) return BCD_HIP_EINVAL;
    if (!nb_layers) return bad(acc->ctx, "null layer count");
    *nb_layers = acc->nlayers;
    return BCD_HIP_OK;
}

void bcd_hip_accum_destroy(bcd_hip_accum *acc)
{
    if (!acc) return;
    DeviceGuard guard(acc->ctx);
    (void)hipStreamSynchronize(acc->ctx->stream);
    for (DevBuf *b : { &acc->state, &acc->dropped, &acc->keys[0], &acc->keys[1], &acc->vals[0], &acc->vals[1], &acc->sort, &acc->plan_red,
                       &acc->plan_c, &acc->plan_ends, &acc->plan_err, &acc->plan_cnt, &acc->plan_tmp })
        if (b->p) (void)hipFree(b->p);
    for (DevBuf *b : { &acc->table, &acc->cells, &acc->layers, &acc->features })
        if (b->p) (void)hipFree(b->p);
    if (acc->table_stage) (void)hipHostFree(acc->table_stage);
    if (acc->filter_ev) (void)hipEventDestroy(acc->filter_ev);
    for (int i = 0; i < 2; ++i) {
        if (acc->stage[i]) (void)hipHostFree(acc->stage[i]);
        if (acc->chunk[i]) (void)hipFree(acc->chunk[i]);
        if (acc->stage_ev[i]) (void)hipEventDestroy(acc->stage_ev[i]);
    }
    if (acc->ev_merge) (void)hipEventDestroy(acc->ev_merge);
    delete acc;
}

int bcd_hip_accum_reset(bcd_hip_accum *acc)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, hipMemsetAsync(acc->state.p, 0, accum_state_bytes(acc), ctx->stream));
    if (acc->nlayers > 0) HIPCHK(ctx, hipMemsetAsync(acc->layers.p, 0, accum_layer_bytes(acc), ctx->stream));
    if (acc->nfeat > 0) HIPCHK(ctx, hipMemsetAsync(acc->features.p, 0, accum_feature_bytes(acc), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(acc->dropped.p, 0, sizeof(unsigned long long), ctx->stream));
    acc->submitted = 0;
    return BCD_HIP_OK;
}

namespace {

// the refusals of the adds: a plain add would move a layered accumulator's weight sums without its layers
int accum_check_layered(bcd_hip_accum *acc, bool layered_call)
{
    if (acc->nfeat > 0) return bad(acc->ctx, "the accumulator has feature channels: use the _features form of this add");
    if (layered_call && acc->nlayers == 0) return bad(acc->ctx, "the accumulator has no layers (bcd_hip_accum_create_layers)");
    if (!layered_call && acc->nlayers > 0) return bad(acc->ctx, "the accumulator has colour layers: use the _layers form of this add");
    return BCD_HIP_OK;
}

// the refusals of a _features add: the layer list is there exactly when the accumulator has layers
int accum_check_featured(bcd_hip_accum *acc, const float *const *d_layers)
{
    if (acc->nfeat == 0) return bad(acc->ctx, "the accumulator has no feature channels (bcd_hip_accum_create_features)");
    if (d_layers && acc->nlayers == 0) return bad(acc->ctx, "a layer list on an accumulator without layers");
    return BCD_HIP_OK;
}

// the layers' pointer list of a _layers add (host array of nlayers device pointers) into a table, each advanced by `offset` floats
int accum_layer_table(bcd_hip_accum *acc, const float *const *d_layers, BcdAccumLayerIn &in)
{
    if (!d_layers) return bad(acc->ctx, "null layer list");
    for (int l = 0; l < BCD_ACCUM_MAX_LAYERS; ++l) in.src[l] = nullptr;
    for (int l = 0; l < acc->nlayers; ++l) {
        if (!d_layers[l]) return bad(acc->ctx, "null layer samples");
        in.src[l] = d_layers[l];
    }
    return BCD_HIP_OK;
}

BcdAccumLayerIn accum_layer_offset(const bcd_hip_accum *acc, const BcdAccumLayerIn &in, int64_t offset)
{
    BcdAccumLayerIn o = in;
    for (int l = 0; l < acc->nlayers; ++l) o.src[l] = in.src[l] + offset;
    return o;
}

// the three adds; layers: the table of a _layers call, or nullptr on an accumulator without layers; d_features: the samples' feature
// channels on an accumulator with features (never null there), laid out like the beauty's samples of the call
int accum_add_dense(bcd_hip_accum *acc, const float *d_samples, const float *d_weights, int row_begin, int rows, int spp, int channels,
                    const float *const *d_layer_samples, int layer_channels, const float *d_features);
int accum_add_scattered(bcd_hip_accum *acc, const int32_t *d_pixel, const float *d_rgb, const float *d_weights, int64_t n, const float *const *d_layer_rgb,
                        const float *d_features);
int accum_add_splatted(bcd_hip_accum *acc, const float *d_xy, const float *d_rgb, const float *d_weights, int64_t n, const float *const *d_layer_rgb,
                       const float *d_features);

} // namespace

int bcd_hip_accum_add_dense(bcd_hip_accum *acc, const float *d_samples, const float *d_weights, int row_begin, int rows, int spp, int channels)
{
    if (!acc) return BCD_HIP_EINVAL;
    RCCHK(accum_check_layered(acc, false));
    return accum_add_dense(acc, d_samples, d_weights, row_begin, rows, spp, channels, nullptr, 3, nullptr);
}

int bcd_hip_accum_add_dense_layers(bcd_hip_accum *acc, const float *d_samples, const float *d_weights, int row_begin, int rows, int spp, int channels,
                                   const float *const *d_layer_samples, int layer_channels)
{
    if (!acc) return BCD_HIP_EINVAL;
    RCCHK(accum_check_layered(acc, true));
    return accum_add_dense(acc, d_samples, d_weights, row_begin, rows, spp, channels, d_layer_samples, layer_channels, nullptr);
}

int bcd_hip_accum_add_scattered(bcd_hip_accum *acc, const int32_t *d_pixel, const float *d_rgb, const float *d_weights, int64_t n)
{
    if (!acc) return BCD_HIP_EINVAL;
    RCCHK(accum_check_layered(acc, false));
    return accum_add_scattered(acc, d_pixel, d_rgb, d_weights, n, nullptr, nullptr);
}

int bcd_hip_accum_add_scattered_layers(bcd_hip_accum *acc, const int32_t *d_pixel, const float *d_rgb, const float *d_weights, int64_t n,
                                       const float *const *d_layer_rgb)
{
    if (!acc) return BCD_HIP_EINVAL;
    RCCHK(accum_check_layered(acc, true));
    return accum_add_scattered(acc, d_pixel, d_rgb, d_weights, n, d_layer_rgb, nullptr);
}

int bcd_hip_accum_add_splatted(bcd_hip_accum *acc, const float *d_xy, const float *d_rgb, const float *d_weights, int64_t n)
{
    if (!acc) return BCD_HIP_EINVAL;
    RCCHK(accum_check_layered(acc, false));
    return accum_add_splatted(acc, d_xy, d_rgb, d_weights, n, nullptr, nullptr);
}

int bcd_hip_accum_add_splatted_layers(bcd_hip_accum *acc, const float *d_xy, const float *d_rgb, const float *d_weights, int64_t n,
                                      const float *const *d_layer_rgb)
{
    if (!acc) return BCD_HIP_EINVAL;
    RCCHK(accum_check_layered(acc, true));
    return accum_add_splatted(acc, d_xy, d_rgb, d_weights, n, d_layer_rgb, nullptr);
}

int bcd_hip_accum_add_dense_features(bcd_hip_accum *acc, const float *d_samples, const float *d_weights, int row_begin, int rows, int spp, int channels,
                                     const float *const *d_layer_samples, int layer_channels, const float *d_features)
{
    if (!acc) return BCD_HIP_EINVAL;
    RCCHK(accum_check_featured(acc, d_layer_samples));
    if (!d_features) return bad(acc->ctx, "null features");
    return accum_add_dense(acc, d_samples, d_weights, row_begin, rows, spp, channels, d_layer_samples, layer_channels, d_features);
}

int bcd_hip_accum_add_scattered_features(bcd_hip_accum *acc, const int32_t *d_pixel, const float *d_rgb, const float *d_weights, int64_t n,
                                         const float *const *d_layer_rgb, const float *d_features)
{
    if (!acc) return BCD_HIP_EINVAL;
    RCCHK(accum_check_featured(acc, d_layer_rgb));
    if (n > 0 && !d_features) return bad(acc->ctx, "null features");
    return accum_add_scattered(acc, d_pixel, d_rgb, d_weights, n, d_layer_rgb, d_features);
}

int bcd_hip_accum_add_splatted_features(bcd_hip_accum *acc, const float *d_xy, const float *d_rgb, const float *d_weights, int64_t n,
                                        const float *const *d_layer_rgb, const float *d_features)
{
    if (!acc) return BCD_HIP_EINVAL;
    RCCHK(accum_check_featured(acc, d_layer_rgb));
    if (n > 0 && !d_features) return bad(acc->ctx, "null features");
    return accum_add_splatted(acc, d_xy, d_rgb, d_weights, n, d_layer_rgb, d_features);
}

namespace {

int accum_add_dense(bcd_hip_accum *acc, const float *d_samples, const float *d_weights, int row_begin, int rows, int spp, int channels,
                    const float *const *d_layer_samples, int layer_channels, const float *d_features)
{
    bcd_hip_ctx *ctx = acc->ctx;
    if (!d_samples) return bad(ctx, "null samples");
    if (channels != 3 && channels != 4) return bad(ctx, "channels must be 3 or 4");
    if (layer_channels != 3 && layer_channels != 4) return bad(ctx, "layer_channels must be 3 or 4");
    if (spp < 1) return bad(ctx, "spp must be >= 1");
    if (rows < 1 || row_begin < 0 || row_begin > acc->H - rows) return bad(ctx, "row range outside the frame");
    BcdAccumLayerIn in;
    if (acc->nlayers > 0) RCCHK(accum_layer_table(acc, d_layer_samples, in));
    DEVICE_GUARD(ctx);
    const int64_t npix = (int64_t)rows * acc->W;
    HIPCHK(ctx, bcd_launch_accum_dense(d_samples, d_weights, (int64_t)row_begin * acc->W, npix, acc->N, spp, channels, acc->nbins, acc->gamma,
                                       acc->maxval, (float *)acc->state.p, ctx->stream));
    if (acc->nlayers > 0)
        HIPCHK(ctx, bcd_launch_accum_dense_layers(in, acc->nlayers, d_weights, (int64_t)row_begin * acc->W, npix, acc->N, spp, layer_channels,
                                                  (float *)acc->layers.p, ctx->stream));
    if (acc->nfeat > 0)
        HIPCHK(ctx, bcd_launch_feat_dense(d_features, acc->nfeat, d_weights, (int64_t)row_begin * acc->W, npix, acc->N, spp, (float *)acc->features.p,
                                          ctx->stream));
    acc->submitted += npix * spp;
    return BCD_HIP_OK;
}

int accum_add_scattered(bcd_hip_accum *acc, const int32_t *d_pixel, const float *d_rgb, const float *d_weights, int64_t n, const float *const *d_layer_rgb,
                        const float *d_features)
{
    bcd_hip_ctx *ctx = acc->ctx;
    if (n < 0) return bad(ctx, "negative sample count");
    if (n == 0) return BCD_HIP_OK;
    if (!d_pixel || !d_rgb) return bad(ctx, "null samples");
    BcdAccumLayerIn in;
    if (acc->nlayers > 0) RCCHK(accum_layer_table(acc, d_layer_rgb, in));
    DEVICE_GUARD(ctx);
    const int64_t chunk = acc->capacity > 0 ? acc->capacity : std::min<int64_t>(n, (int64_t)1 << 30);
    if (acc->capacity == 0) RCCHK(accum_scratch(acc, std::min(n, chunk)));
    const int end_bit = 64 - __builtin_clzll((unsigned long long)acc->N);
    uint32_t *k0 = (uint32_t *)acc->keys[0].p, *k1 = (uint32_t *)acc->keys[1].p, *v0 = (uint32_t *)acc->vals[0].p, *v1 = (uint32_t *)acc->vals[1].p;
    for (int64_t b = 0; b < n; b += chunk) { // chunks in stream order: a pixel's samples of chunk c are applied after those of chunk c - 1
        const int64_t m = std::min(chunk, n - b);
        size_t bytes = acc->sort.bytes;
        HIPCHK(ctx, bcd_launch_accum_keys(d_pixel + b, m, acc->N, k0, v0, (unsigned long long *)acc->dropped.p, ctx->stream));
        HIPCHK(ctx, bcd_accum_sort(acc->sort.p, &bytes, k0, k1, v0, v1, m, end_bit, ctx->stream));
        HIPCHK(ctx, bcd_launch_accum_segments(k1, v1, m, acc->N, d_rgb + b * 3, d_weights ? d_weights + b : nullptr, acc->nbins, acc->gamma,
                                              acc->maxval, (float *)acc->state.p, ctx->stream));
        if (acc->nlayers > 0) // (on the chunk's sorted keys and values, before the next chunk overwrites them)
            HIPCHK(ctx, bcd_launch_accum_segments_layers(k1, v1, m, acc->N, accum_layer_offset(acc, in, b * 3), acc->nlayers,
                                                         d_weights ? d_weights + b : nullptr, (float *)acc->layers.p, ctx->stream));
        if (acc->nfeat > 0) // (the features too)
            HIPCHK(ctx, bcd_launch_feat_segments(k1, v1, m, acc->N, d_features + b * acc->nfeat, acc->nfeat, d_weights ? d_weights + b : nullptr,
                                                 (float *)acc->features.p, ctx->stream));
    }
    acc->submitted += n;
    return BCD_HIP_OK;
}

} // namespace

int bcd_hip_accum_set_filter(bcd_hip_accum *acc, float radius_x, float radius_y, int table_size, const float *h_table)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    if (!h_table) { acc->has_filter = false; return BCD_HIP_OK; }
    if (!(radius_x > 0.f && radius_x <= 3.f) || !(radius_y > 0.f && radius_y <= 3.f)) return bad(ctx, "filter radii must be in (0, 3]");
    if (table_size < 1 || table_size > 64) return bad(ctx, "filter table size must be in [1, 64]");
    const int tt = table_size * table_size;
    for (int i = 0; i < tt; ++i)
        if (!std::isfinite(h_table[i]) || h_table[i] < 0.f)
            return bad(ctx, "filter table entries must be finite and >= 0 (filters with negative lobes are not supported)");
    const int kx = (int)ceilf(radius_x + 0.5f), ky = (int)ceilf(radius_y + 0.5f);
    // (col + 0.5f must be exact for the kernel's neighbour range, and the cells' keys are 32 bits wide)
    if (accum_extended_cells(acc, kx, ky) >= ((int64_t)1 << 32) - 1 || std::max(acc->W, acc->H) >= (1 << 22)) {
        set_err(ctx, "frames of 2^22 pixels or more on a side are not supported with a filter");
        return BCD_HIP_EUNSUPPORTED;
    }
    DEVICE_GUARD(ctx);
    RCCHK(ensure(ctx, acc->table, 64 * 64 * sizeof(float)));
    if (!acc->table_stage) HIPCHK(ctx, hipHostMalloc((void **)&acc->table_stage, 64 * 64 * sizeof(float), hipHostMallocDefault));
    if (!acc->filter_ev) HIPCHK(ctx, hipEventCreateWithFlags(&acc->filter_ev, hipEventDisableTiming));
    if (acc->filter_busy) { HIPCHK(ctx, hipEventSynchronize(acc->filter_ev)); acc->filter_busy = false; }
    std::memcpy(acc->table_stage, h_table, (size_t)tt * sizeof(float));
    HIPCHK(ctx, hipMemcpyAsync(acc->table.p, acc->table_stage, (size_t)tt * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(acc->filter_ev, ctx->stream));
    acc->filter_busy = true;
    // cells further than n from a pixel hold no sample within the radius: a sample of a cell at offset n + 1 is at least n + 0.5 away
    // (exactly representable, and the rounded subtraction is monotone), so n is the smallest integer with n + 0.5 >= r -- never more
    // than K, the candidate range of the definition
    int nx = 0, ny = 0;
    while ((float)nx + 0.5f < radius_x) ++nx;
    while ((float)ny + 0.5f < radius_y) ++ny;
    acc->filter_f[0] = radius_x; acc->filter_f[1] = radius_y; acc->filter_f[2] = 1.f / radius_x; acc->filter_f[3] = 1.f / radius_y;
    acc->filter_g[0] = table_size; acc->filter_g[1] = kx; acc->filter_g[2] = ky;
    acc->filter_g[3] = std::min(nx, kx); acc->filter_g[4] = std::min(ny, ky);
    acc->has_filter = true;
    return BCD_HIP_OK;
}

namespace {

int accum_add_splatted(bcd_hip_accum *acc, const float *d_xy, const float *d_rgb, const float *d_weights, int64_t n, const float *const *d_layer_rgb,
                       const float *d_features)
{
    bcd_hip_ctx *ctx = acc->ctx;
    if (!acc->has_filter) return bad(ctx, "the accumulator has no filter (bcd_hip_accum_set_filter)");
    if (n < 0) return bad(ctx, "negative sample count");
    if (n == 0) return BCD_HIP_OK;
    if (!d_xy || !d_rgb) return bad(ctx, "null samples");
    BcdAccumLayerIn in;
    if (acc->nlayers > 0) RCCHK(accum_layer_table(acc, d_layer_rgb, in));
    DEVICE_GUARD(ctx);
    const int *g = acc->filter_g;
    const int64_t NE = accum_extended_cells(acc, g[1], g[2]);
    // a chunk holds at most as many samples as keep the average ring of a tile within 0.55 of the staging arrays (chunks are applied in
    // stream order, so splitting a batch changes no bit); denser tiles take the kernel's global-memory path
    const int max_staged = bcd_splat_max_staged(g[0]), ring = bcd_splat_ring_cells(g[3], g[4]);
    const int64_t dense = std::max<int64_t>((int64_t)1 << 16, (int64_t)((double)acc->N * 0.55 * max_staged / ring));
    const int64_t chunk = std::min(dense, acc->capacity > 0 ? acc->capacity : std::min<int64_t>(n, (int64_t)1 << 30));
    if (acc->capacity == 0) RCCHK(accum_scratch(acc, std::min(n, chunk)));
    RCCHK(ensure(ctx, acc->cells, (size_t)NE * 2 * sizeof(uint32_t)));
    const int end_bit = 64 - __builtin_clzll((unsigned long long)NE); // keys are <= NE (NE = dropped)
    size_t need = 0;
    HIPCHK(ctx, bcd_accum_sort(nullptr, &need, nullptr, nullptr, nullptr, nullptr, std::min(n, chunk), end_bit, ctx->stream));
    RCCHK(ensure(ctx, acc->sort, need)); // (more key bits than the scattered add's: the storage may differ)
    uint32_t *k0 = (uint32_t *)acc->keys[0].p, *k1 = (uint32_t *)acc->keys[1].p, *v0 = (uint32_t *)acc->vals[0].p, *v1 = (uint32_t *)acc->vals[1].p;
    for (int64_t b = 0; b < n; b += chunk) {
        const int64_t m = std::min(chunk, n - b);
        const float *xy = d_xy + 2 * b, *rgb = d_rgb + 3 * b, *w = d_weights ? d_weights + b : nullptr;
        size_t bytes = acc->sort.bytes;
        HIPCHK(ctx, bcd_launch_splat_keys(xy, m, acc->W, acc->H, acc->filter_f, g, (const float *)acc->table.p, k0, v0,
                                          (unsigned long long *)acc->dropped.p, ctx->stream));
        HIPCHK(ctx, bcd_accum_sort(acc->sort.p, &bytes, k0, k1, v0, v1, m, end_bit, ctx->stream));
        HIPCHK(ctx, bcd_launch_splat_cells(k1, m, NE, acc->cells.p, ctx->stream));
        // staging arrays for 1.5 times the average ring of this chunk plus 8 sigma of a uniform distribution
        const double avg = (double)m * ring / (double)acc->N;
        const int cap = (int)std::min<double>(max_staged, 1.5 * avg + 8.0 * std::sqrt(avg) + 64.0);
        HIPCHK(ctx, bcd_launch_splat(acc->cells.p, v1, xy, rgb, w, acc->W, acc->H, acc->filter_f, g, (const float *)acc->table.p, cap, acc->nbins,
                                     acc->gamma, acc->maxval, (float *)acc->state.p, ctx->stream));
        // the layers on the same cells and sorted values, each with its own colours into its own nine planes
        for (int l = 0; l < acc->nlayers; ++l)
            HIPCHK(ctx, bcd_launch_splat(acc->cells.p, v1, xy, in.src[l] + 3 * b, w, acc->W, acc->H, acc->filter_f, g, (const float *)acc->table.p, cap,
                                         acc->nbins, acc->gamma, acc->maxval, (float *)acc->layers.p + (size_t)l * 9 * (size_t)acc->N, ctx->stream, true));
        // the features on the same cells and sorted values; their staging arrays are sized from the channel count (cap is cut to fit)
        if (acc->nfeat > 0)
            HIPCHK(ctx, bcd_launch_feat_splat(acc->cells.p, v1, xy, d_features + b * acc->nfeat, acc->nfeat, w, acc->W, acc->H, acc->filter_f, g,
                                              (const float *)acc->table.p, cap, (float *)acc->features.p, ctx->stream));
    }
    acc->submitted += n;
    return BCD_HIP_OK;
}

} // namespace

// separable table of a standard filter (host only); 1-D factors at d = (i + 0.5) / TS * r in double, product rounded to float once
int bcd_hip_filter_table(int kind, float radius_x, float radius_y, float param, int table_size, float *h_out)
{
    if (!h_out || table_size < 1 || table_size > 64) return BCD_HIP_EINVAL;
    if (!(radius_x > 0.f && radius_x <= 3.f) || !(radius_y > 0.f && radius_y <= 3.f)) return BCD_HIP_EINVAL;
    if (kind < BCD_HIP_FILTER_BOX || kind > BCD_HIP_FILTER_BLACKMAN_HARRIS) return BCD_HIP_EINVAL;
    if (kind == BCD_HIP_FILTER_GAUSSIAN && !(std::isfinite(param) && param >= 0.f)) return BCD_HIP_EINVAL;
    auto f1 = [&](double d, double r) -> double {
        switch (kind) {
        case BCD_HIP_FILTER_BOX: return 1.0;
        case BCD_HIP_FILTER_TENT: return std::max(0.0, 1.0 - d / r);
        case BCD_HIP_FILTER_GAUSSIAN: return std::max(0.0, std::exp(-(double)param * d * d) - std::exp(-(double)param * r * r));
        default: { // Blackman-Harris window of width 2 r centred on the sample
            const double pi = 3.14159265358979323846, u = (d + r) / (2.0 * r);
            return std::max(0.0, 0.35875 - 0.48829 * std::cos(2.0 * pi * u) + 0.14128 * std::cos(4.0 * pi * u) - 0.01168 * std::cos(6.0 * pi * u));
        }
        }
    };
    for (int iy = 0; iy < table_size; ++iy)
        for (int ix = 0; ix < table_size; ++ix) {
            const double dx = (ix + 0.5) / table_size * (double)radius_x, dy = (iy + 0.5) / table_size * (double)radius_y;
            h_out[iy * table_size + ix] = (float)(f1(dx, (double)radius_x) * f1(dy, (double)radius_y));
        }
    return BCD_HIP_OK;
}

int bcd_hip_accum_statistics(bcd_hip_accum *acc, float *d_nsamples, float *d_mean, float *d_cov, float *d_hist)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    if (!d_nsamples || !d_mean || !d_cov || !d_hist) return bad(ctx, "null output");
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_accum_snapshot((const float *)acc->state.p, acc->N, 3 * acc->nbins, d_nsamples, d_mean, d_cov, d_hist, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_accum_moments(bcd_hip_accum *acc, float *d_nsamples, float *d_mean, float *d_cov)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    if (!d_nsamples || !d_mean || !d_cov) return bad(ctx, "null output");
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_accum_moments((const float *)acc->state.p, acc->N, d_nsamples, d_mean, d_cov, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_accum_layer_statistics(bcd_hip_accum *acc, float *const *d_mean, float *const *d_cov)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    if (acc->nlayers == 0) return bad(ctx, "the accumulator has no layers (bcd_hip_accum_create_layers)");
    if (!d_mean || !d_cov) return bad(ctx, "null output list");
    BcdAccumLayerOut out;
    for (int l = 0; l < BCD_ACCUM_MAX_LAYERS; ++l) out.mean[l] = out.cov[l] = nullptr;
    for (int l = 0; l < acc->nlayers; ++l) {
        if (!d_mean[l] || !d_cov[l]) return bad(ctx, "null output");
        out.mean[l] = d_mean[l];
        out.cov[l] = d_cov[l];
    }
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_accum_snapshot_layers((const float *)acc->state.p, (const float *)acc->layers.p, acc->N, out, acc->nlayers, ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_accum_feature_statistics(bcd_hip_accum *acc, float *d_features, float *d_variances)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    if (acc->nfeat == 0) return bad(ctx, "the accumulator has no feature channels (bcd_hip_accum_create_features)");
    if (!d_features) return bad(ctx, "null output");
    const uintptr_t f = (uintptr_t)d_features, v = (uintptr_t)d_variances, bytes = (uintptr_t)acc->N * acc->nfeat * sizeof(float);
    if (d_variances && f < v + bytes && v < f + bytes) return bad(ctx, "the feature and variance outputs overlap");
    DEVICE_GUARD(ctx);
    HIPCHK(ctx, bcd_launch_feat_snapshot((const float *)acc->state.p, (const float *)acc->features.p, acc->N, acc->nfeat, d_features, d_variances,
                                         ctx->stream));
    return BCD_HIP_OK;
}

int bcd_hip_accum_info(bcd_hip_accum *acc, int64_t *samples_added, int64_t *dropped)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    DEVICE_GUARD(ctx);
    unsigned long long d = 0;
    HIPCHK(ctx, hipMemcpyAsync(&d, acc->dropped.p, sizeof(d), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (samples_added) *samples_added = acc->submitted - (int64_t)d;
    if (dropped) *dropped = (int64_t)d;
    return BCD_HIP_OK;
}

// k_plan_summary writes the summary as int64[3] then a float
static_assert(sizeof(bcd_hip_plan_summary) == 32 && offsetof(bcd_hip_plan_summary, max_error) == 24, "bcd_hip_plan_summary layout");

void bcd_hip_default_plan_params(bcd_hip_plan_params *p)
{
    if (!p) return;
    p->threshold = 0.f;
    p->eps = 1e-3f;
    p->min_samples = 2.f;
    p->max_per_pixel = 16;
}

int bcd_hip_accum_plan(bcd_hip_accum *acc, const bcd_hip_plan_params *prm, int64_t budget, uint64_t offset, float *d_error, int32_t *d_counts,
                       int32_t *d_pixels, int64_t capacity, bcd_hip_plan_summary *d_summary)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    if (!prm) return bad(ctx, "null plan parameters");
    if (!d_pixels || !d_summary) return bad(ctx, "null pixel list or summary");
    if (budget < 0 || budget > INT32_MAX) return bad(ctx, "budget must be in [0, 2^31)");
    if (capacity < budget) return bad(ctx, "pixel list capacity below the budget");
    if (!std::isfinite(prm->threshold) || prm->threshold < 0.f) return bad(ctx, "threshold must be finite and >= 0");
    if (!std::isfinite(prm->eps) || !(prm->eps > 0.f)) return bad(ctx, "eps must be finite and > 0");
    if (!std::isfinite(prm->min_samples) || prm->min_samples < 0.f) return bad(ctx, "min_samples must be finite and >= 0");
    if (prm->max_per_pixel < 1 || prm->max_per_pixel > 65535) return bad(ctx, "max_per_pixel must be in [1, 65535]");
    DEVICE_GUARD(ctx);
    RCCHK(accum_plan_scratch(acc));
    HIPCHK(ctx, hipMemsetAsync(acc->plan_red.p, 0, bcd_plan_red_bytes(), ctx->stream));
    HIPCHK(ctx, bcd_launch_accum_plan((const float *)acc->state.p, acc->N, prm->eps, prm->min_samples, prm->threshold, prm->max_per_pixel, budget,
                                      offset, d_error ? d_error : (float *)acc->plan_err.p, d_counts ? d_counts : (int32_t *)acc->plan_cnt.p,
                                      d_pixels, capacity, (int64_t *)d_summary, acc->plan_red.p, (uint64_t *)acc->plan_c.p,
                                      (int32_t *)acc->plan_ends.p, acc->plan_tmp.p, acc->plan_tmp.bytes, ctx->stream));
    return BCD_HIP_OK;
}

// ---- states: export, import, merge -----------------------------------------------------------------------------
static_assert(sizeof(bcd_hip_accum_state_header) == BCD_HIP_ACCUM_STATE_HEADER_BYTES && offsetof(bcd_hip_accum_state_header, version) == 8 &&
                  offsetof(bcd_hip_accum_state_header, header_bytes) == 12 && offsetof(bcd_hip_accum_state_header, width) == 16 &&
                  offsetof(bcd_hip_accum_state_header, height) == 20 && offsetof(bcd_hip_accum_state_header, nb_bins) == 24 &&
                  offsetof(bcd_hip_accum_state_header, gamma) == 28 && offsetof(bcd_hip_accum_state_header, max_value) == 32 &&
                  offsetof(bcd_hip_accum_state_header, nb_planes) == 36 && offsetof(bcd_hip_accum_state_header, samples_added) == 40 &&
                  offsetof(bcd_hip_accum_state_header, dropped) == 48 && offsetof(bcd_hip_accum_state_header, reserved) == 56,
              "bcd_hip_accum_state_header layout (format v1)");

namespace {

constexpr size_t STATE_CHUNK = (size_t)64 << 20; // bound of a staging / scratch chunk
const char STATE_MAGIC[8] = { 'B', 'C', 'D', 'A', 'C', 'C', 'S', 'T' };
const char LAYERS_MAGIC[8] = { 'B', 'C', 'D', 'A', 'C', 'C', 'L', 'Y' };
const char FEATURES_MAGIC[8] = { 'B', 'C', 'D', 'A', 'C', 'C', 'F', 'T' };

// what is wrong with a serialised layer block of `bytes` bytes (its header copied to *hd), or nullptr
const char *layers_problem(const void *h, int64_t bytes, bcd_hip_accum_layers_header *hd)
{
    if (!h) return "null layer block";
    if (bytes < BCD_HIP_ACCUM_LAYERS_HEADER_BYTES) return "shorter than the 64-byte header";
    memcpy(hd, h, sizeof(*hd));
    if (memcmp(hd->magic, LAYERS_MAGIC, 8) != 0) return "bad magic (not BCDACCLY)";
    if (hd->version != BCD_HIP_ACCUM_LAYERS_VERSION) return "unsupported version (not 1)";
    if (hd->header_bytes != BCD_HIP_ACCUM_LAYERS_HEADER_BYTES) return "header_bytes is not 64";
    if (hd->nb_layers < 1 || hd->nb_layers > BCD_HIP_ACCUM_MAX_LAYERS) return "nb_layers outside [1, 15]";
    if (hd->width <= 0 || hd->height <= 0 || (int64_t)hd->width * hd->height >= ((int64_t)1 << 31)) return "width and height must be positive, below 2^31 pixels";
    if (hd->nb_planes != (uint32_t)(9 * hd->nb_layers)) return "nb_planes is not 9 nb_layers";
    if (bytes != BCD_HIP_ACCUM_LAYERS_HEADER_BYTES + 4 * (int64_t)hd->nb_planes * hd->width * hd->height) return "size is not 64 + 36 nb_layers W H bytes";
    for (uint8_t r : hd->reserved)
        if (r != 0) return "reserved bytes are not zero";
    return nullptr;
}

// a well-formed layer block of this accumulator's frame size and layer count?
int accum_check_layers(bcd_hip_accum *a, const void *h, int64_t bytes)
{
    if (a->nlayers == 0) return bad(a->ctx, "the accumulator has no layers (bcd_hip_accum_create_layers)");
    bcd_hip_accum_layers_header hd;
    if (const char *why = layers_problem(h, bytes, &hd)) return bad(a->ctx, (std::string("not an accumulator layer block (version 1): ") + why).c_str());
    if (hd.width != a->W || hd.height != a->H) return bad(a->ctx, "layer block of another frame size");
    if (hd.nb_layers != a->nlayers) return bad(a->ctx, "layer block with another number of layers");
    return BCD_HIP_OK;
}

// what is wrong with a serialised feature block of `bytes` bytes (its header copied to *hd), or nullptr
const char *features_problem(const void *h, int64_t bytes, bcd_hip_accum_features_header *hd)
{
    if (!h) return "null feature block";
    if (bytes < BCD_HIP_ACCUM_FEATURES_HEADER_BYTES) return "shorter than the 64-byte header";
    memcpy(hd, h, sizeof(*hd));
    if (memcmp(hd->magic, FEATURES_MAGIC, 8) != 0) return "bad magic (not BCDACCFT)";
    if (hd->version != BCD_HIP_ACCUM_FEATURES_VERSION) return "unsupported version (not 1)";
    if (hd->header_bytes != BCD_HIP_ACCUM_FEATURES_HEADER_BYTES) return "header_bytes is not 64";
    if (hd->nb_features < 1 || hd->nb_features > BCD_HIP_ACCUM_MAX_FEATURES) return "nb_features outside [1, 8]";
    if (hd->width <= 0 || hd->height <= 0 || (int64_t)hd->width * hd->height >= ((int64_t)1 << 31)) return "width and height must be positive, below 2^31 pixels";
    if (hd->nb_planes != (uint32_t)(2 * hd->nb_features)) return "nb_planes is not 2 nb_features";
    if (bytes != BCD_HIP_ACCUM_FEATURES_HEADER_BYTES + 4 * (int64_t)hd->nb_planes * hd->width * hd->height) return "size is not 64 + 8 nb_features W H bytes";
    for (uint8_t r : hd->reserved)
        if (r != 0) return "reserved bytes are not zero";
    return nullptr;
}

// a well-formed feature block of this accumulator's frame size and channel count?
int accum_check_features(bcd_hip_accum *a, const void *h, int64_t bytes)
{
    if (a->nfeat == 0) return bad(a->ctx, "the accumulator has no feature channels (bcd_hip_accum_create_features)");
    bcd_hip_accum_features_header hd;
    if (const char *why = features_problem(h, bytes, &hd)) return bad(a->ctx, (std::string("not an accumulator feature block (version 1): ") + why).c_str());
    if (hd.width != a->W || hd.height != a->H) return bad(a->ctx, "feature block of another frame size");
    if (hd.nb_features != a->nfeat) return bad(a->ctx, "feature block with another number of channels");
    return BCD_HIP_OK;
}

// what is wrong with a serialised state of `bytes` bytes (its header copied to *hd), or nullptr
const char *state_problem(const void *h, int64_t bytes, bcd_hip_accum_state_header *hd)
{
    if (!h) return "null state";
    if (bytes < BCD_HIP_ACCUM_STATE_HEADER_BYTES) return "shorter than the 64-byte header";
    memcpy(hd, h, sizeof(*hd));
    if (memcmp(hd->magic, STATE_MAGIC, 8) != 0) return "bad magic (not BCDACCST)";
    if (hd->version != BCD_HIP_ACCUM_STATE_VERSION) return "unsupported version (not 1)";
    if (hd->header_bytes != BCD_HIP_ACCUM_STATE_HEADER_BYTES) return "header_bytes is not 64";
    if (hd->nb_bins < 2 || hd->nb_bins > 85) return "nb_bins outside [2, 85]";
    if (hd->width <= 0 || hd->height <= 0 || (int64_t)hd->width * hd->height >= ((int64_t)1 << 31)) return "width and height must be positive, below 2^31 pixels";
    if (hd->nb_planes != (uint32_t)(11 + 3 * hd->nb_bins)) return "nb_planes is not 11 + 3 nb_bins";
    if (bytes != BCD_HIP_ACCUM_STATE_HEADER_BYTES + 4 * (int64_t)hd->nb_planes * hd->width * hd->height) return "size is not 64 + 4 nb_planes W H bytes";
    for (uint8_t r : hd->reserved)
        if (r != 0) return "reserved bytes are not zero";
    if (hd->samples_added < 0 || hd->dropped < 0) return "negative counters";
    return nullptr;
}

// a well-formed state of this accumulator's geometry and parameters (gamma and max value bit for bit)?
int accum_check_state(bcd_hip_accum *a, const void *h, int64_t bytes, bcd_hip_accum_state_header *hd)
{
    if (const char *why = state_problem(h, bytes, hd)) return bad(a->ctx, (std::string("not an accumulator state (format v1): ") + why).c_str());
    if (hd->width != a->W || hd->height != a->H || hd->nb_bins != a->nbins) return bad(a->ctx, "state of another frame size or bin count");
    if (memcmp(&hd->gamma, &a->gamma, sizeof(float)) != 0 || memcmp(&hd->max_value, &a->maxval, sizeof(float)) != 0)
        return bad(a->ctx, "state with another gamma or max value");
    return BCD_HIP_OK;
}

int accum_check_pair(bcd_hip_accum *dst, bcd_hip_accum *src)
{
    if (!src) return bad(dst->ctx, "null source accumulator");
    if (dst == src) return bad(dst->ctx, "an accumulator cannot be merged into itself");
    if (dst->W != src->W || dst->H != src->H || dst->nbins != src->nbins) return bad(dst->ctx, "accumulators of different frame sizes or bin counts");
    if (dst->nlayers != src->nlayers) return bad(dst->ctx, "accumulators with different numbers of layers");
    if (dst->nfeat != src->nfeat) return bad(dst->ctx, "accumulators with different numbers of feature channels");
    if (memcmp(&dst->gamma, &src->gamma, sizeof(float)) != 0 || memcmp(&dst->maxval, &src->maxval, sizeof(float)) != 0)
        return bad(dst->ctx, "accumulators with different gamma or max value");
    return BCD_HIP_OK;
}

// the pinned staging (host_side) or the device chunks, allocated once; the context's device is current
int accum_chunks(bcd_hip_accum *a, bool host_side)
{
    bcd_hip_ctx *ctx = a->ctx;
    a->chunk_bytes = std::min(STATE_CHUNK, accum_state_bytes(a));
    for (int i = 0; i < 2; ++i) {
        if (host_side && !a->stage_ev[i]) HIPCHK(ctx, hipEventCreateWithFlags(&a->stage_ev[i], hipEventDisableTiming));
        void *&p = host_side ? a->stage[i] : a->chunk[i];
        if (p) continue;
        const hipError_t e = host_side ? hipHostMalloc(&p, a->chunk_bytes, hipHostMallocDefault) : hipMalloc(&p, a->chunk_bytes);
        if (e != hipSuccess) {
            p = nullptr;
            set_err(ctx, std::string(host_side ? "hipHostMalloc" : "hipMalloc") + " of a state chunk failed: " + hipGetErrorString(e));
            return BCD_HIP_ENOMEM;
        }
    }
    return BCD_HIP_OK;
}

// the S bytes of planes at h replace the device buffer `buf` (merge = false) or are added to it, chunk by chunk through the pinned
// staging: the host copy of chunk i + 1 runs while chunk i crosses PCIe.  Returns when h is no longer needed.
int accum_from_host(bcd_hip_accum *a, void *buf, size_t S, const uint8_t *h, bool merge)
{
    bcd_hip_ctx *ctx = a->ctx;
    RCCHK(accum_chunks(a, true));
    if (merge) RCCHK(accum_chunks(a, false));
    const size_t c = a->chunk_bytes;
    uint8_t *st = (uint8_t *)buf;
    for (size_t off = 0, i = 0; off < S; off += c, ++i) {
        const int b = (int)(i & 1);
        const size_t len = std::min(c, S - off);
        if (a->stage_busy[b]) {
            HIPCHK(ctx, hipEventSynchronize(a->stage_ev[b]));
            a->stage_busy[b] = false;
        }
        memcpy(a->stage[b], h + off, len);
        // (merge: chunk[b] was last read by the merge of chunk i - 2, earlier on the same stream)
        HIPCHK(ctx, hipMemcpyAsync(merge ? a->chunk[b] : st + off, a->stage[b], len, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipEventRecord(a->stage_ev[b], ctx->stream));
        a->stage_busy[b] = true;
        if (merge) HIPCHK(ctx, bcd_launch_accum_merge((float *)(st + off), (const float *)a->chunk[b], (int64_t)(len / 4), ctx->num_cus, ctx->stream));
    }
    return BCD_HIP_OK;
}

// the S bytes of the device buffer `buf` to `out`, chunk by chunk; the stream has been synchronised, so no staging copy is in flight
int accum_to_host(bcd_hip_accum *a, const void *buf, size_t S, uint8_t *out)
{
    bcd_hip_ctx *ctx = a->ctx;
    a->stage_busy[0] = a->stage_busy[1] = false;
    // chunk i + 2 crosses PCIe into one pinned buffer while the host copies chunk i + 1 out of the other
    const size_t c = a->chunk_bytes, nch = (S + c - 1) / c;
    const uint8_t *st = (const uint8_t *)buf;
    auto enqueue = [&](size_t i) {
        const int b = (int)(i & 1);
        hipError_t e = hipMemcpyAsync(a->stage[b], st + i * c, std::min(c, S - i * c), hipMemcpyDeviceToHost, ctx->stream);
        return e == hipSuccess ? hipEventRecord(a->stage_ev[b], ctx->stream) : e;
    };
    for (size_t i = 0; i < std::min<size_t>(2, nch); ++i) HIPCHK(ctx, enqueue(i));
    for (size_t i = 0; i < nch; ++i) {
        const int b = (int)(i & 1);
        HIPCHK(ctx, hipEventSynchronize(a->stage_ev[b]));
        memcpy(out + i * c, a->stage[b], std::min(c, S - i * c));
        if (i + 2 < nch) HIPCHK(ctx, enqueue(i + 2));
    }
    return BCD_HIP_OK;
}

} // namespace

int bcd_hip_accum_state_info(const void *h_state, int64_t bytes, bcd_hip_accum_state_header *out)
{
    bcd_hip_accum_state_header hd;
    if (state_problem(h_state, bytes, &hd)) return BCD_HIP_EINVAL;
    if (out) *out = hd;
    return BCD_HIP_OK;
}

int bcd_hip_accum_state_bytes(bcd_hip_accum *acc, int64_t *bytes)
{
    if (!acc) return BCD_HIP_EINVAL;
    if (!bytes) return bad(acc->ctx, "null size");
    *bytes = BCD_HIP_ACCUM_STATE_HEADER_BYTES + (int64_t)accum_state_bytes(acc);
    return BCD_HIP_OK;
}

int bcd_hip_accum_export(bcd_hip_accum *acc, void *h_state, int64_t capacity)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    const size_t S = accum_state_bytes(acc);
    if (!h_state) return bad(ctx, "null state buffer");
    if (capacity < BCD_HIP_ACCUM_STATE_HEADER_BYTES + (int64_t)S) return bad(ctx, "state buffer smaller than bcd_hip_accum_state_bytes");
    DEVICE_GUARD(ctx);
    RCCHK(accum_chunks(acc, true));
    int64_t added = 0, dropped = 0;
    RCCHK(bcd_hip_accum_info(acc, &added, &dropped)); // (synchronises: no staging copy is in flight after it)
    bcd_hip_accum_state_header hd;
    memset(&hd, 0, sizeof(hd));
    memcpy(hd.magic, STATE_MAGIC, 8);
    hd.version = BCD_HIP_ACCUM_STATE_VERSION;
    hd.header_bytes = BCD_HIP_ACCUM_STATE_HEADER_BYTES;
    hd.width = acc->W; hd.height = acc->H; hd.nb_bins = acc->nbins;
    hd.gamma = acc->gamma; hd.max_value = acc->maxval;
    hd.nb_planes = (uint32_t)(11 + 3 * acc->nbins);
    hd.samples_added = added; hd.dropped = dropped;
    uint8_t *out = (uint8_t *)h_state;
    memcpy(out, &hd, sizeof(hd));
    out += BCD_HIP_ACCUM_STATE_HEADER_BYTES;
    return accum_to_host(acc, acc->state.p, S, out);
}

int bcd_hip_accum_import(bcd_hip_accum *acc, const void *h_state, int64_t bytes)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    bcd_hip_accum_state_header hd;
    RCCHK(accum_check_state(acc, h_state, bytes, &hd));
    DEVICE_GUARD(ctx);
    RCCHK(accum_from_host(acc, acc->state.p, accum_state_bytes(acc), (const uint8_t *)h_state + BCD_HIP_ACCUM_STATE_HEADER_BYTES, false));
    HIPCHK(ctx, bcd_launch_accum_counter((unsigned long long *)acc->dropped.p, nullptr, (unsigned long long)hd.dropped, 0, ctx->stream));
    acc->submitted = hd.samples_added + hd.dropped;
    return BCD_HIP_OK;
}

int bcd_hip_accum_merge_state(bcd_hip_accum *acc, const void *h_state, int64_t bytes)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    bcd_hip_accum_state_header hd;
    RCCHK(accum_check_state(acc, h_state, bytes, &hd));
    DEVICE_GUARD(ctx);
    RCCHK(accum_from_host(acc, acc->state.p, accum_state_bytes(acc), (const uint8_t *)h_state + BCD_HIP_ACCUM_STATE_HEADER_BYTES, true));
    HIPCHK(ctx, bcd_launch_accum_counter((unsigned long long *)acc->dropped.p, nullptr, (unsigned long long)hd.dropped, 1, ctx->stream));
    acc->submitted += hd.samples_added + hd.dropped;
    return BCD_HIP_OK;
}

int bcd_hip_accum_merge(bcd_hip_accum *dst, bcd_hip_accum *src)
{
    if (!dst) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = dst->ctx;
    RCCHK(accum_check_pair(dst, src));
    bcd_hip_ctx *sctx = src->ctx;
    { // everything enqueued on src's stream so far ...
        DeviceGuard g(sctx);
        if (!g.ok) { set_err(ctx, "hipSetDevice failed"); return BCD_HIP_EDEVICE; }
        HIPCHK(ctx, hipEventRecord(src->ev_merge, sctx->stream));
    }
    DEVICE_GUARD(ctx);
    // ... comes before the reads on dst's stream
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, src->ev_merge, 0));
    const size_t S = accum_state_bytes(dst), SL = accum_layer_bytes(dst), SF = accum_feature_bytes(dst);
    const char *env = getenv("BCD_HIP_ACCUM_MERGE_COPY"); // 1: the chunked copy of a cross-device merge on one device too (tests)
    if (sctx->device == ctx->device && !(env && env[0] == '1')) {
        HIPCHK(ctx, bcd_launch_accum_merge((float *)dst->state.p, (const float *)src->state.p, (int64_t)(S / 4), ctx->num_cus, ctx->stream));
        if (SL) HIPCHK(ctx, bcd_launch_accum_merge((float *)dst->layers.p, (const float *)src->layers.p, (int64_t)(SL / 4), ctx->num_cus, ctx->stream));
        if (SF) HIPCHK(ctx, bcd_launch_accum_merge((float *)dst->features.p, (const float *)src->features.p, (int64_t)(SF / 4), ctx->num_cus, ctx->stream));
        HIPCHK(ctx, bcd_launch_accum_counter((unsigned long long *)dst->dropped.p, (const unsigned long long *)src->dropped.p, 0, 1, ctx->stream));
    } else {
        // src's state in chunks into dst-side scratch (peer copies; no peer access needed), each chunk merged after its copy
        RCCHK(accum_chunks(dst, false));
        const size_t c = dst->chunk_bytes;
        for (int part = 0; part < 3; ++part) { // the shared state, then the layer planes, then the feature planes
            uint8_t *st = (uint8_t *)(part == 0 ? dst->state.p : part == 1 ? dst->layers.p : dst->features.p);
            const uint8_t *ss = (const uint8_t *)(part == 0 ? src->state.p : part == 1 ? src->layers.p : src->features.p);
            const size_t bytes = part == 0 ? S : part == 1 ? SL : SF;
            for (size_t off = 0, i = 0; off < bytes; off += c, ++i) {
                void *buf = dst->chunk[i & 1];
                const size_t len = std::min(c, bytes - off);
                HIPCHK(ctx, hipMemcpyPeerAsync(buf, ctx->device, ss + off, sctx->device, len, ctx->stream));
                HIPCHK(ctx, bcd_launch_accum_merge((float *)(st + off), (const float *)buf, (int64_t)(len / 4), ctx->num_cus, ctx->stream));
            }
        }
        HIPCHK(ctx, hipMemcpyPeerAsync(dst->chunk[0], ctx->device, src->dropped.p, sctx->device, sizeof(unsigned long long), ctx->stream));
        HIPCHK(ctx, bcd_launch_accum_counter((unsigned long long *)dst->dropped.p, (const unsigned long long *)dst->chunk[0], 0, 1, ctx->stream));
    }
    // dst's reads come before whatever is enqueued on src's stream from now on
    HIPCHK(ctx, hipEventRecord(dst->ev_merge, ctx->stream));
    {
        DeviceGuard g(sctx);
        if (!g.ok) { set_err(ctx, "hipSetDevice failed"); return BCD_HIP_EDEVICE; }
        HIPCHK(ctx, hipStreamWaitEvent(sctx->stream, dst->ev_merge, 0));
    }
    dst->submitted += src->submitted;
    return BCD_HIP_OK;
}

// ---- the layer block: the layers' planes beside the v1 state ---------------------------------------------------
static_assert(sizeof(bcd_hip_accum_layers_header) == BCD_HIP_ACCUM_LAYERS_HEADER_BYTES && offsetof(bcd_hip_accum_layers_header, version) == 8 &&
                  offsetof(bcd_hip_accum_layers_header, header_bytes) == 12 && offsetof(bcd_hip_accum_layers_header, width) == 16 &&
                  offsetof(bcd_hip_accum_layers_header, height) == 20 && offsetof(bcd_hip_accum_layers_header, nb_layers) == 24 &&
                  offsetof(bcd_hip_accum_layers_header, nb_planes) == 28 && offsetof(bcd_hip_accum_layers_header, reserved) == 32,
              "bcd_hip_accum_layers_header layout (version 1)");

int bcd_hip_accum_layers_state_info(const void *h_layers, int64_t bytes, bcd_hip_accum_layers_header *out)
{
    bcd_hip_accum_layers_header hd;
    if (layers_problem(h_layers, bytes, &hd)) return BCD_HIP_EINVAL;
    if (out) *out = hd;
    return BCD_HIP_OK;
}

int bcd_hip_accum_layers_state_bytes(bcd_hip_accum *acc, int64_t *bytes)
{
    if (!acc) return BCD_HIP_EINVAL;
    if (!bytes) return bad(acc->ctx, "null size");
    if (acc->nlayers == 0) return bad(acc->ctx, "the accumulator has no layers (bcd_hip_accum_create_layers)");
    *bytes = BCD_HIP_ACCUM_LAYERS_HEADER_BYTES + (int64_t)accum_layer_bytes(acc);
    return BCD_HIP_OK;
}

int bcd_hip_accum_export_layers(bcd_hip_accum *acc, void *h_layers, int64_t capacity)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    if (acc->nlayers == 0) return bad(ctx, "the accumulator has no layers (bcd_hip_accum_create_layers)");
    const size_t S = accum_layer_bytes(acc);
    if (!h_layers) return bad(ctx, "null layer block buffer");
    if (capacity < BCD_HIP_ACCUM_LAYERS_HEADER_BYTES + (int64_t)S) return bad(ctx, "buffer smaller than bcd_hip_accum_layers_state_bytes");
    DEVICE_GUARD(ctx);
    RCCHK(accum_chunks(acc, true));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // (no staging copy is in flight after it)
    bcd_hip_accum_layers_header hd;
    memset(&hd, 0, sizeof(hd));
    memcpy(hd.magic, LAYERS_MAGIC, 8);
    hd.version = BCD_HIP_ACCUM_LAYERS_VERSION;
    hd.header_bytes = BCD_HIP_ACCUM_LAYERS_HEADER_BYTES;
    hd.width = acc->W; hd.height = acc->H; hd.nb_layers = acc->nlayers;
    hd.nb_planes = (uint32_t)(9 * acc->nlayers);
    memcpy(h_layers, &hd, sizeof(hd));
    return accum_to_host(acc, acc->layers.p, S, (uint8_t *)h_layers + BCD_HIP_ACCUM_LAYERS_HEADER_BYTES);
}

int bcd_hip_accum_import_layers(bcd_hip_accum *acc, const void *h_layers, int64_t bytes)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    RCCHK(accum_check_layers(acc, h_layers, bytes));
    DEVICE_GUARD(ctx);
    return accum_from_host(acc, acc->layers.p, accum_layer_bytes(acc), (const uint8_t *)h_layers + BCD_HIP_ACCUM_LAYERS_HEADER_BYTES, false);
}

int bcd_hip_accum_merge_layers_state(bcd_hip_accum *acc, const void *h_layers, int64_t bytes)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    RCCHK(accum_check_layers(acc, h_layers, bytes));
    DEVICE_GUARD(ctx);
    return accum_from_host(acc, acc->layers.p, accum_layer_bytes(acc), (const uint8_t *)h_layers + BCD_HIP_ACCUM_LAYERS_HEADER_BYTES, true);
}

// ---- the feature block: the feature planes beside the v1 state and the layer block -----------------------------
static_assert(sizeof(bcd_hip_accum_features_header) == BCD_HIP_ACCUM_FEATURES_HEADER_BYTES && offsetof(bcd_hip_accum_features_header, version) == 8 &&
                  offsetof(bcd_hip_accum_features_header, header_bytes) == 12 && offsetof(bcd_hip_accum_features_header, width) == 16 &&
                  offsetof(bcd_hip_accum_features_header, height) == 20 && offsetof(bcd_hip_accum_features_header, nb_features) == 24 &&
                  offsetof(bcd_hip_accum_features_header, nb_planes) == 28 && offsetof(bcd_hip_accum_features_header, reserved) == 32,
              "bcd_hip_accum_features_header layout (version 1)");

int bcd_hip_accum_features_state_info(const void *h_features, int64_t bytes, bcd_hip_accum_features_header *out)
{
    bcd_hip_accum_features_header hd;
    if (features_problem(h_features, bytes, &hd)) return BCD_HIP_EINVAL;
    if (out) *out = hd;
    return BCD_HIP_OK;
}

int bcd_hip_accum_features_state_bytes(bcd_hip_accum *acc, int64_t *bytes)
{
    if (!acc) return BCD_HIP_EINVAL;
    if (!bytes) return bad(acc->ctx, "null size");
    if (acc->nfeat == 0) return bad(acc->ctx, "the accumulator has no feature channels (bcd_hip_accum_create_features)");
    *bytes = BCD_HIP_ACCUM_FEATURES_HEADER_BYTES + (int64_t)accum_feature_bytes(acc);
    return BCD_HIP_OK;
}

int bcd_hip_accum_export_features(bcd_hip_accum *acc, void *h_features, int64_t capacity)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    if (acc->nfeat == 0) return bad(ctx, "the accumulator has no feature channels (bcd_hip_accum_create_features)");
    const size_t S = accum_feature_bytes(acc);
    if (!h_features) return bad(ctx, "null feature block buffer");
    if (capacity < BCD_HIP_ACCUM_FEATURES_HEADER_BYTES + (int64_t)S) return bad(ctx, "buffer smaller than bcd_hip_accum_features_state_bytes");
    DEVICE_GUARD(ctx);
    RCCHK(accum_chunks(acc, true));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // (no staging copy is in flight after it)
    bcd_hip_accum_features_header hd;
    memset(&hd, 0, sizeof(hd));
    memcpy(hd.magic, FEATURES_MAGIC, 8);
    hd.version = BCD_HIP_ACCUM_FEATURES_VERSION;
    hd.header_bytes = BCD_HIP_ACCUM_FEATURES_HEADER_BYTES;
    hd.width = acc->W; hd.height = acc->H; hd.nb_features = acc->nfeat;
    hd.nb_planes = (uint32_t)(2 * acc->nfeat);
    memcpy(h_features, &hd, sizeof(hd));
    return accum_to_host(acc, acc->features.p, S, (uint8_t *)h_features + BCD_HIP_ACCUM_FEATURES_HEADER_BYTES);
}

int bcd_hip_accum_import_features(bcd_hip_accum *acc, const void *h_features, int64_t bytes)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    RCCHK(accum_check_features(acc, h_features, bytes));
    DEVICE_GUARD(ctx);
    return accum_from_host(acc, acc->features.p, accum_feature_bytes(acc), (const uint8_t *)h_features + BCD_HIP_ACCUM_FEATURES_HEADER_BYTES, false);
}

int bcd_hip_accum_merge_features_state(bcd_hip_accum *acc, const void *h_features, int64_t bytes)
{
    if (!acc) return BCD_HIP_EINVAL;
    bcd_hip_ctx *ctx = acc->ctx;
    RCCHK(accum_check_features(acc, h_features, bytes));
    DEVICE_GUARD(ctx);
    return accum_from_host(acc, acc->features.p, accum_feature_bytes(acc), (const uint8_t *)h_features + BCD_HIP_ACCUM_FEATURES_HEADER_BYTES, true);
}

} // extern "C"
