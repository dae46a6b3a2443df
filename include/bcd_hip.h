/*
 * bcd_hip.h -- C ABI of the MI355X (gfx950) denoising engine: libbcd_hip.so
 *
 * This is the drop-in boundary UNDER the reference's C++ API.  The reference has no C ABI
 * (SURVEY.md 8b); the entry points below are exactly the calls that the library's own
 * bcd::Denoiser::denoise() / bcd::MultiscaleDenoiser::denoise() (bcd_amd/host/) make, i.e. what
 * replaces, in the reference:
 *     Denoiser::denoise()                 src/core/Denoiser.cpp:84-212
 *     MultiscaleDenoiser::denoise()       src/core/MultiscaleDenoiser.cpp:31-136
 *     DenoisingUnit::*                    src/core/DenoisingUnit.cpp:157-693
 *     CudaHistogramDistance (per-pixel CUDA offload, not reproduced)  src/core/CudaHistogramDistance.cu:164-239
 *
 * Conventions
 *   - every image is the reference's interleaved DeepImage layout, fp32:
 *         index = (line * W + col) * depth + d      (include/bcd/core/DeepImage.hpp:385-396)
 *     colours depth 3, nbOfSamples depth 1, histograms depth D (= 3 x bins), covariances depth 6 in
 *     the order xx,yy,zz,yz,xz,xy (include/bcd/core/CovarianceMatrix.h:18-27).
 *   - pointers named d_* are DEVICE pointers (HBM), h_* are host pointers.
 *   - every function returns 0 on success, a negative BCD_HIP_E* code otherwise, and never calls
 *     exit() (unlike HANDLE_ERROR, include/bcd/core/CudaUtils.h:18-30).
 *   - work is enqueued on the context's stream; calls that return host-visible results synchronise it.
 */
#ifndef BCD_HIP_H
#define BCD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCD_HIP_OK 0
#define BCD_HIP_EINVAL (-1)   /* null / empty / mismatched inputs (Denoiser.cpp:266-347 returns false) */
#define BCD_HIP_EDEVICE (-2)  /* HIP runtime error, message in bcd_hip_last_error()                     */
#define BCD_HIP_ENOMEM (-3)
#define BCD_HIP_EUNSUPPORTED (-4)

typedef struct bcd_hip_ctx bcd_hip_ctx;

/* IDenoiser::setProgressCallback (include/bcd/core/IDenoiser.h:91, fired from src/core/Denoiser.cpp:181-192): called from the
 * engine's host threads, serialised, with monotone values in (0, 1] -- every scale reports when its processed set is known and
 * when its estimate is complete, weighted by its share of the pixels */
typedef void (*bcd_hip_progress_fn)(float progress, void *user);

/* mirrors bcd::DenoiserParameters (include/bcd/core/IDenoiser.h:20-44) */
typedef struct bcd_hip_params {
    float    hist_dist_threshold;     /* m_histogramDistanceThreshold          default 1     */
    int32_t  patch_radius;            /* m_patchRadius                         default 1     */
    int32_t  search_radius;           /* m_searchWindowRadius                  default 6     */
    float    min_eigen_value;         /* m_minEigenValue                       default 1e-8  */
    int32_t  use_random_pixel_order;  /* m_useRandomPixelOrder                 default 1     (0 scanline, 1 seeded shuffle, 2 the reference's
                                         multi-thread -r 0 list: even strips of 2b lines, then the odd ones, Denoiser.cpp:381-414; single GPU only) */
    float    marked_skip_probability; /* m_markedPixelsSkippingProbability     default 1     */
    uint32_t order_seed;              /* seed of the visiting order; the reference seeds its
                                         shuffle from the wall clock (Denoiser.cpp:418)      */
} bcd_hip_params;

/* per-scale counters filled by the denoise calls (cf. COMPUTE_DENOISING_STATS,
 * include/bcd/core/DenoisingUnit.h:35-65) */
typedef struct bcd_hip_scale_stats {
    int32_t width, height;
    int64_t main_pixels;      /* (W-2w)(H-2w)                                    */
    int64_t processed;        /* main pixels not skipped                          */
    int64_t fallback;         /* processed through the <3P+1 similar-patch path   */
    int64_t similar_total;    /* sum of |S| over processed pixels                 */
    int32_t active_rounds;    /* fixed-point rounds of the marking strategy       */
    float   ms_similarity;    /* GPU time of the distance + mask kernels (events) */
    float   ms_active;
    float   ms_bayes;
    float   ms_total;
    int32_t similarity_path;  /* 1 = approximate planes + exact verification at the threshold, 2 = the same with the RATIO form of the distance
                               * kernel (general sample counts: any counts that are not one power of two), 0 = exact planes,
                               * 3 = planes from means and covariances (bcd_hip_denoise_moments: no histogram was read; borderline_pairs is 0) */
    int32_t borderline_pairs; /* pairs re-evaluated exactly (similarity_path >= 1)  */
    int32_t cu_share;         /* share (%) of the CU slots this scale's persistent estimate kernels took (100: all)  */
    int32_t spectral_inverses; /* full estimates (3x3 patches, default search radius) whose matrix inverse failed the sweep's checks and took
                                  the spectral branch of inverseSymmetricMatrix in the LDS kernel (normally 0)        */
} bcd_hip_scale_stats;

/* ---- context ------------------------------------------------------------------------------ */
int  bcd_hip_ctx_create(bcd_hip_ctx **ctx, int device, void *hip_stream /* hipStream_t or NULL */);
void bcd_hip_ctx_destroy(bcd_hip_ctx *ctx);
const char *bcd_hip_last_error(const bcd_hip_ctx *ctx);
int  bcd_hip_device_count(void);
void bcd_hip_default_params(bcd_hip_params *p);
/* enable per-stage event timing into the stats (adds stream synchronisations) */
int  bcd_hip_set_profiling(bcd_hip_ctx *ctx, int enabled);
/* multiscale runs drive the (independent) scales concurrently, one HIP stream + host thread each (default on; also
 * disabled by BCD_HIP_SERIAL_SCALES=1).  Results are identical either way. */
int  bcd_hip_set_concurrent_scales(bcd_hip_ctx *ctx, int enabled);
/* similar-patch selection through approximate pair-distance planes (binary16 T plane, exact bin counts) with an exact
 * re-evaluation of every pair within tau (1 +- 2^-10) (BCD_APPROX_DELTA; the approximate distance is within 5e-4 of the exact one).
 * Default on for w = 1, D in {24, 36, 60} and tau in [2^-6, 64] -- other settings take the exact kernels; also disabled by
 * BCD_HIP_EXACT_SIMILARITY=1.  The masks are bit-identical either way; 0 forces the exact kernels. */
int  bcd_hip_set_fast_similarity(bcd_hip_ctx *ctx, int enabled);
/* the approximate planes as ONE signed binary16 margin plane E = T - tau C per pixel pair (2 bytes per entry, no count plane; default) or, 0 or
 * BCD_HIP_TC_PLANES=1, as the T and C planes (3 bytes per entry) for A/B measurement.  The masks are bit-identical either way. */
int  bcd_hip_set_margin_planes(bcd_hip_ctx *ctx, int enabled);
/* process-wide: 1 = the eigensolver of the Bayesian steps (Eigen::SelfAdjointEigenSolver of DenoisingUnit.cpp:589,617) runs to off^2 <= 1e-12 diag^2
 * instead of the production rule (2e-9 + first-order correction of the positive part): ~1.5 % of a step for a 3x smaller deviation on
 * ill-conditioned low-sample frames (4K at 8 spp: 2.9e-6 instead of 9.8e-6 from the CPU path).  Default: the environment's BCD_HIP_STRICT_EIGEN (0). */
int  bcd_hip_set_strict_eigensolver(int enabled);
/* process-wide: 1 (default) = the prepare and eigensolver phases of a full estimate (patch radius 1, search radius 6) run as ONE persistent kernel,
 * k_prepare_solve27 -- a wavefront prepares two items and solves the pair --, 0 = as two kernels, one after the other.  The records they leave, and
 * therefore the results, are the same bits either way (bcd_hip_selftest_prepare_solve).  Initial value: 0 if the environment has
 * BCD_HIP_PREPARE_SOLVE_SPLIT=1. */
int  bcd_hip_set_fused_prepare_solve(int enabled);
/* share (1..100 %, default 100) of the device's CU slots the persistent estimate kernels of this context occupy.  A caller that
 * runs several contexts on one device at once lowers it for the contexts that have slack, so that the short kernels of the one on
 * the critical path find room beside them (bcd_hip_denoise does this itself for its coarse scales; the multi-GPU driver uses
 * it for its per-scale contexts).  Results do not depend on it. */
int  bcd_hip_set_cu_share(bcd_hip_ctx *ctx, int percent);
int  bcd_hip_set_progress_callback(bcd_hip_ctx *ctx, bcd_hip_progress_fn fn, void *user);
int  bcd_hip_get_stats(const bcd_hip_ctx *ctx, int scale, bcd_hip_scale_stats *out);
/* duration (ms, HIP events on the context's stream) and launch count of the pair-distance kernel
 * accumulated since the last reset -- the dominant kernel measured by bench.py's roofline */
int  bcd_hip_kernel_time(const bcd_hip_ctx *ctx, float *ms_pairdist, int32_t *launches);
int  bcd_hip_reset_kernel_time(bcd_hip_ctx *ctx);

/* ---- whole path, device-resident inputs (what bench.py times) ----------------------------------
 * replaces Denoiser::denoise() (nb_scales == 1) / MultiscaleDenoiser::denoise() (nb_scales > 1).
 * d_out: W*H*3 floats. */
int bcd_hip_denoise(bcd_hip_ctx *ctx, const float *d_colors, const float *d_nsamples,
                    const float *d_histograms, const float *d_covariances,
                    int W, int H, int D, int nb_scales, const bcd_hip_params *prm, float *d_out);

/* The same call in two halves (round 6): _begin hands the frame to a worker thread of the context and returns at once, _wait returns when the frame is
 * complete (d_out valid, every stream of the context synchronised) with the status bcd_hip_denoise would have returned.  One frame per context at a
 * time; inputs, output and the context must stay untouched until _wait.  For callers with independent frames (a sequence, AOV passes): two contexts
 * with a frame in flight each keep the chip busier than one blocking call after the other -- the results are those of the blocking call. */
int bcd_hip_denoise_begin(bcd_hip_ctx *ctx, const float *d_colors, const float *d_nsamples,
                          const float *d_histograms, const float *d_covariances,
                          int W, int H, int D, int nb_scales, const bcd_hip_params *prm, float *d_out);
int bcd_hip_denoise_wait(bcd_hip_ctx *ctx);

/* ---- several colour layers, one similar-patch selection -----------------------------------------
 * A renderer's beauty image plus its light groups / diffuse / specular / ... layers, denoised with ONE filter: the similar sets, |S|, the marking,
 * the processed / fallback lists and the count image depend only on the histograms, the sample counts and the visiting order, so they are computed
 * once per scale; only the estimate stage runs per layer.  Layer k of the result is what
 *     bcd_hip_denoise(ctx, layers[k].d_colors, d_nsamples, d_histograms, layers[k].d_covariances, ..., layers[k].d_out)
 * returns with the same parameters (same arithmetic; the float atomics of the aggregation may arrive in another order), at far less than the cost of
 * nb_layers such calls, and without a histogram image per layer.  Layer 0 goes through the code path of bcd_hip_denoise.
 *   d_colors, d_out: W*H*3 floats, d_covariances: W*H*6 floats, all device pointers; 1 <= nb_layers <= BCD_HIP_MAX_LAYERS.
 * Every argument is checked before any device work: a null pointer, a layer count out of range, an output that is (or overlaps) an input or another
 * output, or a geometry bcd_hip_denoise refuses give BCD_HIP_EINVAL / BCD_HIP_EUNSUPPORTED and a message.
 * bcd_hip_get_stats describes the shared selection; spectral_inverses is the SUM over the layers (acceptance of a sweep inverse depends on the layer's
 * matrices), bcd_hip_layer_spectral_inverses gives one layer's share.  Row bands and bcd_hip_multi_* take one layer per call. */
#define BCD_HIP_MAX_LAYERS 16
typedef struct { const float *d_colors; const float *d_covariances; float *d_out; } bcd_hip_layer;
int bcd_hip_denoise_layers(bcd_hip_ctx *ctx, const float *d_nsamples, const float *d_histograms, int W, int H, int D, int nb_scales,
                           const bcd_hip_params *prm, const bcd_hip_layer *layers, int nb_layers);
/* full estimates of `layer` at `scale` of the last bcd_hip_denoise_layers call whose sweep inverse failed its checks (see bcd_hip_scale_stats) */
int bcd_hip_layer_spectral_inverses(const bcd_hip_ctx *ctx, int scale, int layer, int32_t *count);

/* ---- a frame's selection, kept ------------------------------------------------------------------
 * What the estimate stage needs of a frame besides colours and covariances -- per scale the mask words, |S|, the pixel states, the full-estimate and
 * the fallback list with their lengths, the count image and the sample counts of that level, plus the parameters -- held in buffers of its own, so
 * that further layers of the frame (a light group a compositor asks for later; the previews of a progressive render between two refreshes of the
 * selection) cost the estimate stage alone.  A selection belongs to the context it was created on, must be destroyed before it, and is left intact
 * by every other call on that context.  Its buffers are allocated by the first _keep and only ever grow.
 *   _keep:    bcd_hip_denoise_layers (same results, same bcd_hip_get_stats / bcd_hip_layer_spectral_inverses, same refusals), after which `sel` holds
 *             the selection of every scale, replacing what it held.  A call that fails leaves `sel` invalid.
 *   _denoise: the estimate stage on the kept selection for 1 .. BCD_HIP_MAX_LAYERS layers of the kept frame size (these need not be the layers of the
 *             _keep call): no distance, mask, verification or marking kernel runs and no histogram is read.  d_nsamples NULL: the kept sample counts
 *             -- every layer is then what bcd_hip_denoise_layers returns for it on the kept frame (same arithmetic, other order of the float atomics).
 *             Other sample counts (W*H floats) replace the kept ones wherever the estimate stage reads counts (covariance / n, the sample-count
 *             pyramid and the covariance pyramid weighted by it); the selection, the lists and the count images stay the kept ones.  Reusing a
 *             selection on statistics that have moved on is an approximation the caller chooses.
 *             Afterwards bcd_hip_get_stats reports the kept processed / fallback / similar_total / similarity_path with ms_similarity = ms_active = 0
 *             and spectral_inverses summed over the layers of this call (bcd_hip_layer_spectral_inverses: one layer's share).
 *             Refused before any device work (BCD_HIP_EINVAL and a message): a null or never-filled selection, one of another device, a layer count
 *             out of range, null or overlapping images (the rules of bcd_hip_denoise_layers).
 *   _info:    host only.  _read: one scale copied out in the layouts of bcd_hip_similarity_masks / bcd_hip_active_set (d_mask: w*h*words uint32,
 *             d_nsim: w*h int32, d_state: w*h bytes, d_count: the count image, w*h int32); any pointer may be NULL; synchronises. */
typedef struct bcd_hip_selection bcd_hip_selection;
#define BCD_HIP_SELECTION_MAX_SCALES 16
typedef struct bcd_hip_selection_scale {
    int32_t width, height;
    int64_t processed;        /* as bcd_hip_scale_stats */
    int64_t fallback;
    int64_t similar_total;
    int32_t similarity_path;
    int32_t reserved;
} bcd_hip_selection_scale;
/* (a struct tag, not a typedef: the entry point that fills it has the same name) */
struct bcd_hip_selection_info {
    int32_t valid;            /* 1: a _keep call has filled the selection */
    int32_t W, H, D, nb_scales;
    bcd_hip_params params;    /* of the _keep call */
    int64_t device_bytes;     /* held by the selection */
    bcd_hip_selection_scale scale[BCD_HIP_SELECTION_MAX_SCALES];
};
int  bcd_hip_selection_create(bcd_hip_ctx *ctx, bcd_hip_selection **sel);
void bcd_hip_selection_destroy(bcd_hip_selection *sel);
int  bcd_hip_denoise_layers_keep(bcd_hip_ctx *ctx, const float *d_nsamples, const float *d_histograms, int W, int H, int D, int nb_scales,
                                 const bcd_hip_params *prm, const bcd_hip_layer *layers, int nb_layers, bcd_hip_selection *sel);
int  bcd_hip_selection_denoise(bcd_hip_selection *sel, const float *d_nsamples, const bcd_hip_layer *layers, int nb_layers);
int  bcd_hip_selection_info(const bcd_hip_selection *sel, struct bcd_hip_selection_info *out);
int  bcd_hip_selection_read(bcd_hip_selection *sel, int scale, uint32_t *d_mask, int32_t *d_nsim, uint8_t *d_state, int32_t *d_count);

/* ---- similar patches from means and covariances, without histograms ----------
 * For producers that keep a running mean and variance per pixel and no sample histogram (a film; bcd_hip_accum_moments): the selection is decided
 * from the GUIDE's colours m and the xx, yy, zz entries v of its per-pixel covariances P -- bit for bit what bcd_hip_pixel_cov returns, i.e. the
 * covariance of the pixel's mean -- in place of the chi-square histogram distance.  For pixels x and y = x + delta, channels k = 0, 1, 2 in order, from
 * s = 0.f, n = 0, in float32 without contraction:
 *     d = m_k(x) - m_k(y);   q = (v_k(x) + v_k(y)) + var_floor;   if (q > 0.f) { s = s + (d * d) / q; n = n + 1; }      (a NaN q is not counted)
 *     T_delta(x) = s, C_delta(x) = n
 * and the patch distance is that of the histogram path on these planes: the sum of T over the patch (row-major, from 0.f) divided by the float of the
 * summed counts, similar iff <= prm->hist_dist_threshold; 0 / 0 is NaN and "not similar".  Window clipping, mask bit layout and |S| are those of
 * bcd_hip_similarity_masks.  Between pixels of equal signal the distance has expectation 1; hist_dist_threshold thresholds ANOTHER quantity here than
 * in the histogram calls ("Without histograms").  var_floor (finite, >= 0; 1e-8 is a usual value) keeps pixels of zero variance
 * comparable; with 0 such a pixel is not similar to itself.
 * Everything behind the masks -- marking, lists, estimate, further layers, kept selection, pyramid, merges -- is the code of bcd_hip_denoise_layers.
 *   _similarity_masks_moments: the stage; d_colors W*H*3, d_pixel_cov W*H*6 (bcd_hip_pixel_cov), outputs as bcd_hip_similarity_masks.
 *   _window_distances_moments: the twin of bcd_hip_window_distances: (2b+1)^2 floats, +inf outside.
 *   _denoise_moments: layers[0] is the guide and is denoised like every other layer; layers 1.. follow on the one selection exactly as in
 *             bcd_hip_denoise_layers.  Level s of the guide's pyramid is what the estimate stage uses there (colours averaged, counts summed, covariances
 *             weighted by the counts, P of that level from them); no histogram level exists.  sel NULL, or a selection of this context that is
 *             filled as by bcd_hip_denoise_layers_keep and served by the unchanged bcd_hip_selection_denoise / _read / _info (which reports D = 0).
 *             bcd_hip_get_stats / bcd_hip_selection_info report similarity_path 3.
 *             Refused before any device work, with a message, the context staying usable: everything bcd_hip_denoise_layers refuses, a var_floor
 *             that is negative or not finite, a selection of another context.
 *   _denoise_moments_host: plain uploads, the resident call, downloads.  opt (may be NULL) as in bcd_hip_denoise_layers_host_ex: spike_factor > 0 runs
 *             bcd_hip_spike_filter_layers without histograms on the resident copies first (with several layers it needs filter_layers, else
 *             BCD_HIP_EUNSUPPORTED); zero_bad_values applies to every output.
 * NOT offered for this selection: row bands (bcd_hip_denoise_band[s]), bcd_hip_multi_*, and the _begin / _wait halves. */
int bcd_hip_similarity_masks_moments(bcd_hip_ctx *ctx, const float *d_colors, const float *d_pixel_cov, int W, int H, int patch_radius, int search_radius,
                                     float threshold, float var_floor, uint32_t *d_mask, int32_t *d_count);
int bcd_hip_window_distances_moments(bcd_hip_ctx *ctx, const float *d_colors, const float *d_pixel_cov, int W, int H, int patch_radius, int search_radius,
                                     float var_floor, int line, int col, float *h_out);
int bcd_hip_denoise_moments(bcd_hip_ctx *ctx, const float *d_nsamples, int W, int H, int nb_scales, const bcd_hip_params *prm, float var_floor,
                            const bcd_hip_layer *layers, int nb_layers, bcd_hip_selection *sel /* NULL, or kept as by _layers_keep */);

/* ---- the selection gated by auxiliary feature buffers ----------------------------
 * Renderers hand a denoiser noise-free or nearly noise-free buffers beside the radiance: albedo, shading normal, depth, object id.  A guide makes them
 * stop patches from being averaged across a texture or geometry edge that the radiance statistics cannot see at low sample counts.
 * A guide is: F channels, 1 <= F <= BCD_HIP_GUIDE_MAX_CHANNELS; a feature image f of W*H*F floats, pixel-interleaved like every DeepImage; an optional
 * variance image v of W*H*F floats, the variance of the pixel's feature MEAN (NULL: v == 0); per-channel floors eps_k, a HOST array of F floats, each
 * finite and >= 0; a threshold tau_g, finite and >= 0.
 * Definition (float32, no contraction, IEEE division).  For pixels x and y = x + delta, channels k = 0 .. F-1 in order, from s = 0.f, n = 0:
 *     d = f_k(x) - f_k(y)
 *     q = (v_k(x) + v_k(y)) + eps_k                                  (v absent: q = 0.f + eps_k)
 *     if (q > 0.f) { t = (d * d) / q;  if (t == t) { s = s + t; n = n + 1; } }
 *     T_delta(x) = s,  C_delta(x) = n
 * A NaN term is skipped (depth inf against depth inf on a background).  An infinite term is counted and makes the pair dissimilar (inf against a finite
 * depth).  T / C are bitwise symmetric, as for the moments.  The patch distance, the membership test (sum of T) / float(sum of C) <= tau_g, window
 * clipping, bit layout and |S| are those of bcd_hip_similarity_masks -- the same kernels produce them --; in particular 0 / 0 is NaN and "not similar".
 * The guided selection is  mask = selection mask AND feature mask, |S| = popcount.  A pure AND: no special case for the centre bit, nothing else of the
 * selection changes, and the gate follows every run and re-run of the selection pass.
 * Pyramid: level s + 1 of the features is bcd_hip_downscale_avg of level s (D = F); level s + 1 of the variances is bcd_hip_downscale_avg of level s
 * times 0.25f; tau_g and the floors are the same at every level.
 * Without variances eps_k is the squared tolerance sigma_k^2 of channel k, the distance is the mean over the patch and the counted channels of
 * (delta f / sigma_k)^2 and tau_g = 1 means "one sigma rms"; a channel with eps_k = 0 and no variance is switched off ("Auxiliary
 * features").
 *   _similarity_masks_guide: the feature masks and their counts alone, outputs as bcd_hip_similarity_masks.
 *   _window_distances_guide: the twin of bcd_hip_window_distances_moments: (2b+1)^2 floats, +inf outside.
 *   _gate_masks: d_mask[p][j] &= d_gate[p][j] for the ((2b+1)^2 + 31) / 32 words of every pixel, d_count[p] = the bits that remain.
 *   _denoise_guided: with d_histograms given, bcd_hip_denoise_layers (sel NULL) or bcd_hip_denoise_layers_keep with the gate; with d_histograms NULL
 *             (D is not looked at), bcd_hip_denoise_moments with the gate -- var_floor is read only then.  The layers follow the gated selection; a kept
 *             selection holds the gated masks and is served by the unchanged bcd_hip_selection_denoise / _read / _info, which need no features.
 *             Refused before any device work, with a message, the context staying usable: everything the underlying call refuses; F outside 1..8; a NULL
 *             guide, feature pointer or floors; a floor or threshold that is negative or not finite; no channel able to count (every floor 0 and no
 *             variances); a selection of another context.
 *   _denoise_guided_host: plain uploads of the features and variances, then the call on the resident copies by the route of
 *             bcd_hip_denoise_layers_host_ex (h_histograms given) or bcd_hip_denoise_moments_host (NULL), with their options and refusals.
 * With no guide given every other call is bit for bit what it was.  NOT offered with a guide: row bands, bcd_hip_multi_*, the _begin / _wait halves. */
#define BCD_HIP_GUIDE_MAX_CHANNELS 8
typedef struct bcd_hip_guide {
    const float *features;   /* W*H*nb_channels floats (device for the resident calls, host for _denoise_guided_host) */
    const float *variances;  /* the same size, or NULL */
    int32_t      nb_channels;
    const float *floors;     /* HOST array of nb_channels floats */
    float        threshold;
} bcd_hip_guide;
int bcd_hip_similarity_masks_guide(bcd_hip_ctx *ctx, const bcd_hip_guide *guide, int W, int H, int patch_radius, int search_radius, uint32_t *d_mask,
                                   int32_t *d_count);
int bcd_hip_window_distances_guide(bcd_hip_ctx *ctx, const bcd_hip_guide *guide, int W, int H, int patch_radius, int search_radius, int line, int col,
                                   float *h_out);
int bcd_hip_gate_masks(bcd_hip_ctx *ctx, uint32_t *d_mask, int32_t *d_count, const uint32_t *d_gate, int W, int H, int search_radius);
int bcd_hip_denoise_guided(bcd_hip_ctx *ctx, const float *d_nsamples, const float *d_histograms /* NULL: selection from means and covariances */, int W, int H,
                           int D, int nb_scales, const bcd_hip_params *prm, float var_floor, const bcd_hip_layer *layers, int nb_layers,
                           const bcd_hip_guide *guide, bcd_hip_selection *sel /* NULL, or kept as by _layers_keep */);

/* ---- similar patches from a neighbouring frame of a sequence -------------------------
 * Frames t - 1 and t + 1 of an animation show almost the same surfaces as frame t under independent noise.  The cross-frame selection finds, for every
 * main pixel p of the frame, the main pixels q of a NEIGHBOUR frame (same W, H, D) that may lend their statistics to p:
 *   - the cross set S_f(p) is the set of main pixels q of the neighbour inside the clipped window of p -- the same PixelWindow(p, radius b, border w) as in
 *     the frame itself, displacement (0, 0) included -- with d_f(p, q) <= tau;
 *   - d_f is histogramPatchDistance (DenoisingUnit.cpp:336-386) with the first patch read from the frame and the second from the neighbour, in the
 *     reference's operations: per patch offset, in row-major order, a sequential sum over the bins with b1 + b2 > 1 of
 *     (n2 b1 - n1 b2)^2 / (n1 n2 (b1 + b2)), n1 taken from the frame and n2 from the neighbour; integer bin counts; one IEEE division; no contraction;
 *   - NaN (0 / 0: no counted bin in the patch pair) is never similar;
 *   - the mask layout is that of bcd_hip_similarity_masks: bit (dl + b)(2b + 1) + (dc + b) in word bit >> 5 of the pixel's ((2b+1)^2 + 31) / 32 words;
 *   - the pair-distance planes are not symmetric between two frames, so all (2b+1)^2 displacements are evaluated.
 * A frame compared with itself gives the masks of bcd_hip_similarity_masks bit for bit.
 *   _similarity_masks_cross: d_mask_nb W*H*words uint32 and d_count_nb W*H int32 (= |S_f|) of one neighbour; pixels that are not main pixels get zeros.
 *   _window_distances_cross: the twin of bcd_hip_window_distances: the (2b+1)^2 cross distances of one main pixel, +inf outside its clipped window.
 * Both accept what their in-frame twins accept (w <= 2, b <= 15, D <= 255), refuse the rest before any device work, and synchronise.
 *
 * The estimate over the union of the sets.  Frame 0 is the frame itself, frames 1 .. F its neighbours, 1 <= F <= BCD_HIP_MAX_NEIGHBOURS; every frame
 * brings its colours, its per-pixel covariances (bcd_hip_pixel_cov of ITS covariances and sample counts) and the masks of its similar set for every pixel
 * of frame 0 (frame 0: the in-frame masks of bcd_hip_similarity_masks, frame f: bcd_hip_similarity_masks_cross).
 *   - member order: S_0 in window row-major order, then S_1 .. S_F in the order given, each in window row-major order; |S| = |S_0| + sum |S_f| is handed in
 *     as d_nsim_total (the marking kernels take masks and |S| as separate tensors: they are handed the in-frame masks and the total |S|, so a processed
 *     pixel marks its in-frame members only and other frames are never marked);
 *   - full estimate (|S| >= 3P + 1): computeNoiseCovPatchesMean, the colour mean and the empirical covariance (DenoisingUnit.cpp:400-419, 500-536) run over all
 *     members in member order, each member's per-pixel covariance coming from its own frame; Steps 1 and 2 are those of bcd_hip_bayes_accumulate; only the
 *     estimates of the members in S_0 are computed and aggregated into d_sum / d_count -- the neighbours lend statistics only;
 *   - fallback (|S| < 3P + 1): denoiseOnlyMainPatch (:455-481) with the average over the colour patches of all members, added to the main patch only.
 *   _bayes_accumulate_temporal: the twin of bcd_hip_bayes_accumulate (d_sum / d_count are accumulated into: zero them first); patch radius 1 and search
 *             radius 6 only (anything else: BCD_HIP_EUNSUPPORTED).  With nb_frames = 1 it computes what bcd_hip_bayes_accumulate computes.  Refused before any
 *             device work, with a message, the context staying usable: a null pointer, nb_frames outside 1 .. 5, an accumulator that overlaps an input or the
 *             other accumulator.  Synchronises; bcd_hip_bayes_last_redo_count reports its redo list. */
#define BCD_HIP_MAX_NEIGHBOURS 4
/* The frame call.  Inputs are the frame and nb_neighbours neighbour frames, 0 <= nb_neighbours <= BCD_HIP_MAX_NEIGHBOURS, each with colours, sample counts,
 * histograms and covariances of the same W, H, D, all device-resident (all host buffers for _host).  Per scale the steps are those above: S_0 by the code
 * of bcd_hip_denoise, one cross pass per neighbour ahead of the marking, the marking on the in-frame masks and the total |S|, the estimate over all frames.
 * Multiscale: every neighbour gets its own pyramid, built with the reducers of the frame's (colours averaged, counts and histograms summed, covariances
 * weighted by the counts); scale s uses level s of every frame; the merge, the visiting order, the per-scale seeds and the -m / -r semantics are those of
 * bcd_hip_denoise.  The scales run one after the other on the context's main workspace.  With nb_neighbours = 0 the call IS bcd_hip_denoise
 * (bcd_hip_denoise_host): it delegates.  Motion vectors arrive through bcd_hip_denoise_temporal_motion below; `reserved` must be NULL.
 * Refused before any device work, with a message, the context staying usable: with neighbours, any geometry but patch radius 1 and search radius 6
 * (BCD_HIP_EUNSUPPORTED); nb_neighbours outside 0 .. 4; a null image; a non-NULL `reserved`; an output that is or overlaps an input; what bcd_hip_denoise
 * refuses.  Kept selections, the moment selection, row bands and bcd_hip_multi_* do not combine with this call; colour layers do through
 * bcd_hip_denoise_temporal_layers below, the feature-gated selection through bcd_hip_denoise_temporal_guided further down.
 * bcd_hip_get_stats: similar_total is the sum of the total |S|, similarity_path that of the in-frame pass, ms_similarity includes the cross passes.
 *   _host: whole uploads (no streaming), the resident call, one download: the same result. */
typedef struct { const float *d_colors, *d_nsamples, *d_histograms, *d_covariances; const void *reserved; } bcd_hip_frame;
int bcd_hip_denoise_temporal(bcd_hip_ctx *ctx, const float *d_colors, const float *d_nsamples, const float *d_histograms, const float *d_covariances,
                             const bcd_hip_frame *neighbours, int nb_neighbours, int W, int H, int D, int nb_scales, const bcd_hip_params *prm, float *d_out);
int bcd_hip_denoise_temporal_host(bcd_hip_ctx *ctx, const float *h_colors, const float *h_nsamples, const float *h_histograms, const float *h_covariances,
                                  const bcd_hip_frame *neighbours /* host pointers */, int nb_neighbours, int W, int H, int D, int nb_scales,
                                  const bcd_hip_params *prm, float *h_out);
typedef struct { const float *d_colors; const float *d_pixel_cov; const uint32_t *d_mask; } bcd_hip_stage_frame;   /* [0] = the frame itself */
int bcd_hip_bayes_accumulate_temporal(bcd_hip_ctx *ctx, const bcd_hip_stage_frame *frames, int nb_frames, const int32_t *d_nsim_total, const uint8_t *d_state,
                                      int W, int H, int patch_radius, int search_radius, float min_eigen_value, float *d_sum, int32_t *d_count);
int bcd_hip_similarity_masks_cross(bcd_hip_ctx *ctx, const float *d_histograms, const float *d_nsamples, const float *d_histograms_nb,
                                   const float *d_nsamples_nb, int W, int H, int D, int patch_radius, int search_radius, float threshold,
                                   uint32_t *d_mask_nb, int32_t *d_count_nb);
int bcd_hip_window_distances_cross(bcd_hip_ctx *ctx, const float *d_histograms, const float *d_nsamples, const float *d_histograms_nb,
                                   const float *d_nsamples_nb, int W, int H, int D, int patch_radius, int search_radius, int line, int col, float *h_out);

/* ---- a sequence denoised through a sliding window that reuses cross masks ("Sequences") ----
 * Within one call the cross passes (frame -> neighbour) and (neighbour -> frame) look at different pixel pairs; between two calls they look at the SAME pairs
 * with the roles swapped, and the cross distance is bit for bit symmetric under that swap (diff changes sign exactly and is squared, n1 n2 and b1 + b2
 * commute, bins and patch offsets are summed in the same order).  So the cross masks of (B -> A) are a transposition of those of (A -> B).
 *   _transpose_masks_cross: side = 2b + 1, nbits = side^2, words = (nbits + 31) / 32, delta_k = (k / side - b, k % side - b).  For every pixel p and every
 *             k < nbits: if p + delta_k lies in the image, out(p) bit k = in(p + delta_k) bit (nbits - 1 - k); otherwise the bit is 0.  Bits >= nbits of the
 *             last word are 0.  count(p) = popcount of the output mask; d_count_out may be NULL.  No main-pixel rule is applied: real cross masks never hold
 *             a bit towards or at a pixel that is not a main pixel, so the transposed masks do not either.  d_mask_in / d_mask_out: W*H*words uint32 in the
 *             layout of bcd_hip_similarity_masks_cross.  Search radius 1 .. 6 (larger: BCD_HIP_EUNSUPPORTED -- neighbour frames exist at b = 6 only).
 *             Refused before any device work, with a message, the context staying usable: a null pointer, a non-positive size, b < 1, an output that
 *             overlaps the input or the counts.  Synchronises.
 * The sequence object keeps the last 2 radius + 1 frames resident, copies (or uploads) every frame once, builds its pyramid and per-pixel covariances once,
 * and runs the cross pass of every unordered pair of frames once: popping frame t, a neighbour f > t is searched as bcd_hip_denoise_temporal searches it and
 * the masks of every scale are kept with the pair (24 B per pixel and level); a neighbour f < t takes its masks from _transpose_masks_cross on the kept
 * masks of (f, t), and no distance plane is written.
 *   Definition.  Frame t of a sequence of T frames comes out as what bcd_hip_denoise_temporal returns for frame t with the neighbours
 *   max(0, t - radius) .. min(T - 1, t + radius) except t, in ascending frame order, with the sequence's nb_scales and params (the same order_seed for every
 *   frame).  The in-frame masks, every cross mask, |S|, the marking and the lists are bit for bit those of that call; the frame differs by the order of the
 *   float atomics only.  After a pop bcd_hip_get_stats describes that frame as after that call.  A frame without neighbours (T = 1) is bcd_hip_denoise.
 *   Protocol.  _push copies the four images (device to device; _push_host: from host memory) -- the caller's buffers are free again when it returns.  A push
 *   of frame p is refused ("pop first") while p > next_pop + radius.  _end says no further frame follows.  _ready is the number of frames that can be popped
 *   now: frame t can once frame t + radius is pushed, or after _end.  _pop writes the next frame (W*H*3 floats; _pop_host: to host memory) and its index.
 *   _set_reuse(0) searches every pair directly (for comparisons and tests; default 1).  _last_masks copies, after a pop, the masks (and their counts) of
 *   neighbour `neighbour` of the popped frame at `scale`: 0 the in-frame set, 1 .. the neighbours in ascending frame order.  _reset forgets every frame and
 *   counter and keeps the buffers.  _destroy frees them; a sequence must be destroyed before its context.
 *   Scope: histogram selection, one colour layer, patch radius 1, search radius 6, radius 1 .. 2 (2 radius <= BCD_HIP_MAX_NEIGHBOURS).  Colour layers, the
 *   feature gate and the moment selection come through bcd_hip_sequence_create_mode further down, the spike prefilter through
 *   bcd_hip_sequence_set_prefilter, per-step motion fields through bcd_hip_sequence_push_frame_motion (a warped pair is not transposed); row bands and
 *   several GPUs are out.
 *   Refused before any device work, with a message: what bcd_hip_denoise_temporal refuses; a radius outside 1 .. 2; any other geometry
 *   (BCD_HIP_EUNSUPPORTED); a null image; a push beyond the ring or after _end; a pop that is not ready.
 * A sequence handle is an opaque pointer, written by _create and passed as void *. */
int bcd_hip_transpose_masks_cross(bcd_hip_ctx *ctx, const uint32_t *d_mask_in, int W, int H, int search_radius, uint32_t *d_mask_out, int32_t *d_count_out);
/* (a struct tag, not a typedef: the entry point that fills it has the same name) */
struct bcd_hip_sequence_info {
    int64_t frames_pushed, frames_popped;
    int64_t device_bytes;       /* held by the sequence's own buffers */
    int64_t bytes_uploaded;     /* host to device, by _push_host */
    int64_t pyramids_built;     /* one per pushed frame */
    int64_t cross_computed;     /* cross passes run (all scales of a pair count as one) */
    int64_t cross_transposed;   /* cross passes replaced by a transposition */
};
int bcd_hip_sequence_create(bcd_hip_ctx *ctx, int W, int H, int D, int nb_scales, int radius, const bcd_hip_params *prm, void **out);
int bcd_hip_sequence_push(void *seq, const float *d_colors, const float *d_nsamples, const float *d_histograms, const float *d_covariances);
int bcd_hip_sequence_push_host(void *seq, const float *h_colors, const float *h_nsamples, const float *h_histograms, const float *h_covariances);
int bcd_hip_sequence_end(void *seq);
int bcd_hip_sequence_ready(void *seq);
int bcd_hip_sequence_pop(void *seq, float *d_out, int64_t *frame_index);
int bcd_hip_sequence_pop_host(void *seq, float *h_out, int64_t *frame_index);
int bcd_hip_sequence_set_reuse(void *seq, int on);
int bcd_hip_sequence_last_masks(void *seq, int neighbour, int scale, uint32_t *d_mask, int32_t *d_count);
int bcd_hip_sequence_info(void *seq, struct bcd_hip_sequence_info *info);
int bcd_hip_sequence_reset(void *seq);
void bcd_hip_sequence_destroy(void *seq);

/* ---- the colour layers of a frame denoised with its neighbour frames ("Layers") ----
 * bcd_hip_denoise_layers and bcd_hip_denoise_temporal combined.  The inputs are
 *   - the frame's sample counts and histograms;
 *   - L layers, 1 <= L <= BCD_HIP_MAX_LAYERS, each with colours, covariances and an output;
 *   - F neighbour frames, 0 <= F <= BCD_HIP_MAX_NEIGHBOURS.  Each neighbour brings its sample counts, its histograms and the same L layers (colours and
 *     covariances) in the same order.
 * Layer k of the result is what bcd_hip_denoise_temporal returns for the inputs
 *   - frame: (colours_k, nsamples, histograms, covariances_k);
 *   - neighbours: (colours_{f,k}, nsamples_f, histograms_f, covariances_{f,k}).
 * The arithmetic is the same.  Only the order of the float atomics on the sum image differs: the relation bcd_hip_denoise_layers states for its layers.
 * Per scale the in-frame set S_0, the cross sets S_1 .. S_F, the total |S|, the marking, the lists of full estimates and fallback pixels and the count
 * image are computed once; only the estimate stage runs per layer.  Every layer of every frame gets its own pyramid: colours are averaged, covariances are
 * reduced with the frame's sample counts.  bcd_hip_get_stats describes the shared selection, spectral_inverses being the sum over the layers;
 * bcd_hip_layer_spectral_inverses answers per layer after this call too.
 * Delegations: nb_neighbours == 0 IS bcd_hip_denoise_layers, nb_layers == 1 IS bcd_hip_denoise_temporal (likewise for _host).
 * Refused before any device work, with a message, the context staying usable: everything bcd_hip_denoise_temporal and bcd_hip_denoise_layers refuse; a NULL
 * layer list in a neighbour; a NULL image in any layer of any frame; a non-NULL `reserved`; an output that is, or overlaps, any input of any frame or
 * another output; with neighbours, any geometry but patch radius 1 and search radius 6 (BCD_HIP_EUNSUPPORTED).  Kept selections, the moment
 * selection, row bands and bcd_hip_multi_* do not combine with this call (the spike prefilter: bcd_hip_denoise_temporal_host_ex); motion vectors arrive through
 * bcd_hip_denoise_temporal_layers_motion below, the feature-gated selection through bcd_hip_denoise_temporal_guided.
 *   _host: every pointer is a host pointer; whole uploads (no streaming, no spike prefilter: that is bcd_hip_denoise_temporal_host_ex), the resident call, one
 *             download per layer: the same result.
 *   _bayes_accumulate_temporal_layers: the estimate stage -- the twin of bcd_hip_bayes_accumulate_temporal for nb_layers layers on ONE selection.  frames[f]
 *             holds host arrays of nb_layers device pointers (the colours and the per-pixel covariances of that frame's layers) and the frame's masks, [0]
 *             being the frame itself; d_sum is a host array of nb_layers device pointers.  It writes ONE count image, per layer one sum image (accumulated
 *             into, like the count image: zero them first) and h_redo[k], the items of layer k that took the redo list.  Patch radius 1 and search radius 6
 *             only (BCD_HIP_EUNSUPPORTED); null pointers, nb_frames outside 1 .. 5, nb_layers outside 1 .. 16, an accumulator that overlaps an input or
 *             another accumulator are refused before any device work.  Synchronises. */
typedef struct { const float *d_colors; const float *d_covariances; } bcd_hip_frame_layer;
typedef struct {
    const float *d_nsamples, *d_histograms;
    const bcd_hip_frame_layer *layers; /* nb_layers of them, in the order of the frame's layers */
    const void *reserved;              /* NULL */
} bcd_hip_frame_layers;
int bcd_hip_denoise_temporal_layers(bcd_hip_ctx *ctx, const float *d_nsamples, const float *d_histograms, const bcd_hip_frame_layers *neighbours, int nb_neighbours,
                                    int W, int H, int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer *layers, int nb_layers);
int bcd_hip_denoise_temporal_layers_host(bcd_hip_ctx *ctx, const float *h_nsamples, const float *h_histograms, const bcd_hip_frame_layers *neighbours /* host pointers */,
                                         int nb_neighbours, int W, int H, int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer *layers /* host pointers */,
                                         int nb_layers);
typedef struct { const float *const *d_colors; const float *const *d_pixel_cov; const uint32_t *d_mask; } bcd_hip_stage_frame_layers; /* [0] = the frame itself */
int bcd_hip_bayes_accumulate_temporal_layers(bcd_hip_ctx *ctx, const bcd_hip_stage_frame_layers *frames, int nb_frames, int nb_layers, const int32_t *d_nsim_total,
                                             const uint8_t *d_state, int W, int H, int patch_radius, int search_radius, float min_eigen_value, float *const *d_sum,
                                             int32_t *d_count, int32_t *h_redo);

/* ---- motion: neighbour frames reprojected by a motion field before the cross passes ("Motion") ----
 * The temporal calls above search every neighbour in the window around the SAME pixel, which is right for a locked camera only.  The motion calls take
 * one motion field per neighbour, reproject ("warp") that neighbour into the frame's pixel grid with an integer gather, and then run the calls above on the
 * warped neighbours, with one addition: an explicit validity gate on the cross masks.  `reserved` of bcd_hip_frame / bcd_hip_frame_layers keeps its
 * meaning (NULL, or refused): the fields arrive through d_motion.
 *   - Motion field of neighbour f: W*H*2 floats, interleaved (dx, dy) per pixel in the frame's pixel order.  Pixel (l, c) of the frame shows what pixel
 *     (l + ry, c + rx) of neighbour f shows, rx = rintf(dx), ry = rintf(dy), round to nearest even.  d_motion has nb_neighbours entries; a NULL entry means
 *     zero motion for that neighbour (it is neither copied nor gated).
 *   - Validity: valid_f(l, c) = 1 when dx and dy are finite, |dx|, |dy| < 2^24 and the source pixel lies inside the image, else 0.  A renderer marks a
 *     disoccluded pixel by writing NaN.
 *   - Warp: a valid pixel of the warped neighbour takes the source pixel's colours, sample count, histogram and covariance -- in the layered call the
 *     colours and covariance of every layer -- bit for bit; an invalid pixel is +0.0f in all of them.  Nothing is interpolated: sub-pixel motion is rounded.
 *   - Coarser scales: the warped neighbour's pyramid is built by the reducers of the frame's; a coarse pixel is valid when all four pixels
 *     (2l, 2l + 1) x (2c, 2c + 1) the reducers read for it are valid (a last odd line or column is read by no coarse pixel).
 *   - Gate: pvalid_f(q) = AND of valid_f(q + o) over the (2w+1)^2 patch offsets.  For every main pixel p and window displacement delta, bit delta of the
 *     cross mask of neighbour f is cleared unless pvalid_f(p + delta); |S_f| is the popcount of what remains.  The gate runs at every scale between the
 *     cross masks and the sum of the counts, so the marking and the estimate never see a member whose patch holds an invalid pixel.  (A pixel of zeros is
 *     not reliably dissimilar by itself: its distance terms are 0/0 only where the frame's pixel has a bin above 1.)
 *   - Everything else is the plain call's: member order, the 3P + 1 rule, the marking on the in-frame masks, multiscale, seeds, statistics.
 * With every field NULL the calls delegate to their plain twins.  With zero-valued fields every pixel is valid and the result is the plain call's.
 * Extra device memory per warped neighbour: (10 + D) * 4 bytes per pixel (280 at D = 60), 36 per extra layer, and 4/3 + 1 bytes of validity.
 * Refused before any device work, with a message, the context staying usable: everything the plain calls refuse; a NULL d_motion with neighbours present; an
 * output that overlaps a motion field.  Sub-pixel resampling, consistency checks, search radius 12 and the combinations the plain calls exclude stay out.
 *   _host: every pointer is a host pointer (the fields too); whole uploads, the resident call, one download.
 * Stage calls (they synchronise):
 *   _warp_frame: the four images of `frame` gathered through d_motion (NULL: zero motion) into `out`, d_valid W*H bytes.  D % 4 == 0 with 16-byte aligned
 *             histogram images moves 16 bytes per lane; anything else is served element by element.  A destination that overlaps an input, the field or
 *             another destination is refused.
 *   _warp_layers: the same for the colours and covariances of nb_layers layers (1 .. BCD_HIP_MAX_LAYERS).
 *   _valid_downscale: the validity of the (W / 2) x (H / 2) level; W, H >= 2.
 *   _gate_masks_valid: d_mask (W*H*words) and d_count (W*H) of one neighbour, as bcd_hip_similarity_masks_cross writes them, gated IN PLACE with the
 *             validity bytes d_valid of that level.  The window is clipped as there: a bit whose pixel is not a main pixel is cleared, a pixel that is not
 *             a main pixel gets empty masks and count 0.  Geometry as bcd_hip_similarity_masks_cross. */
typedef struct { float *d_colors, *d_nsamples, *d_histograms, *d_covariances; } bcd_hip_warped_frame;
typedef struct { float *d_colors; float *d_covariances; } bcd_hip_warped_layer;
int bcd_hip_denoise_temporal_motion(bcd_hip_ctx *ctx, const float *d_colors, const float *d_nsamples, const float *d_histograms, const float *d_covariances,
                                    const bcd_hip_frame *neighbours, int nb_neighbours, const float *const *d_motion /* nb_neighbours entries, each NULL or W*H*2 */,
                                    int W, int H, int D, int nb_scales, const bcd_hip_params *prm, float *d_out);
int bcd_hip_denoise_temporal_motion_host(bcd_hip_ctx *ctx, const float *h_colors, const float *h_nsamples, const float *h_histograms, const float *h_covariances,
                                         const bcd_hip_frame *neighbours /* host pointers */, int nb_neighbours, const float *const *h_motion, int W, int H, int D,
                                         int nb_scales, const bcd_hip_params *prm, float *h_out);
int bcd_hip_denoise_temporal_layers_motion(bcd_hip_ctx *ctx, const float *d_nsamples, const float *d_histograms, const bcd_hip_frame_layers *neighbours,
                                           int nb_neighbours, const float *const *d_motion, int W, int H, int D, int nb_scales, const bcd_hip_params *prm,
                                           const bcd_hip_layer *layers, int nb_layers);
int bcd_hip_denoise_temporal_layers_motion_host(bcd_hip_ctx *ctx, const float *h_nsamples, const float *h_histograms, const bcd_hip_frame_layers *neighbours,
                                                int nb_neighbours, const float *const *h_motion, int W, int H, int D, int nb_scales, const bcd_hip_params *prm,
                                                const bcd_hip_layer *layers /* host pointers */, int nb_layers);
int bcd_hip_warp_frame(bcd_hip_ctx *ctx, const bcd_hip_frame *frame, const float *d_motion, int W, int H, int D, const bcd_hip_warped_frame *out, uint8_t *d_valid);
int bcd_hip_warp_layers(bcd_hip_ctx *ctx, const bcd_hip_frame_layer *layers, int nb_layers, const float *d_motion, int W, int H, const bcd_hip_warped_layer *out,
                        uint8_t *d_valid);
int bcd_hip_valid_downscale(bcd_hip_ctx *ctx, const uint8_t *d_valid, int W, int H, uint8_t *d_out);
int bcd_hip_gate_masks_valid(bcd_hip_ctx *ctx, uint32_t *d_mask, int32_t *d_count, const uint8_t *d_valid, int W, int H, int patch_radius, int search_radius);

/* ---- features: the cross-frame selection gated by auxiliary feature buffers ("Features") ----
 * The gate of bcd_hip_denoise_guided protects the in-frame search; this one protects the cross-frame search too.  Across frames there is motion: an object
 * that moved, or a warp whose rounded or stale vectors land on another surface, and at low sample counts the histogram distance cannot tell the two surfaces
 * apart.  Inputs are those of bcd_hip_denoise_temporal_layers_motion plus a guide (bcd_hip_guide: F channels, 1 <= F <= 8, features f0, optional variances
 * v0, host floors eps_k, threshold tau_g) and, per neighbour j = 1 .. N, a feature image fj of W*H*F floats and a variance image vj exactly when the frame
 * has one.  Floors and threshold are the guide's, for every frame and every scale.  float32, no contraction, the correctly rounded division:
 * 1. Cross feature planes.  For pixel x of the frame and pixel y = x + delta of neighbour j, y inside the image, channels k = 0 .. F-1 in order, from
 *    s = 0.f, n = 0:
 *        d = f0_k(x) - fj_k(y)
 *        q = (v0_k(x) + vj_k(y)) + eps_k                             (no variances: q = 0.f + eps_k)
 *        if (q > 0.f) { t = (d * d) / q;  if (t == t) { s = s + t; n = n + 1; } }
 *        T_delta(x) = s,  C_delta(x) = n
 *    The term of bcd_hip_denoise_guided with the second operand read from the neighbour: a NaN term is skipped, an infinite term counts.  There is no
 *    symmetry between two frames, so all (2b+1)^2 displacements are evaluated; plane k = (dl + b)(2b + 1) + (dc + b) is mask bit k.
 * 2. Cross feature mask G_j(p): what bcd_hip_similarity_masks_cross makes of its planes, made of these with tau_g -- the (2w+1)^2 entries added in patch
 *    row-major order from 0.f, integer counts, one division, the test <= tau_g, NaN never similar, the clipped window, the main-pixel rule, the bit layout
 *    and empty masks off the main pixels.
 * 3. Gate.  S_0 is gated as in bcd_hip_denoise_guided (the mask ANDed with the in-frame feature mask of bcd_hip_similarity_masks_guide, |S_0| the
 *    popcount); for every neighbour, cross mask &= G_j and |S_j| is the popcount; total |S| = |S_0| + sum |S_j|.  A pure AND with no special case for
 *    delta = 0.  The gates run at every scale, ahead of the sum of the counts and the marking.
 * 4. Motion.  A neighbour with a motion field has its features and variances gathered by the same source pixel and the same validity as its other images: a
 *    valid pixel is copied bit for bit, an invalid pixel becomes +0.0f.  The gather happens at full resolution, before the pyramid is built.  The validity
 *    gate of the motion calls stays; the three ANDs commute.
 * 5. Pyramid, for every frame: features bcd_hip_downscale_avg (D = F), variances bcd_hip_downscale_avg times 0.25f; a warped neighbour's pyramid is built
 *    from the warped images.
 * 6. Everything else is the plain calls': member order, the 3P + 1 rule, marking on the (gated) in-frame masks, estimate, fallback, multiscale, seeds,
 *    layers on one selection.  bcd_hip_get_stats describes the gated selection; similar_total is the sum of the gated total |S|.
 * A neighbour whose features and variances ARE the frame's gives G_j equal, bit for bit, to the in-frame feature mask of bcd_hip_similarity_masks_guide.
 *   _denoise_temporal_guided: L = 1 .. 16 layers, d_motion NULL (nothing is warped) or nb_neighbours entries, each NULL or W*H*2 floats.  nb_neighbours == 0 IS
 *             bcd_hip_denoise_guided (histograms, sel = NULL).  Refused before any device work, with a message, the context staying usable: everything
 *             bcd_hip_denoise_temporal_layers_motion and bcd_hip_denoise_guided refuse; a NULL guide, neighbour_guides or neighbour feature pointer;
 *             variances present in some frames and not in others; d_histograms == NULL (the cross-frame moment selection is bcd_hip_denoise_temporal_moments); an output that overlaps a
 *             feature or variance image of any frame; with neighbours, any geometry but patch radius 1 and search radius 6 (BCD_HIP_EUNSUPPORTED).
 *   _denoise_temporal_guided_host: the same, every pointer a host pointer: whole uploads, the resident call, one download per layer.
 *   _similarity_masks_guide_cross: G_j and its counts alone, outputs as bcd_hip_similarity_masks_cross.
 *   _window_distances_guide_cross: the twin of bcd_hip_window_distances_cross: the (2b+1)^2 cross feature distances of one main pixel, +inf outside.
 *   _warp_features: the gather of bcd_hip_warp_layers for the feature image (and the variance image: d_variances_out is NULL exactly when in->variances is)
 *             of nb_channels floats per pixel; d_valid W*H bytes.  A destination that overlaps an input, the field or another destination is refused.
 * The stage calls accept what bcd_hip_similarity_masks_cross accepts (w <= 2, b <= 15) with F <= 8, refuse the rest before any device work, and synchronise.
 * Kept selections, the moment selection, search radius 12, row bands and bcd_hip_multi_* do not combine with these calls; the spike prefilter comes through
 * bcd_hip_denoise_temporal_host_ex (a resident caller composes bcd_hip_spike_filter_layers with the call). */
typedef struct { const float *features; const float *variances; /* NULL iff the guide's are */ } bcd_hip_guide_images;
int bcd_hip_denoise_temporal_guided(bcd_hip_ctx *ctx, const float *d_nsamples, const float *d_histograms, const bcd_hip_frame_layers *neighbours, int nb_neighbours,
                                    const float *const *d_motion /* NULL: nothing is warped; else nb_neighbours entries, each NULL or W*H*2 */, int W, int H, int D,
                                    int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer *layers, int nb_layers, const bcd_hip_guide *guide,
                                    const bcd_hip_guide_images *neighbour_guides /* nb_neighbours */);
int bcd_hip_denoise_temporal_guided_host(bcd_hip_ctx *ctx, const float *h_nsamples, const float *h_histograms, const bcd_hip_frame_layers *neighbours /* host pointers */,
                                         int nb_neighbours, const float *const *h_motion, int W, int H, int D, int nb_scales, const bcd_hip_params *prm,
                                         const bcd_hip_layer *layers /* host pointers */, int nb_layers, const bcd_hip_guide *guide /* host images */,
                                         const bcd_hip_guide_images *neighbour_guides /* host images */);
int bcd_hip_similarity_masks_guide_cross(bcd_hip_ctx *ctx, const bcd_hip_guide *guide, const bcd_hip_guide_images *neighbour, int W, int H, int patch_radius,
                                         int search_radius, uint32_t *d_mask, int32_t *d_count);
int bcd_hip_window_distances_guide_cross(bcd_hip_ctx *ctx, const bcd_hip_guide *guide, const bcd_hip_guide_images *neighbour, int W, int H, int patch_radius,
                                         int search_radius, int line, int col, float *h_out);
int bcd_hip_warp_features(bcd_hip_ctx *ctx, const bcd_hip_guide_images *in, int nb_channels, const float *d_motion, int W, int H, float *d_features_out,
                          float *d_variances_out /* NULL iff in->variances */, uint8_t *d_valid);

/* ---- moments: the cross-frame selection from means and covariances, without histograms ("Moments") ----
 * A producer without histograms (a film with a running mean and variance, bcd_hip_accum_moments) denoises single frames through bcd_hip_denoise_moments; these
 * calls let it use neighbour frames too.  Inputs are those of bcd_hip_denoise_temporal_layers_motion without any histogram image, the variance floor of
 * bcd_hip_denoise_moments and, optionally, the guide of bcd_hip_denoise_temporal_guided.  layers[0] is the guide layer of the selection and is denoised like
 * the others; every neighbour brings the same layers in the same order.  float32, no contraction, the correctly rounded division:
 * 1. Cross moment planes.  For pixel x of the frame and pixel y = x + delta of neighbour j, y inside the image, with m0, mj the colours of layer 0 of the frame
 *    and of the neighbour, v0, vj the xx, yy, zz entries of their per-pixel covariances (what bcd_hip_pixel_cov returns for that frame's covariances and its
 *    own sample counts) and eps the one var_floor of the call, channels k = 0, 1, 2 in order, from s = 0.f, n = 0:
 *        d = m0_k(x) - mj_k(y)
 *        q = (v0_k(x) + vj_k(y)) + eps
 *        if (q > 0.f) { s = s + (d * d) / q; n = n + 1; }
 *        T_delta(x) = s,  C_delta(x) = n
 *    The term of bcd_hip_similarity_masks_moments with the second operand read from the neighbour: a NaN q is not counted, a NaN or infinite term IS counted
 *    and makes the pair dissimilar (the feature term above skips a NaN term; this one does not).  There is no symmetry between two frames, so all (2b+1)^2
 *    displacements are evaluated.
 * 2. Cross mask: what bcd_hip_similarity_masks_cross makes of its planes, made of these with prm->hist_dist_threshold -- the (2w+1)^2 entries of T added in
 *    patch row-major order from 0.f, the counts summed as integers, one division, the test <= tau, NaN never similar, the clipped window, the main-pixel
 *    rule, mask bit (dl + b)(2b + 1) + (dc + b), empty masks off the main pixels.
 * 3. S_0 is the in-frame pass of bcd_hip_denoise_moments (similarity path 3).  The total |S|, the marking on the in-frame masks, member order, the 3P + 1
 *    rule, estimate, fallback, layers on one selection, seeds and merges are those of bcd_hip_denoise_temporal_layers.
 * 4. Pyramid, for every frame, that of bcd_hip_denoise_moments: colours averaged, counts summed, covariances weighted by that frame's counts; there is no
 *    histogram level.
 * 5. Motion.  A neighbour with a field has its sample counts and every layer's colours and covariances gathered as in the motion calls; nothing of a
 *    histogram is gathered.  The validity gate of the motion calls stays: a warped-out pixel has mean 0 and variance 0, which is not reliably dissimilar
 *    (against a dark, low-variance pixel of the frame the term is small, and with eps = 0 it is 0/0 only where the frame's variance is 0 too).
 * 6. Feature gate, with a guide: S_0 and every S_j are gated exactly as in bcd_hip_denoise_temporal_guided.
 * A neighbour whose colours and per-pixel covariances ARE the frame's gives the in-frame masks of bcd_hip_similarity_masks_moments, bit for bit.
 *   _denoise_temporal_moments: L = 1 .. 16 layers; neighbours[f].d_histograms is ignored and may be NULL; d_motion NULL (nothing is warped) or nb_neighbours
 *             entries, each NULL or W*H*2 floats; guide NULL (no feature gate) with neighbour_guides NULL, or both given.  nb_neighbours == 0 IS
 *             bcd_hip_denoise_moments (sel = NULL), with a guide bcd_hip_denoise_guided with NULL histograms (neighbour_guides is not looked at then).
 *             bcd_hip_get_stats reports similarity_path 3, similar_total the sum of the total |S|, ms_similarity with the cross passes; the distance kernels
 *             are timed for bcd_hip_kernel_time.  Refused before any device work, with a message, the context staying usable: everything
 *             bcd_hip_denoise_temporal_layers_motion and bcd_hip_denoise_moments refuse, histogram pointers aside; with a guide, what
 *             bcd_hip_denoise_temporal_guided refuses; guide and neighbour_guides not both NULL or both given; an output that overlaps any input; with
 *             neighbours, any geometry but patch radius 1 and search radius 6 (BCD_HIP_EUNSUPPORTED).
 *   _denoise_temporal_moments_host: the same, every pointer a host pointer: whole uploads, the resident call, one download per layer.
 *   _similarity_masks_moments_cross: the cross masks and counts of one neighbour alone, outputs as bcd_hip_similarity_masks_cross.  d_pixel_cov and
 *             d_pixel_cov_nb are per-pixel covariances (W*H*6).  form 0 is the production choice, 1 the planes (a distance kernel, then the mask kernel of
 *             bcd_hip_similarity_masks_cross), 2 one fused kernel that writes no planes and serves patch radius 1 with search radius 1 .. 6 -- elsewhere
 *             form 2 returns BCD_HIP_EUNSUPPORTED.  Every form gives the same masks and counts, bit for bit.
 *   _window_distances_moments_cross: the twin of bcd_hip_window_distances_cross: the (2b+1)^2 cross moment distances of one main pixel, +inf outside.
 * The stage calls accept what bcd_hip_similarity_masks_moments accepts (w <= 2, b <= 15, a finite var_floor >= 0), refuse the rest before any device work,
 * and synchronise.  Kept selections, row bands, bcd_hip_multi_* and any search radius other than 6 do not combine with the frame calls; the spike prefilter
 * comes through bcd_hip_denoise_temporal_host_ex (a resident caller composes bcd_hip_spike_filter_layers with the call). */
int bcd_hip_similarity_masks_moments_cross(bcd_hip_ctx *ctx, const float *d_colors, const float *d_pixel_cov, const float *d_colors_nb, const float *d_pixel_cov_nb,
                                           int W, int H, int patch_radius, int search_radius, float threshold, float var_floor, int form, uint32_t *d_mask_nb,
                                           int32_t *d_count_nb);
int bcd_hip_window_distances_moments_cross(bcd_hip_ctx *ctx, const float *d_colors, const float *d_pixel_cov, const float *d_colors_nb, const float *d_pixel_cov_nb,
                                           int W, int H, int patch_radius, int search_radius, float var_floor, int line, int col, float *h_out);
int bcd_hip_denoise_temporal_moments(bcd_hip_ctx *ctx, const float *d_nsamples, const bcd_hip_frame_layers *neighbours /* d_histograms ignored, may be NULL */,
                                     int nb_neighbours, const float *const *d_motion /* NULL: nothing is warped; else nb_neighbours entries, each NULL or W*H*2 */,
                                     int W, int H, int nb_scales, const bcd_hip_params *prm, float var_floor, const bcd_hip_layer *layers, int nb_layers,
                                     const bcd_hip_guide *guide /* NULL: no feature gate */, const bcd_hip_guide_images *neighbour_guides /* NULL iff guide is */);
int bcd_hip_denoise_temporal_moments_host(bcd_hip_ctx *ctx, const float *h_nsamples, const bcd_hip_frame_layers *neighbours /* host pointers */, int nb_neighbours,
                                          const float *const *h_motion, int W, int H, int nb_scales, const bcd_hip_params *prm, float var_floor,
                                          const bcd_hip_layer *layers /* host pointers */, int nb_layers, const bcd_hip_guide *guide /* host images */,
                                          const bcd_hip_guide_images *neighbour_guides /* host images */);

/* ---- sequences in a mode: colour layers, the moment selection, the feature gate ("Sequences", "Modes") ----
 * The cross moment term (d = m0(x) - mj(y), q = (v0(x) + vj(y)) + eps, d d / q) and the cross feature term of bcd_hip_denoise_temporal_guided have the form of the
 * histogram term: with the roles of the two frames swapped d changes sign and is squared, the one addition inside q commutes, and the pixel pairs of a patch
 * are visited in the same row-major order.  So their cross masks of (B -> A) are the transposition (bcd_hip_transpose_masks_cross) of those of (A -> B), bit
 * for bit; the transposition distributes over the AND of the gate, so the GATED masks a pop keeps for a pair are transposed as they are.
 *   Mode.  nb_layers L = 1 .. 16 colour layers; moments 0: selection from histograms, 1: from means and covariances with var_floor, layer 0 being the guide
 *   layer (no histogram is stored and D is not looked at); nb_features F = 0: no feature gate, 1 .. 8: the gate of bcd_hip_guide with feature_variances (0 / 1:
 *   every frame brings variances or none does), feature_floors (HOST array of F floats) and feature_threshold.  `reserved` must be NULL.
 *   Definition.  Frame t of T comes out, per layer, as what the matching frame call returns for frame t with the neighbours max(0, t - radius) ..
 *   min(T - 1, t + radius) except t in ascending order, no motion field, the sequence's params: bcd_hip_denoise_temporal_layers (histograms, no gate),
 *   bcd_hip_denoise_temporal_guided (histograms with the gate), bcd_hip_denoise_temporal_moments (moments, with or without the gate).  In-frame masks, cross
 *   masks, |S|, marking, lists, bcd_hip_get_stats and bcd_hip_layer_spectral_inverses are bit for bit those of that call; the layers differ by the order of
 *   float atomics only.  A frame without neighbours (T = 1) is bcd_hip_denoise_layers, bcd_hip_denoise_guided or bcd_hip_denoise_moments.
 *   A transposed neighbour runs neither a cross pass nor its cross feature pass; the in-frame set of every frame is computed and gated per pop.
 *   _create_mode: with L = 1, histograms and no gate the sequence is the one bcd_hip_sequence_create makes and takes its path; it then accepts the plain
 *             and the _frame / _layers calls alike.  Any other mode accepts only _push_frame[_host] and _pop_layers[_host], and a sequence made by
 *             bcd_hip_sequence_create only the plain calls.  _end, _ready, _set_reuse, _last_masks, _info, _reset and _destroy serve every sequence.
 *   _push_frame[_host]: one frame -- sample counts, histograms (NULL exactly in a moments sequence), L layers, features and variances as the mode says.
 *             Everything is copied or uploaded once, every pyramid level and the per-pixel covariances of all layers are built once.
 *   _pop_layers[_host]: nb_layers must be L; outs[k] takes layer k (W*H*3 floats).
 *   _mode_info: the mode, and cross_feature_passes: the cross feature passes launched (one per gated neighbour and scale) -- 0 for a transposed neighbour.
 *   Refused before any device work, with a message, the context staying usable: what the matching frame call refuses for the mode and geometry (anything but
 *   patch radius 1 and search radius 6: BCD_HIP_EUNSUPPORTED); L outside 1 .. 16, F outside 0 .. 8; a guide that cannot count; a negative or non-finite floor,
 *   threshold or var_floor; a cross feature kernel that cannot be launched; a non-NULL `reserved`; a push whose shape does not match the mode; a pop with a
 *   wrong layer count or a null output; a plain call on a sequence of another mode and the reverse.
 *   Out of scope: row bands, several GPUs.  The spike prefilter comes through bcd_hip_sequence_set_prefilter below, motion fields through
 *   bcd_hip_sequence_push_frame_motion further down (a warped pair is not symmetric and its pyramids are per pair: it is computed from both sides). */
typedef struct bcd_hip_sequence_mode {
    int32_t      nb_layers;
    int32_t      moments;
    float        var_floor;
    int32_t      nb_features;
    int32_t      feature_variances;
    const float *feature_floors;
    float        feature_threshold;
    const void  *reserved;
} bcd_hip_sequence_mode;
typedef struct bcd_hip_sequence_frame {
    const float *nsamples;
    const float *histograms;
    const bcd_hip_frame_layer *layers;
    const float *features;
    const float *variances;
    const void  *reserved;
} bcd_hip_sequence_frame;
struct bcd_hip_sequence_mode_info {
    int32_t nb_layers, moments, nb_features, feature_variances;
    int64_t cross_feature_passes;
    int64_t reserved;
};
int bcd_hip_sequence_create_mode(bcd_hip_ctx *ctx, int W, int H, int D, int nb_scales, int radius, const bcd_hip_params *prm, const bcd_hip_sequence_mode *mode,
                                 void **out);
int bcd_hip_sequence_push_frame(void *seq, const bcd_hip_sequence_frame *frame /* device images */);
int bcd_hip_sequence_push_frame_host(void *seq, const bcd_hip_sequence_frame *frame /* host images */);
int bcd_hip_sequence_pop_layers(void *seq, float *const *d_outs, int nb_layers, int64_t *frame_index);
int bcd_hip_sequence_pop_layers_host(void *seq, float *const *h_outs, int nb_layers, int64_t *frame_index);
int bcd_hip_sequence_mode_info(void *seq, struct bcd_hip_sequence_mode_info *info);

/* ---- the spike prefilter in every frame of temporal calls and sequences ("Prefilter") ----
 * Every frame is prefiltered on its own: the frame and each neighbour pass through bcd_hip_spike_filter_layers with the factor -- the sample counts, the
 * histograms (unless in moment selection) and all L layers, the decision coming from that frame's own layer-0 colours -- and the result is what the existing
 * call returns for the filtered frames; bcd_hip_get_stats reports likewise.  Feature and variance images are not moved (the precedent of
 * bcd_hip_denoise_guided_host with a factor).  Motion fields are not moved: a neighbour is filtered in its own pixel grid BEFORE it is warped.  Every layer
 * always follows the decision.  The filter runs in place (bcd_hip_spike_filter_layers_inplace) on the copies the library owns: no second set of frame
 * buffers is allocated.
 *   _denoise_temporal_host_ex: with opt == NULL or spike_factor <= 0 the call IS the existing host call that takes exactly these arguments, and delegates:
 *             h_histograms NULL: bcd_hip_denoise_temporal_moments_host; else with a guide: bcd_hip_denoise_temporal_guided_host; else with h_motion:
 *             bcd_hip_denoise_temporal_layers_motion_host; else bcd_hip_denoise_temporal_layers_host (var_floor is read in moment selection only).  With
 *             spike_factor > 0 the uploaded copies of every frame are filtered behind the uploads, then the same call runs.  nb_neighbours == 0 with a factor
 *             is the matching single-frame host call with that factor and filter_layers = 1 (bcd_hip_denoise_layers_host_ex, bcd_hip_denoise_guided_host,
 *             bcd_hip_denoise_moments_host).  Refused before any device work: what the delegated call refuses; a non-NULL `reserved`; a NaN or infinite
 *             factor; W or H < 3 with a factor.
 *   The resident frame calls take no prefilter argument -- their inputs are the caller's const buffers: a resident caller composes
 *   bcd_hip_spike_filter_layers (or _inplace, on buffers it may change) with the call.
 *   _sequence_set_prefilter: factor <= 0: off (the default).  Accepted only while the sequence holds no frame -- after its creation or _reset --, refused
 *             with a message otherwise, as are a NaN or infinite factor and a frame smaller than 3x3 with a factor.  It serves every mode.  Frame t then pops
 *             as what the frame call of its mode returns for frames that were each filtered as above: masks, |S|, marking, lists and stats are bit for bit
 *             those of that call, the frame differs by the order of the float atomics only.  Each frame is filtered once, by its push, in place in its
 *             slot, ahead of its pyramid and per-pixel covariances; device pushes and host pushes take the same path; the slot's features stay as pushed.
 *             Both directions of a pair see the same filtered frames, so the reuse counters equal those of a run without the prefilter.
 *   _sequence_prefilter_info: frames filtered and pixels moved since the creation or the last _reset (struct bcd_hip_sequence_info keeps its layout).
 * Out of scope: a temporal spike decision (outliers judged against other frames), moving feature images, row bands and several GPUs. */
typedef struct { float spike_factor; const void *reserved; /* NULL */ } bcd_hip_temporal_host_options;
int bcd_hip_denoise_temporal_host_ex(bcd_hip_ctx *ctx, const float *h_nsamples, const float *h_histograms /* NULL: moment selection */,
                                     const bcd_hip_frame_layers *neighbours, int nb_neighbours, const float *const *h_motion /* NULL or nb_neighbours entries */,
                                     int W, int H, int D, int nb_scales, const bcd_hip_params *prm, float var_floor /* moment selection only */,
                                     const bcd_hip_layer *layers, int nb_layers, const bcd_hip_guide *guide /* NULL: no gate */,
                                     const bcd_hip_guide_images *neighbour_guides, const bcd_hip_temporal_host_options *opt);
int bcd_hip_sequence_set_prefilter(void *seq, float factor);   /* <= 0: off (the default) */
int bcd_hip_sequence_prefilter_info(void *seq, int64_t *frames_filtered, int64_t *pixels_moved);

/* ---- sequences that take per-step motion fields ("Sequences with motion") ----
 * A renderer produces the vector of a pixel to the previous frame and at best to the next one; a window of radius 2 needs the fields two frames away, which are
 * compositions of the steps.
 *   _compose_motion: a is the field frame t -> frame u, b the field frame u -> frame v in frame-u pixel order, out the field t -> v; each W*H*2 floats,
 *             interleaved (dx, dy), in the convention of bcd_hip_warp_frame.  Per pixel p = (l, c): (dx1, dy1) = a(p); p is broken when dx1 or dy1 is not
 *             finite or |.| >= 2^24, or when q = (l + rintf(dy1), c + rintf(dx1)) lies outside the image; otherwise (dx2, dy2) = b(q) and p is broken when
 *             these are not finite or |.| >= 2^24; otherwise sx = rintf(dx1) + rintf(dx2), sy likewise, as int32, and p is broken when |sx| or |sy| >= 2^24.
 *             A broken pixel stores (NaN, NaN), any other ((float)sx, (float)sy).  For any images X, warp(warp(X, b), a) == warp(X, out) bit for bit, the
 *             validity of the right side being valid_a(p) AND valid_b(q(p)); whether the final source lies inside the image is the warp's own rule.
 *             Refused before any device work, the context staying usable: a null pointer, W or H <= 0, out overlapping a or b.  Synchronises.
 *   _sequence_push_frame_motion[_host]: _push_frame[_host] with the fields frame t -> t - 1 (motion_prev) and t -> t + 1 (motion_next) of the pushed frame t,
 *             W*H*2 floats each; either may be NULL: zero motion.  Accepted by every sequence of _create_mode (one of bcd_hip_sequence_create refuses it, like
 *             _push_frame); _push_frame[_host] is this call with both fields NULL.  The fields are copied into the slot (8 B per pixel each, allocated when the
 *             first field arrives) and are not touched by the spike prefilter: a frame is filtered in its own grid at its push and warped afterwards.
 *   Definition.  Frame t pops as what the matching frame call -- bcd_hip_denoise_temporal_layers_motion, bcd_hip_denoise_temporal_guided or
 *   bcd_hip_denoise_temporal_moments with d_motion -- returns for frame t with the neighbours max(0, t - radius) .. min(T - 1, t + radius) except t in ascending
 *   order, the field of neighbour t -+ 1 being the pushed step field, that of t - 2 compose(prev[t], prev[t - 1]) and that of t + 2
 *   compose(next[t], next[t + 1]); in a composition one NULL operand yields the other as it is, two yield NULL.  Masks, |S|, marking, lists,
 *   bcd_hip_get_stats and bcd_hip_layer_spectral_inverses are bit for bit those of that call; the layers differ by the order of float atomics only.
 *   A neighbour whose direction t -> f has a field is warped from its slot per pop (its pyramid and per-pixel covariances are built from the warped images, its
 *   cross masks pass the validity gate).  A pair (t, f) is kept and transposed exactly when both directions, t -> f and f -> t, are NULL: with every field NULL
 *   the sequence takes the path of _push_frame, counters included.
 *   _sequence_motion_info: neighbours warped and fields composed by the pops since the creation or the last _reset. */
int bcd_hip_compose_motion(bcd_hip_ctx *ctx, const float *d_a, const float *d_b, int W, int H, float *d_out);
int bcd_hip_sequence_push_frame_motion(void *seq, const bcd_hip_sequence_frame *frame /* device images */, const float *d_motion_prev, const float *d_motion_next);
int bcd_hip_sequence_push_frame_motion_host(void *seq, const bcd_hip_sequence_frame *frame /* host images */, const float *h_motion_prev, const float *h_motion_next);
int bcd_hip_sequence_motion_info(void *seq, int64_t *neighbours_warped, int64_t *fields_composed);

/* row-block variant for multi-GPU tiling: the images are a horizontal band of a larger frame;
 * only main pixels on local lines [main_row_begin, main_row_end) are processed, and instead of the
 * finalised colours the raw accumulators are returned (d_sum W*H*3 floats, d_count W*H int32), so
 * that neighbouring bands can exchange and add their halo lines before bcd_hip_finalize(). */
int bcd_hip_denoise_band(bcd_hip_ctx *ctx, const float *d_colors, const float *d_nsamples,
                         const float *d_histograms, const float *d_covariances,
                         int W, int H, int D, int main_row_begin, int main_row_end,
                         const bcd_hip_params *prm, uint32_t order_seed, float *d_sum, int32_t *d_count);

/* several bands at once -- the per-scale bands of one rank in the multi-GPU path -- run concurrently (job i on its own
 * stream / host thread / workspace, stats slot i), like the scales of bcd_hip_denoise() */
typedef struct bcd_hip_band_job {
    const float *d_colors, *d_nsamples, *d_histograms, *d_covariances;
    int32_t W, H, D, main_row_begin, main_row_end;
    uint32_t order_seed;
    float *d_sum;
    int32_t *d_count;
} bcd_hip_band_job;
int bcd_hip_denoise_bands(bcd_hip_ctx *ctx, const bcd_hip_band_job *jobs, int njobs, const bcd_hip_params *prm);

/* ---- one frame over several GPUs of a node (what bcd::Denoiser::setDevices / bcd_cli --devices use) ------------------
 * Row-band partition: rank r (one host thread + device devices[r]) owns a band of main pixels aligned to 2^(S-1) lines, holds
 * (b + w) halo lines of input per scale, rebuilds the pyramid for its band, and exchanges with its two neighbours only: |S| and
 * marking states of b boundary lines between marking batches (the visiting order is the whole frame's, so the result is the
 * single-GPU frame for every -m / -r setting), (b + w) accumulator halo lines, and 2 + 1 output lines for the merges.
 * Transport: RCCL point-to-point over xGMI (ncclSend / ncclRecv, one communicator per scale) when the ranks are distinct devices;
 * several ranks on ONE device (tests, debugging) exchange through device copies.  Host buffers in, host buffer out. */
typedef struct bcd_hip_multi bcd_hip_multi;
typedef struct bcd_hip_multi_stats {
    int32_t n_ranks;
    int32_t transport;          /* 1 = RCCL, 0 = in-process copies (ranks share a device) */
    int64_t frames;
    int32_t marking_rounds[8];  /* exchange + marking batches per scale of the last frame */
    float   compute_ms;         /* bcd_hip_multi_denoise_host: last frame between "every rank has its inputs" and "every rank has its band" */
} bcd_hip_multi_stats;
int  bcd_hip_multi_create(bcd_hip_multi **m, const int *devices, int n_ranks);
void bcd_hip_multi_destroy(bcd_hip_multi *m);
const char *bcd_hip_multi_last_error(const bcd_hip_multi *m);
int  bcd_hip_multi_get_stats(const bcd_hip_multi *m, bcd_hip_multi_stats *out);
/* IDenoiser::setProgressCallback for the multi-device path: every (rank, scale) reports its owned pixels when its processed set
 * is known and when its estimate is complete; calls are serialised and monotone, the last value is 1 */
int  bcd_hip_multi_set_progress_callback(bcd_hip_multi *m, bcd_hip_progress_fn fn, void *user);
int  bcd_hip_multi_set_frame_timeout(bcd_hip_multi *m, int milliseconds);
/* Failures.  A call that returns an error leaves the handle usable for the next frame: barriers, gates and the error state are
 * reset on entry.  On the RCCL transport the first failure of a frame aborts the local communicators (ncclCommAbort -- peers blocked
 * in a send / receive / all-reduce are released instead of waiting for ever), and a frame that has not finished after
 * BCD_HIP_MULTI_TIMEOUT_S seconds (default 600; 0 = never; bcd_hip_multi_set_frame_timeout sets it in milliseconds) is failed the
 * same way by the handle's watchdog thread, which is what ends a frame whose peer process died.  bcd_hip_multi_create handles rebuild their communicators on the next call; a bcd_hip_multi_create_rank handle (one process
 * per GPU) needs fresh unique ids from all processes: bcd_hip_multi_rank_renew_ids, or destroy and create it again. */
/* Communication trace of the last frame (debugging / tests): per rank, in the order the rank ENQUEUED them, four values per
 * operation: channel (scale, or nb_scales for the merges), kind (0 = neighbour exchange, 1 = all-reduce), bytes exchanged with the
 * rank above, bytes exchanged with the rank below.  All ranks must show the same (channel, kind) sequence and neighbours the same
 * sizes -- the conditions under which the RCCL transport cannot block.  get returns the number of values (4 per operation). */
int  bcd_hip_multi_set_comm_trace(bcd_hip_multi *m, int enabled);
int  bcd_hip_multi_get_comm_trace(bcd_hip_multi *m, int rank, int64_t *out, int capacity);
int  bcd_hip_multi_denoise_host(bcd_hip_multi *m, const float *h_colors, const float *h_nsamples, const float *h_histograms,
                                const float *h_covariances, int W, int H, int D, int nb_scales, const bcd_hip_params *prm, float *h_out);
/* The same partition with ONE PROCESS PER GPU (MPI-style launchers; what bench.py --gpus N uses): every process creates the handle
 * of its own rank from unique ids all processes share (rank 0 calls bcd_hip_multi_unique_id once per channel -- nb_scales + 1 of
 * them -- and distributes the bytes by whatever means the launcher offers), configures the frame, uploads the lines
 * [first_input_line, +nb_input_lines) of the four inputs once, and calls bcd_hip_multi_rank_step per frame: inputs and result of
 * the band stay in HBM.  bcd_hip_multi_rank_download copies the owned lines [first_owned_line, +nb_owned_lines) of the result. */
#define BCD_HIP_MULTI_ID_BYTES 128
int  bcd_hip_multi_unique_id(char *out /* BCD_HIP_MULTI_ID_BYTES */);
/* which RCCL library this build talks to: "rccl version <code> from <path of the shared object ncclCommInitRank resolved to>" (a process that also
 * maps a second copy -- an ML framework's bundled one -- can tell which of the two serves the band driver; BCD_HIP_MULTI_VERBOSE=1 prints the same at communicator creation) */
int  bcd_hip_multi_rccl_info(char *out, int capacity);
int  bcd_hip_multi_create_rank(bcd_hip_multi **m, int rank, int n_ranks, int device, const char *ids, int n_ids);
int  bcd_hip_multi_rank_configure(bcd_hip_multi *m, int W, int H, int D, int nb_scales, const bcd_hip_params *prm, int *first_input_line,
                                  int *nb_input_lines, int *first_owned_line, int *nb_owned_lines);
int  bcd_hip_multi_rank_upload(bcd_hip_multi *m, const float *h_colors, const float *h_nsamples, const float *h_histograms, const float *h_covariances);
int  bcd_hip_multi_rank_step(bcd_hip_multi *m);
int  bcd_hip_multi_rank_download(bcd_hip_multi *m, float *h_out_owned);
/* After a failure (or a timeout) the communicators of a one-rank handle are gone and their unique ids are consumed: instead of
 * destroying the handle, every process may hand in nb_scales + 1 FRESH ids (shared like the first set) and go on with the next frame;
 * contexts, streams and the resident band stay. */
int  bcd_hip_multi_rank_renew_ids(bcd_hip_multi *m, const char *ids, int n_ids);
/* Loopback (tests on a one-GPU box; a handle made by bcd_hip_multi_create_rank(rank 0 of 1) with ids): the rank is its own neighbour on
 * both sides, so that a frame enqueues every exchange and all-reduce of the band protocol on real RCCL communicators (ncclCommInitRank
 * with n = 1, grouped self send / recv) in the order and with the sizes a band inside a larger world would use; received data goes to
 * scratch and the result is the single-GPU frame. */
int  bcd_hip_multi_set_loopback(bcd_hip_multi *m, int enabled);
/* One device, real RCCL, through the driver's own transport code: communicators of a world of one from real unique ids, a grouped
 * self send / recv of two halo_bytes buffers and the int64 all-reduce on two channels (data checked), a simulated failure
 * (ncclCommAbort; the aborted communicators refuse further use; consumed ids cannot rebuild them), renewal from fresh ids, a second
 * exchange.  0 = all of it worked; `report` gets one line either way. */
int  bcd_hip_multi_selftest_transport(int device, long long halo_bytes, char *report, int report_capacity);

/* ---- whole path, host buffers (what bcd::Denoiser / bcd_cli call): H2D + denoise + D2H -------- */
int bcd_hip_denoise_host(bcd_hip_ctx *ctx, const float *h_colors, const float *h_nsamples,
                         const float *h_histograms, const float *h_covariances,
                         int W, int H, int D, int nb_scales, const bcd_hip_params *prm, float *h_out);
/* the same with the steps either side of the path kept on the device (one upload, one download): the spike prefilter of
 * bcd_cli -p 1 (SpikeRemovalFilter::filter, src/cli/main.cpp:428-441) on the uploaded copies -- the host images are NOT modified --
 * and the clean-up of the result (checkAndPutToZeroNegativeInfNaNValues, :389-420).  The device copies stay in the context. */
typedef struct bcd_hip_host_options {
    float   spike_factor;     /* > 0: prefilter with this standard-deviation factor (--p-factor); <= 0: off */
    int32_t zero_bad_values;  /* != 0: negative / infinite / NaN output values become 0 */
} bcd_hip_host_options;
int bcd_hip_denoise_host_ex(bcd_hip_ctx *ctx, const float *h_colors, const float *h_nsamples,
                            const float *h_histograms, const float *h_covariances,
                            int W, int H, int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_host_options *opt, float *h_out);
/* bcd_hip_denoise_layers for host images (layers[0] is the primary layer: its images and the shared inputs travel like those of
 * bcd_hip_denoise_host_ex, the other layers as plain copies).  opt->zero_bad_values applies to every output; the spike prefilter moves whole pixels
 * by the first layer's colours and is refused (BCD_HIP_EUNSUPPORTED) with more than one layer by this call (bcd_hip_denoise_layers_host_ex offers it). */
typedef struct { const float *h_colors; const float *h_covariances; float *h_out; } bcd_hip_host_layer;
int bcd_hip_denoise_layers_host(bcd_hip_ctx *ctx, const float *h_nsamples, const float *h_histograms, int W, int H, int D, int nb_scales,
                                const bcd_hip_params *prm, const bcd_hip_host_options *opt, const bcd_hip_host_layer *layers, int nb_layers);
/* The same with the spike prefilter over EVERY layer, on request.  filter_layers == 0 (or one layer, or no factor): bcd_hip_denoise_layers_host, its
 * refusal included.  filter_layers != 0 with spike_factor > 0 and several layers: the primary layer travels and is filtered as in
 * bcd_hip_denoise_host_ex; the other layers are uploaded as plain copies, and once the frame has arrived the source map of the UNFILTERED primary
 * colours (still resident) gathers their colours and covariances into a second set of device slices, which the frame reads -- no second trip over
 * the link.  The outputs are those of bcd_hip_spike_filter_layers followed by bcd_hip_denoise_layers on resident copies (same arithmetic; the float
 * atomics of the aggregation may arrive in another order); layer 0 is what bcd_hip_denoise_host_ex returns for it with the same factor. */
typedef struct { float spike_factor; int32_t zero_bad_values; int32_t filter_layers; } bcd_hip_layers_host_options;
int bcd_hip_denoise_layers_host_ex(bcd_hip_ctx *ctx, const float *h_nsamples, const float *h_histograms, int W, int H, int D, int nb_scales,
                                   const bcd_hip_params *prm, const bcd_hip_layers_host_options *opt,
                                   const bcd_hip_host_layer *layers, int nb_layers);

/* bcd_hip_denoise_moments for host images (see there) */
int bcd_hip_denoise_moments_host(bcd_hip_ctx *ctx, const float *h_nsamples, int W, int H, int nb_scales, const bcd_hip_params *prm,
                                 const bcd_hip_layers_host_options *opt, float var_floor, const bcd_hip_host_layer *layers, int nb_layers);

/* bcd_hip_denoise_guided for host images (see there): guide->features and guide->variances are HOST images */
int bcd_hip_denoise_guided_host(bcd_hip_ctx *ctx, const float *h_nsamples, const float *h_histograms /* NULL: selection from means and covariances */, int W,
                                int H, int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_layers_host_options *opt, float var_floor,
                                const bcd_hip_host_layer *layers, int nb_layers, const bcd_hip_guide *guide);

/* The histogram image of the last bcd_hip_denoise_host(_ex) call: its size, and the bytes that crossed the link.  On frames of >= 256 lines the
 * image travels without its zeros -- host threads pack every piece into one bit per value ("is not +0.0f", a test on the bit pattern: lossless)
 * plus the remaining values while the previous piece travels, a kernel rebuilds the fp32 image in HBM; an image with more than 60 % of
 * non-zero values is copied as it is.  BCD_HIP_SPARSE_UPLOAD=0 turns it off, BCD_HIP_UPLOAD_THREADS=<n> sets the packing threads (default:
 * half the host's hardware threads, at most 16). */
int bcd_hip_last_upload_bytes(const bcd_hip_ctx *ctx, int64_t *hist_bytes, int64_t *hist_bytes_sent);
/* host-side self-test of the packer (no device needed): packs the 32 values at in32 with the form this process uses -- returned: 0 scalar,
 * 2 AVX2, 5 AVX-512 (BCD_HIP_UPLOAD_SIMD=scalar|avx2|avx512 forces one the host has) -- into out64 (>= 64 values of room), sets the mask bits
 * and the number of values kept */
int bcd_hip_selftest_pack32(const uint32_t *in32, uint32_t *out64, uint32_t *bits, int *count);

/* ---- stages (device pointers) -- exposed for parity tests and multi-GPU composition ------------ */
/* The head of a scale's chain in two launches (the band driver's form of what bcd_hip_denoise does per scale): the per-pixel covariances
 * (bcd_hip_pixel_cov) with the accumulators d_sum (3 floats per pixel) / d_count cleared in the same pass, and every counter, flag and work queue
 * the following stage calls on this context start from (similarity masks, marking steps, the estimate) cleared in one launch instead of a fill each */
int bcd_hip_scale_begin(bcd_hip_ctx *ctx, const float *d_covariances, const float *d_nsamples, int W, int H, float *d_pixcov, float *d_sum, int32_t *d_count);
/* Denoiser::computePixelCovFromSampleCov   src/core/Denoiser.cpp:357-373 */
int bcd_hip_pixel_cov(bcd_hip_ctx *ctx, const float *d_cov, const float *d_nsamples, int W, int H, float *d_out);
/* DenoisingUnit::selectSimilarPatches for every main pixel   src/core/DenoisingUnit.cpp:196-219,336-386
 * d_mask: W*H*words uint32, bit (dl+b)*(2b+1)+(dc+b); d_count: W*H int32 = |S|.  words = ceil((2b+1)^2/32) */
int bcd_hip_similarity_masks(bcd_hip_ctx *ctx, const float *d_histograms, const float *d_nsamples,
                             int W, int H, int D, int patch_radius, int search_radius, float threshold,
                             uint32_t *d_mask, int32_t *d_count);
/* The same in three steps, for callers that have a host round trip of their own coming (the multi-GPU driver: its first marking
 * batch): _deferred enqueues the production kernels and copies their validity flags to the host WITHOUT waiting; after the caller's
 * next synchronisation of the context's stream, _verdict says whether the masks have to be recomputed with the exact kernels
 * (inputs outside the guarded range, borderline list overflowed) -- then call _exact. */
int bcd_hip_similarity_masks_deferred(bcd_hip_ctx *ctx, const float *d_histograms, const float *d_nsamples,
                                      int W, int H, int D, int patch_radius, int search_radius, float threshold,
                                      uint32_t *d_mask, int32_t *d_count);
int bcd_hip_similarity_masks_verdict(bcd_hip_ctx *ctx, int *redo);
int bcd_hip_similarity_masks_exact(bcd_hip_ctx *ctx, const float *d_histograms, const float *d_nsamples,
                                   int W, int H, int D, int patch_radius, int search_radius, float threshold,
                                   uint32_t *d_mask, int32_t *d_count);
/* How the last similarity pass of this context's main workspace ended (bcd_hip_similarity_masks[_deferred / _exact], or the finest scale of a frame):
 * *path = 0 exact planes, 1 approximate planes of one power-of-two sample count or of the reference's general formula, 2 approximate planes of the RATIO form;
 * *borderline = pairs that pass listed for exact re-evaluation and *capacity = the pairs its list holds (both 0 on path 0).  A pass that had to be redone
 * -- inputs outside the guarded range, list overflowed, RATIO form declined -- reports the pass that replaced it.  Read-only; waits for the context's stream. */
int bcd_hip_similarity_last_path(bcd_hip_ctx *ctx, int32_t *path, int32_t *borderline, int32_t *capacity);
/* raw patch distances of one main pixel to its window (debug / parity): (2b+1)^2 floats, +inf outside */
int bcd_hip_window_distances(bcd_hip_ctx *ctx, const float *d_histograms, const float *d_nsamples,
                             int W, int H, int D, int patch_radius, int search_radius,
                             int line, int col, float *h_out);
/* the marking strategy (DenoisingUnit.cpp:164-173,690) as a parallel fixed point.
 * d_state: W*H uint8: 0 = not a main pixel / outside band, 1 = processed, 2 = skipped. */
int bcd_hip_active_set(bcd_hip_ctx *ctx, const uint32_t *d_mask, const int32_t *d_count,
                       int W, int H, int patch_radius, int search_radius,
                       int main_row_begin, int main_row_end,
                       float skip_probability, int random_order, uint32_t seed,
                       uint8_t *d_state, int32_t *rounds);
/* the two halves of bcd_hip_active_set, for the multi-GPU band path: between two steps neighbouring bands exchange the states
 * of their boundary lines.  Only lines [main_row_begin, main_row_end) are initialised / decided; row_offset = line of the full
 * frame under local line 0 (keys and hashes are functions of the global pixel index).  bcd_hip_active_step keeps the dependency
 * lists it extracts on the first call after bcd_hip_active_init (same masks and counts until the next init); first_pass is a hint ("everything still undecided")
 * that implementations may ignore. */
int bcd_hip_active_init(bcd_hip_ctx *ctx, const int32_t *d_count, int W, int H, int patch_radius, int main_row_begin, int main_row_end,
                        float skip_probability, uint32_t seed, int row_offset, uint8_t *d_state);
int bcd_hip_active_step(bcd_hip_ctx *ctx, const uint32_t *d_mask, const int32_t *d_count, int W, int H, int patch_radius, int search_radius,
                        int main_row_begin, int main_row_end, int random_order, uint32_t seed, int row_offset, int first_pass,
                        uint8_t *d_state, int32_t *undecided);
/* bcd_hip_active_step in two halves, for a caller whose own reduction follows in stream order (the multi-GPU driver's all-reduce; round 6): _enqueue
 * launches the batch without waiting and, if d_total is not null, leaves on the DEVICE the rank's contribution to the all-reduced count of undecided
 * pixels -- the count after the batch, + 2^40 when with_verdict != 0 and the masks of the last bcd_hip_similarity_masks_deferred on this context are
 * not valid (the test bcd_hip_similarity_masks_verdict makes on the host); after the caller's synchronisation of the context's stream _collect returns
 * the local count and the number of launches the batch needed. */
int bcd_hip_active_step_enqueue(bcd_hip_ctx *ctx, const uint32_t *d_mask, const int32_t *d_count, int W, int H, int patch_radius, int search_radius,
                                int main_row_begin, int main_row_end, int random_order, uint32_t seed, int row_offset,
                                uint8_t *d_state, int64_t *d_total, int with_verdict);
int bcd_hip_active_step_collect(bcd_hip_ctx *ctx, int32_t *undecided, int32_t *launches);
/* denoiseSelectedPatches / denoiseOnlyMainPatch + aggregateOutputPatches for every processed pixel
 * (DenoisingUnit.cpp:388-481,672-693); d_sum / d_count are accumulated into (zero them first). */
int bcd_hip_bayes_accumulate(bcd_hip_ctx *ctx, const float *d_colors, const float *d_pixel_cov,
                             const uint32_t *d_mask, const int32_t *d_nsim, const uint8_t *d_state,
                             int W, int H, int patch_radius, int search_radius, float min_eigen_value,
                             float *d_sum, int32_t *d_count);
/* Items of the last bcd_hip_bayes_accumulate[_rows] call on this context (patch radius 1) that the register-resident finish kernel handed to the redo
 * list because the sweep inverse failed its checks (the spectral branch of inverseSymmetricMatrix, DenoisingUnit.cpp:578-604).  Read-only; waits for
 * the context's stream.  What bcd_hip_get_stats reports as spectral_inverses after bcd_hip_denoise, for a stage-level call. */
int bcd_hip_bayes_last_redo_count(bcd_hip_ctx *ctx, int32_t *count);
/* The estimate stage of bcd_hip_denoise_layers on a selection the caller supplies (parity tests: constructed similar sets handed to the layered kernels):
 * bcd_hip_bayes_accumulate on layers[0], then -- once its lists are on the host -- the code that serves the further layers of a scale inside
 * bcd_hip_denoise_layers (one launch of the layered tile kernel for the fallback pixels of all of them, the full-estimate chain per layer over the first
 * layer's item list), in the order a frame runs them.  Every layer brings its colours (W*H*3), per-pixel covariances (W*H*6) and a ZEROED sum image
 * (W*H*3); d_count (W*H, zeroed) is shared and written by the first layer only.  h_redo[nb_layers] (host, may be NULL) receives per layer the items that
 * took the redo list (what bcd_hip_bayes_last_redo_count reports for a single layer, and bcd_hip_layer_spectral_inverses after a frame);
 * bcd_hip_bayes_last_redo_count then returns their sum.  Synchronises the context's stream.  Checked before any device work, as bcd_hip_denoise_layers:
 * null pointers, 1 <= nb_layers <= BCD_HIP_MAX_LAYERS, a sum image that is (or overlaps) an input, the count image or another sum image, a refused geometry. */
typedef struct { const float *d_colors; const float *d_pixel_cov; float *d_sum; } bcd_hip_stage_layer;
int bcd_hip_bayes_accumulate_layers(bcd_hip_ctx *ctx, const bcd_hip_stage_layer *layers, int nb_layers,
                                    const uint32_t *d_mask, const int32_t *d_nsim, const uint8_t *d_state,
                                    int W, int H, int patch_radius, int search_radius, float min_eigen_value,
                                    int32_t *d_count, int32_t *h_redo);
/* The layer-batched streaming kernels of bcd_hip_denoise_layers, one launch for 1 <= nb_layers <= BCD_HIP_MAX_LAYERS images each (parity tests: per value
 * they are bcd_hip_pixel_cov / _finalize / _downscale_avg / _downscale_cov / _merge).  The lists are HOST arrays of nb_layers device pointers; no image of
 * a list may be null.  _pixel_cov writes layer k's per-pixel covariances to d_pixcov + k*W*H*6 and clears d_sum + k*W*H*3 (the workspace layout of a frame);
 * d_nsamples (W*H) and d_count (npix) are the shared images.  _merge: d_hi[k] (W*H*3) <- d_hi[k] - up(down(d_hi[k])) + up(d_lo[k]), d_lo[k] being (W/2)*(H/2)*3. */
int bcd_hip_layers_pixel_cov(bcd_hip_ctx *ctx, const float *const *d_cov, int nb_layers, const float *d_nsamples, int W, int H, float *d_pixcov, float *d_sum);
int bcd_hip_layers_finalize(bcd_hip_ctx *ctx, const float *const *d_sum, float *const *d_out, int nb_layers, const int32_t *d_count, int64_t npix);
int bcd_hip_layers_downscale_avg(bcd_hip_ctx *ctx, const float *const *d_in, float *const *d_out, int nb_layers, int W, int H);
int bcd_hip_layers_downscale_cov(bcd_hip_ctx *ctx, const float *const *d_cov, float *const *d_out, int nb_layers, const float *d_nsamples, int W, int H);
int bcd_hip_layers_merge(bcd_hip_ctx *ctx, float *const *d_hi, const float *const *d_lo, int nb_layers, int W, int H);
/* The same for the processed pixels of lines [row_begin, row_end) only (a row band's owned lines), optionally SPECULATIVE (round 6; patch radius 1):
 * d_skip_if points at a device word that the work already enqueued on the context's stream leaves at zero when this estimate is wanted (the band
 * driver: the all-reduced count of undecided pixels of the marking batch just enqueued), h_skip_if at the host copy of that word, copied on the same
 * stream before this call.  The call enqueues the lists and the estimate kernels -- which do nothing when the word is not zero -- waits for ONE event
 * (list lengths + the word) and reports *skipped = 1 if the word was not zero: the caller continues its marking and calls again. */
int bcd_hip_bayes_accumulate_rows(bcd_hip_ctx *ctx, const float *d_colors, const float *d_pixel_cov,
                                  const uint32_t *d_mask, const int32_t *d_nsim, const uint8_t *d_state,
                                  int W, int H, int patch_radius, int search_radius, float min_eigen_value,
                                  float *d_sum, int32_t *d_count, int row_begin, int row_end,
                                  const int64_t *d_skip_if, const int64_t *h_skip_if, int *skipped);
/* Denoiser::finalAggregation   src/core/Denoiser.cpp:458-469 */
int bcd_hip_finalize(bcd_hip_ctx *ctx, const float *d_sum, const int32_t *d_count, int64_t npix, float *d_out);
/* the same on `rows` lines of a row band (multi-GPU path), with the accumulator halos received from the neighbouring bands added
 * to the first / last `halo` lines first (nullptr pair at a frame border): one launch instead of four adds and a finalisation */
int bcd_hip_finalize_band(bcd_hip_ctx *ctx, const float *d_sum, const int32_t *d_count, int W, int rows, int halo,
                          const float *d_up_sum, const int32_t *d_up_count, const float *d_down_sum, const int32_t *d_down_count,
                          float *d_out);
/* MultiscaleDenoiser pyramid + merge   src/core/MultiscaleDenoiser.cpp:243-334,453-548 */
int bcd_hip_downscale_sum(bcd_hip_ctx *ctx, const float *d_in, int W, int H, int D, float *d_out);
int bcd_hip_downscale_avg(bcd_hip_ctx *ctx, const float *d_in, int W, int H, int D, float *d_out);
int bcd_hip_downscale_cov(bcd_hip_ctx *ctx, const float *d_cov, const float *d_nsamples, int W, int H, float *d_out);
int bcd_hip_interpolate(bcd_hip_ctx *ctx, const float *d_lo, int w, int h, int D, float *d_hi, int W, int H);
/* d_hi (W x H x D) <- d_hi - up(down(d_hi)) + up(d_lo) */
int bcd_hip_merge(bcd_hip_ctx *ctx, float *d_hi, int W, int H, const float *d_lo, int D);
/* SpikeRemovalFilter::filter   src/core/SpikeRemovalFilter.cpp:18-116 (out of place) */
int bcd_hip_spike_filter(bcd_hip_ctx *ctx, const float *d_colors, const float *d_nsamples,
                         const float *d_histograms, const float *d_covariances, int W, int H, int D, float factor,
                         float *d_colors_out, float *d_nsamples_out, float *d_histograms_out, float *d_covariances_out);
/* ---- the spike prefilter through a source map ------------------------------------------------
 * SpikeRemovalFilter::filter decides from the colours alone which neighbour replaces a pixel and then copies that neighbour's whole pixel
 * (src/core/SpikeRemovalFilter.cpp:61-72).  The decision, kept as an image, prefilters any number of further images consistently: the
 * colour layers of a frame, or the moments of a preview that reads no histogram.
 * Source map: M is an int32 image of W*H entries, W, H >= 3.  M[p] is the pixel (line * W + col) that SpikeRemovalFilter::filter with
 *   factor f copies into p, decided from the colour image given; M[p] = p where the pixel is not a spike, and where the median neighbour
 *   is the pixel itself.  It is the source index bcd_hip_spike_filter copies from, nothing else (one device function serves both).
 *   `moved` is the number of pixels with M[p] != p.
 * Apply: dst[p * depth + z] = src[M[p] * depth + z] for every p and z < depth.  A copy of bits: NaN payloads and -0 survive.  Any depth
 *   >= 1; out of place (maps have chains: a moved pixel whose source is itself moved).  An entry of M outside [0, W*H) is read as p, so a
 *   bad map cannot make the device read outside the images.
 *   _map:    d_colors W*H*3 floats, d_map W*H int32, d_moved NULL or one device int32 (zeroed by the call, then counted into).
 *   _apply:  nb_images (1..32) images of one depth in one launch; d_src / d_dst are HOST arrays of nb_images device pointers.
 *   _filter_layers: the map from layers[0].d_colors, then _apply on the sample counts, the histograms (when given: d_histograms and
 *            o_histograms are both NULL or both not; D is then not read), all colours (one launch) and all covariances (one launch),
 *            1 <= nb_layers <= BCD_HIP_MAX_LAYERS.  With histograms, the sample counts, the histograms and layer 0 have the bits of
 *            bcd_hip_spike_filter's four outputs.  d_map NULL: a scratch map of the context (grown on first use); d_moved as for _map.
 * Everything is enqueued on the context's stream; no call synchronises.  Checked before any device work (BCD_HIP_EINVAL and a message):
 * null pointers, W or H < 3, W*H >= 2^31, depth < 1, the image and layer counts, d_histograms / o_histograms null without the other, an
 * output equal to or overlapping an input, the map or another output. */
int bcd_hip_spike_map(bcd_hip_ctx *ctx, const float *d_colors, int W, int H, float factor, int32_t *d_map, int32_t *d_moved /* NULL or one device int32 */);
int bcd_hip_spike_apply(bcd_hip_ctx *ctx, const int32_t *d_map, int W, int H, int depth, const float *const *d_src, float *const *d_dst, int nb_images /* 1..32 */);
typedef struct { const float *d_colors, *d_covariances; float *d_colors_out, *d_covariances_out; } bcd_hip_spike_layer;
int bcd_hip_spike_filter_layers(bcd_hip_ctx *ctx, const float *d_nsamples, const float *d_histograms /* NULL: no histogram */, int W, int H, int D, float factor,
                                float *o_nsamples, float *o_histograms /* NULL iff d_histograms is */, const bcd_hip_spike_layer *layers, int nb_layers /* 1..16 */,
                                int32_t *d_map /* NULL: the context's scratch */, int32_t *d_moved /* NULL or device int32 */);
/* In place ("In place"): for frames that already sit in buffers of their owner -- the slot of a sequence, the uploaded copies of a host
 * call -- where a second copy of every image is the wrong price for moving a few percent of the pixels.
 * Definition: with m(p) = M[p] when 0 <= M[p] < W*H, else p (the rule of _apply), after the call every image holds at pixel p, bit for bit, the values it
 *   held BEFORE the call at pixel m(p).  Maps have chains (p <- q <- r), swaps, longer cycles and fan-out: the moved pixels (m(p) != p) are listed, their
 *   source values of every image are copied to a staging buffer of the context (grow-only), and a second kernel copies them to their destinations.  Only
 *   moved pixels are read or written; the order of the list varies from run to run and the result does not depend on it.
 *   _apply_inplace: nb_images (1..32) images, image k of depth depths[k] (1 .. 2^24; `depths` a HOST array), gathered through the map in one call.
 *   _filter_layers_inplace: the map from layers[0].d_colors (into d_map, or the context's scratch map), then one in-place gather of the sample counts, the
 *            histograms (NULL: none, D is not read) and every layer's colours and covariances.  The images end with the bits bcd_hip_spike_filter_layers
 *            writes into its separate outputs, and d_map with its map.
 *   h_moved: NULL, or one HOST int32 that receives the number of moved pixels.
 * Both calls read that number back to size the list and the staging buffer: they synchronise once; with no moved pixel nothing further is launched.
 * Checked before any device work (BCD_HIP_EINVAL and a message, the context staying usable): null pointers, W or H < 3, W*H >= 2^31, a depth < 1 (or above
 * 2^24), the image and layer counts, images that overlap each other or the map, histograms given with D < 1. */
int bcd_hip_spike_apply_inplace(bcd_hip_ctx *ctx, const int32_t *d_map, int W, int H, const int32_t *depths /* HOST array, nb_images entries, each >= 1 */,
                                float *const *d_images, int nb_images /* 1..32 */, int32_t *h_moved /* NULL or one host int32 */);
typedef struct { float *d_colors, *d_covariances; } bcd_hip_spike_layer_inplace;
int bcd_hip_spike_filter_layers_inplace(bcd_hip_ctx *ctx, float *d_nsamples, float *d_histograms /* NULL: none */, int W, int H, int D, float factor,
                                        const bcd_hip_spike_layer_inplace *layers, int nb_layers /* 1..16 */,
                                        int32_t *d_map /* NULL: the context's scratch map */, int32_t *h_moved);
/* SamplesAccumulator::addSample + getSamplesStatistics for a whole frame   src/core/SamplesAccumulator.cpp:44-141
 * (lets a GPU renderer keep the statistics in HBM).  d_samples: W*H*spp*3 floats, the spp samples of a pixel contiguous
 * and in accumulation order; d_weights: W*H*spp floats or NULL (all 1).  Outputs in DeepImage layout, hist depth 3*nb_bins.
 * nb_bins in [2, 213] (the accumulator below: [2, 85]); with 2 bins every value takes the saturation branch and lands in bins 0 and 1. */
int bcd_hip_accumulate_samples(bcd_hip_ctx *ctx, const float *d_samples, const float *d_weights, int W, int H, int spp, int nb_bins,
                               float gamma, float max_value, float *d_nsamples, float *d_mean, float *d_cov, float *d_hist);
/* Persistent device SamplesAccumulator: the running sums of SamplesAccumulator (src/core/SamplesAccumulator.cpp:44-105) kept in HBM
 * between calls, fed in batches of any pixel order and any per-pixel count, snapshotted into the four statistics images in DeepImage
 * layout (the inputs of bcd_hip_denoise) without being changed.  Each pixel accumulates its samples in stream order -- batch after
 * batch, and within a scattered batch in the order given -- with the host class's float operations, so nSamples, mean and covariance
 * are bit-identical to bcd::SamplesAccumulator fed the same stream (histograms: device powf round-off); no float atomics.
 * Work is enqueued on the context's stream; only _info synchronises it.  The context must outlive the accumulator.
 *   create: nb_bins in [2, 85]; max_batch_samples > 0 allocates the scattered-add scratch for batches of that many samples at once
 *           (larger batches are applied in chunks of that size; no add allocates), 0 grows it with the batches
 *   add_dense: rows [row_begin, row_begin + rows), spp >= 1 samples per pixel, contiguous, in accumulation order:
 *           d_samples[((line - row_begin) * W + col) * spp + i][channels], channels 3 or 4 (the 4th is ignored);
 *           d_weights [rows * W * spp] or NULL (all 1)
 *   add_scattered: n samples: d_pixel[n] = line * W + col (int32; others are skipped and counted), d_rgb[n][3], d_weights[n] or NULL
 *   statistics: d_nsamples W*H, d_mean W*H*3, d_cov W*H*6, d_hist W*H*3*nb_bins (a pixel without samples: 1/0 -> NaN / inf, as the host)
 *   info: samples accumulated and samples dropped (out-of-range indices) since create / the last reset; synchronises */
typedef struct bcd_hip_accum bcd_hip_accum;
int  bcd_hip_accum_create(bcd_hip_ctx *ctx, int W, int H, int nb_bins, float gamma, float max_value, int64_t max_batch_samples, bcd_hip_accum **acc);
void bcd_hip_accum_destroy(bcd_hip_accum *acc);
int  bcd_hip_accum_reset(bcd_hip_accum *acc);
int  bcd_hip_accum_add_dense(bcd_hip_accum *acc, const float *d_samples, const float *d_weights, int row_begin, int rows, int spp, int channels);
int  bcd_hip_accum_add_scattered(bcd_hip_accum *acc, const int32_t *d_pixel, const float *d_rgb, const float *d_weights, int64_t n);
int  bcd_hip_accum_statistics(bcd_hip_accum *acc, float *d_nsamples, float *d_mean, float *d_cov, float *d_hist);
/* the snapshot without the histograms: the three outputs have the bits of bcd_hip_accum_statistics, no bin is read or written (44 B in and 40 B out
 * per pixel instead of 564 B at 20 bins) -- what bcd_hip_selection_denoise needs of a progressive render between two refreshes of the selection */
int  bcd_hip_accum_moments(bcd_hip_accum *acc, float *d_nsamples, float *d_mean, float *d_cov);
int  bcd_hip_accum_info(bcd_hip_accum *acc, int64_t *samples_added, int64_t *dropped);
/* Splatting through a pixel reconstruction filter: samples at continuous positions go to every pixel of their
 * filter footprint, each with its own filter weight, by the rules of the accumulator: no float atomics, every pixel's contributions
 * applied by one thread in stream order, nSamples / mean / covariance bit-identical to bcd::SamplesAccumulator fed the expanded stream.
 * Definition (all arithmetic float32, no contraction, nothing but the operations written here):
 *   Geometry: pixel (col, line) covers [col, col + 1) x [line, line + 1), its centre is (col + 0.5, line + 0.5).  A sample has a position
 *     (x, y) in these units, a colour and a weight w (1 when no weights are given).
 *   Filter: an accumulator has at most one: radii rx, ry in (0, 3], a table size TS in [1, 64], a table T[TS][TS] of finite, non-negative
 *     floats (row = y index); inv_rx = 1.f / rx, inv_ry = 1.f / ry, Kx = (int)ceilf(rx + 0.5f), Ky likewise (at most 4).
 *   Footprint: c0 = (int)floorf(x), l0 = (int)floorf(y); candidates col = c0 - Kx .. c0 + Kx, line = l0 - Ky .. l0 + Ky.  With
 *     dx = fabsf(((float)col + 0.5f) - x), dy likewise, a candidate belongs to the footprint iff dx < rx && dy < ry, it lies in the frame,
 *     and f = T[iy * TS + ix] != 0 with ix = min((int)(dx * inv_rx * (float)TS), TS - 1) (product evaluated left to right), iy likewise.
 *     Its contribution is addSample(line, col, r, g, b, w * f): one float multiplication for the weight.
 *   Order: a pixel receives its contributions in stream order of the samples (batch after batch, inside a batch in the order given; a
 *     sample contributes to a pixel at most once).  The host restatement: for each sample in order, for line ascending, for col
 *     ascending, addSample.
 *   Counters: a sample whose position is not finite, which lies outside [-Kx, W + Kx) x [-Ky, H + Ky), or whose footprint is empty
 *     contributes nothing and counts as dropped; every other sample adds 1 to samples_added (samples, not contributions).  A sample
 *     just outside the frame whose footprint reaches into it does contribute.
 *   set_filter: copies the table (h_table[table_size * table_size], host memory); ordered on the stream after the adds already enqueued.
 *           h_table == NULL removes the filter.  EINVAL, the previous filter kept, for radii outside (0, 3], a table size outside [1, 64]
 *           and negative, NaN or infinite entries.  Filters with negative lobes (Mitchell, Lanczos) are refused on purpose: negative weights
 *           give negative histogram bins, which the similarity kernels' guards send to the slow exact path.  The filter is not part of a
 *           serialised state: a resumed render sets its filter again.
 *   add_splatted: d_xy[n][2] (x, y), d_rgb[n][3], d_weights[n] or NULL.  EINVAL without a filter, for null pointers or n < 0; n == 0 is a
 *           no-op.  Batches above max_batch_samples are applied in chunks in order (a denser chunk than the kernel's staging holds is split
 *           further; no bit depends on it).  Enqueued on the context's stream, no synchronisation.  The running sums, the state format,
 *           export / import / merge, plan and the snapshot are those of the other adds: a splat is another way of adding to the same sums.
 *   filter_table: host only, no device: the separable table of a standard filter into h_out[table_size * table_size]; the 1-D factors
 *           are evaluated at d = (i + 0.5) / table_size * radius in double, multiplied in double and rounded to float once.  BOX: 1;
 *           TENT: 1 - d / r; GAUSSIAN: exp(-param d^2) - exp(-param r^2), param = alpha >= 0; BLACKMAN_HARRIS: the 4-term window
 *           0.35875 - 0.48829 cos(2 pi u) + 0.14128 cos(4 pi u) - 0.01168 cos(6 pi u) at u = (d + r) / (2 r); each clamped at 0.
 *           EINVAL for an unknown kind, radii outside (0, 3], a table size outside [1, 64], a null output or a bad alpha. */
#define BCD_HIP_FILTER_BOX 0
#define BCD_HIP_FILTER_TENT 1
#define BCD_HIP_FILTER_GAUSSIAN 2
#define BCD_HIP_FILTER_BLACKMAN_HARRIS 3
int  bcd_hip_accum_set_filter(bcd_hip_accum *acc, float radius_x, float radius_y, int table_size, const float *h_table);
int  bcd_hip_accum_add_splatted(bcd_hip_accum *acc, const float *d_xy, const float *d_rgb, const float *d_weights, int64_t n);
int  bcd_hip_filter_table(int kind, float radius_x, float radius_y, float param, int table_size, float *h_out);
/* Adaptive sample planning on the accumulator's state: where the next `budget` samples go, decided on the device
 * from the noise model the denoiser uses (cov / n), with no host copy and no float atomics; reproducible bit for bit.  Per pixel, from
 * the snapshot's statistics (ns, mean m, covariance c, float32, IEEE division and sqrtf):
 *     t = (c_xx / ns + c_yy / ns) + c_zz / ns   (as c * (1 / ns)),   l = (m_r + m_g) + m_b
 *     e = +inf if !(ns >= min_samples) or t, l not finite, else sqrtf(max(t / 3, 0)) / (eps + max(l / 3, 0))
 * A pixel is active when e > threshold; E = the largest finite e of the active pixels.  Weight q = 0 (inactive), 2^24 (e = inf), else
 * max(1, (uint32)((e / E) * 2^24)).  With C the inclusive scan of q in pixel order (line * W + col), Q its total and u = offset mod Q:
 *     n_p = min(max_per_pixel, floor((C_p B + u) / Q) - floor((C_{p-1} B + u) / Q))        (exact integers; Q = 0 or B = 0: all 0)
 * so before the cap the counts sum to B exactly and each is the floor or the ceiling of B q_p / Q; changing `offset` from pass to pass
 * rotates the leftover fractions over the pixels.
 *   plan: budget B in [0, 2^31); d_error W*H floats or NULL; d_counts W*H int32 or NULL; d_pixels[capacity], capacity >= budget,
 *         receives T = sum n_p pixel indices in ascending order, pixel p repeated n_p times (the d_pixel of add_scattered); d_summary
 *         receives planned T, the active pixels, the unsampled ones (active with e = inf) and E.  Enqueued on the context's stream, no
 *         synchronisation; the state is not changed.  EINVAL with nothing enqueued for null acc / params / d_pixels / d_summary,
 *         capacity < budget, threshold not finite or < 0, eps not finite or <= 0, min_samples not finite or < 0, max_per_pixel outside
 *         [1, 65535].  The scratch is allocated by create when max_batch_samples > 0, else by the first plan; later plans never allocate.
 *   default_plan_params: threshold 0, eps 1e-3, min_samples 2, max_per_pixel 16 */
typedef struct bcd_hip_plan_params {
    float   threshold;      /* tau: pixels with e <= tau get no samples               default 0     */
    float   eps;            /* added to the luminance of the relative error            default 1e-3  */
    float   min_samples;    /* pixels whose weight sum is below it have e = inf         default 2     */
    int32_t max_per_pixel;  /* K: cap of n_p                                             default 16    */
} bcd_hip_plan_params;
typedef struct bcd_hip_plan_summary {
    int64_t planned;        /* T, the entries written to d_pixels                                    */
    int64_t active;         /* pixels with e > threshold                                              */
    int64_t unsampled;      /* active pixels with e = inf (below min_samples, or non-finite statistics) */
    float   max_error;      /* E, the largest finite e of the active pixels (0 if none)               */
} bcd_hip_plan_summary;
void bcd_hip_default_plan_params(bcd_hip_plan_params *p);
int  bcd_hip_accum_plan(bcd_hip_accum *acc, const bcd_hip_plan_params *params, int64_t budget, uint64_t offset, float *d_error, int32_t *d_counts,
                        int32_t *d_pixels, int64_t capacity, bcd_hip_plan_summary *d_summary);
/* States: export, import, merge.  Serialised state, format v1: a 64-byte little-endian header, then the
 * nb_planes = 11 + 3 * nb_bins planes exactly as they sit in HBM, nb_planes * height * width fp32 values: ACC_W (weight sum), ACC_W2
 * (squared-weight sum), the 3 weighted colour sums, the 6 weighted second moments (xx, yy, zz, yz, xz, xy), then the bins channel-major
 * (bin index ch * nb_bins + bin); each plane in pixel order line * width + col.  The total size is exactly 64 + 4 * nb_planes * W * H
 * bytes.  Field offsets: magic 0, version 8, header_bytes 12, width 16, height 20, nb_bins 24, gamma 28, max_value 32, nb_planes 36,
 * samples_added 40, dropped 48, reserved 56.
 *   state_info: host only (no device, no context): reads the first 64 bytes at h_state, `bytes` being the size of the whole state;
 *           EINVAL unless magic, version, header_bytes, nb_bins in [2, 85], positive sizes below 2^31 pixels, nb_planes, the exact size,
 *           zero reserved bytes and non-negative counters hold.  out may be NULL.
 *   state_bytes: the serialised size of the accumulator's state (no synchronisation).
 *   export: header + planes into h_state[capacity]; synchronises; the state is unchanged.
 *   import: replaces the state and the counters; W, H, nb_bins, gamma and max_value must equal the accumulator's (gamma and max_value
 *           bit for bit).
 *   merge_state / merge: dst[i] = dst[i] + src[i] for every float of the state, one IEEE fp32 add and nothing else; samples_added and
 *           dropped add up.  A merge of A into B has the bits of a merge of B into A; addition is not associative, so a caller that
 *           merges several states fixes the order.
 * Import and merge refuse a malformed state, a geometry or parameter mismatch, dst == src and null pointers with EINVAL before any
 * device work, the state untouched; a refused call does not block the next one (after EDEVICE the state is undefined).  import and
 * merge_state return once h_state is no longer needed (it goes through two pinned staging chunks of at most 64 MiB owned by the
 * accumulator, allocated on first use); their device work stays ordered on the context's stream.  merge reads everything already
 * enqueued on src's stream and nothing enqueued there after the call (events in both directions, the host is not blocked); src may
 * belong to another context, on the same or another device (another device: chunks of at most 64 MiB through two dst-side scratch
 * buffers, peer copies; no peer access needed).  No scratch of the state's size is ever allocated. */
typedef struct bcd_hip_accum_state_header {
    char     magic[8];       /* the 8 bytes BCDACCST, no terminator */
    uint32_t version;        /* 1 */
    uint32_t header_bytes;   /* 64: offset of the first plane */
    int32_t  width, height, nb_bins;
    float    gamma, max_value;
    uint32_t nb_planes;      /* 11 + 3 * nb_bins */
    int64_t  samples_added;  /* as bcd_hip_accum_info */
    int64_t  dropped;
    uint8_t  reserved[8];    /* zero */
} bcd_hip_accum_state_header;
#define BCD_HIP_ACCUM_STATE_VERSION 1
#define BCD_HIP_ACCUM_STATE_HEADER_BYTES 64
int  bcd_hip_accum_state_info(const void *h_state, int64_t bytes, bcd_hip_accum_state_header *out);
int  bcd_hip_accum_state_bytes(bcd_hip_accum *acc, int64_t *bytes);
int  bcd_hip_accum_export(bcd_hip_accum *acc, void *h_state, int64_t capacity);
int  bcd_hip_accum_import(bcd_hip_accum *acc, const void *h_state, int64_t bytes);
int  bcd_hip_accum_merge_state(bcd_hip_accum *acc, const void *h_state, int64_t bytes);
int  bcd_hip_accum_merge(bcd_hip_accum *dst, bcd_hip_accum *src);
/* Colour layers beside the beauty: an accumulator created with nb_layers extra colour layers keeps, per layer, the
 * nine running sums that bcd_hip_denoise_layers needs of it -- 3 weighted colour sums and 6 weighted second moments (xx, yy, zz, yz, xz,
 * xy), 36 bytes per pixel -- in a buffer of its own, layer-major, each plane in pixel order.  The weight sum, the squared-weight sum and
 * the histogram are the beauty's: every layer sees the same sample weights.  The shared state, its format v1 and every entry point
 * above behave as on an accumulator without layers, except that the plain adds are refused.
 *   Rule: every add takes the layers' colours beside the beauty's.  Each (pixel, layer) is owned by one thread and receives its
 *     contributions in stream order, with the nine colour-sum operations of addSample in their order and the beauty's weight (for splats
 *     w * f); no float atomics.  Layer k's mean and covariance are therefore bit for bit those of a separate accumulator (the host class
 *     or bcd_hip_accum_*) fed layer k's colours with the same weights and stream, and the beauty's four statistics are bit for bit those
 *     of an accumulator without layers.  The beauty goes through the kernels of the plain adds.
 *   create_layers: nb_layers in [1, BCD_HIP_ACCUM_MAX_LAYERS], otherwise EINVAL; everything else is create.  With max_batch_samples > 0 no
 *           later add allocates.  nb_layers: 0 for an accumulator made by create.
 *   add_dense_layers / add_scattered_layers / add_splatted_layers: the plain add's arguments, then d_layer_*: a HOST array of nb_layers
 *           DEVICE pointers, none null, each to data laid out like the beauty's buffer of that call (dense: layer_channels, 3 or 4, floats
 *           per sample, independent of `channels`; scattered and splatted: [n][3]).  Dropped samples (out-of-range indices, non-finite
 *           positions, empty footprints) are dropped for every layer and counted once.  Batches split into chunks as the plain forms
 *           do; no bit depends on the split.
 *   Refusals, EINVAL with a message before any device work, the state untouched: a plain add_dense / add_scattered / add_splatted on
 *           an accumulator with layers (it would move the weight sums without the layers), a _layers add on one without, a null list or
 *           a null entry.
 *   layer_statistics: d_mean, d_cov: HOST arrays of nb_layers DEVICE pointers to W*H*3 and W*H*6 floats; the statistics of
 *           bcd_hip_accum_statistics on each layer's sums with the shared weight sums.  Enqueued on the context's stream, no
 *           synchronisation, the state unchanged.  bcd_hip_accum_statistics gives the beauty.  Together they are the inputs of
 *           bcd_hip_denoise_layers (beauty first).
 *   reset clears the layers; merge needs equal nb_layers on both sides (EINVAL otherwise) and adds the layer planes too, one fp32 add
 *           per float on either of its paths; plan reads the beauty.
 *   Layer block: the serialised layers, a block of its own, so that format v1 is not touched: a 64-byte little-endian header -- magic
 *           "BCDACCLY" 0, version (1) 8, header_bytes (64) 12, width 16, height 20, nb_layers 24, nb_planes = 9 * nb_layers 28, 32 zero
 *           reserved bytes 32 -- then the planes as they sit in HBM; exactly 64 + 36 * nb_layers * W * H bytes.  A checkpoint of an
 *           accumulator with layers is its v1 state (export / import / merge_state, which act on the shared part alone) PLUS its layer
 *           block (export_layers / import_layers / merge_layers_state); the caller keeps the two together.
 *   layers_state_info: host only (no device, no context), as state_info: EINVAL unless magic, version, header_bytes, nb_layers in
 *           [1, 15], positive sizes below 2^31 pixels, nb_planes, the exact size and zero reserved bytes hold.  out may be NULL.
 *   layers_state_bytes / export_layers / import_layers / merge_layers_state: as their v1 counterparts, through the same staging chunks;
 *           a malformed block, another frame size or another layer count give EINVAL before any device work.  export synchronises. */
#define BCD_HIP_ACCUM_MAX_LAYERS (BCD_HIP_MAX_LAYERS - 1)
int  bcd_hip_accum_create_layers(bcd_hip_ctx *ctx, int W, int H, int nb_bins, float gamma, float max_value, int64_t max_batch_samples, int nb_layers,
                                 bcd_hip_accum **acc);
int  bcd_hip_accum_nb_layers(bcd_hip_accum *acc, int *nb_layers);
int  bcd_hip_accum_add_dense_layers(bcd_hip_accum *acc, const float *d_samples, const float *d_weights, int row_begin, int rows, int spp, int channels,
                                    const float *const *d_layer_samples, int layer_channels);
int  bcd_hip_accum_add_scattered_layers(bcd_hip_accum *acc, const int32_t *d_pixel, const float *d_rgb, const float *d_weights, int64_t n,
                                        const float *const *d_layer_rgb);
int  bcd_hip_accum_add_splatted_layers(bcd_hip_accum *acc, const float *d_xy, const float *d_rgb, const float *d_weights, int64_t n,
                                       const float *const *d_layer_rgb);
int  bcd_hip_accum_layer_statistics(bcd_hip_accum *acc, float *const *d_mean, float *const *d_cov);
typedef struct bcd_hip_accum_layers_header {
    char     magic[8];       /* the 8 bytes BCDACCLY, no terminator */
    uint32_t version;        /* 1 */
    uint32_t header_bytes;   /* 64: offset of the first plane */
    int32_t  width, height, nb_layers;
    uint32_t nb_planes;      /* 9 * nb_layers */
    uint8_t  reserved[32];   /* zero */
} bcd_hip_accum_layers_header;
#define BCD_HIP_ACCUM_LAYERS_VERSION 1
#define BCD_HIP_ACCUM_LAYERS_HEADER_BYTES 64
int  bcd_hip_accum_layers_state_info(const void *h_layers, int64_t bytes, bcd_hip_accum_layers_header *out);
int  bcd_hip_accum_layers_state_bytes(bcd_hip_accum *acc, int64_t *bytes);
int  bcd_hip_accum_export_layers(bcd_hip_accum *acc, void *h_layers, int64_t capacity);
int  bcd_hip_accum_import_layers(bcd_hip_accum *acc, const void *h_layers, int64_t bytes);
int  bcd_hip_accum_merge_layers_state(bcd_hip_accum *acc, const void *h_layers, int64_t bytes);
/* Auxiliary feature channels beside the beauty ("Features"): an accumulator created with nb_features = F channels
 * (albedo, normal, depth, object id ...) keeps, per channel k, two more running sums -- s1_k = sum w x_k and s2_k = sum w x_k x_k, 8 bytes per
 * pixel and channel -- in a buffer of its own, plane-major, channel after channel (s1_0, s2_0, s1_1, ...).  Its snapshot is the pair of
 * images of a bcd_hip_guide: the weighted mean of every channel and the variance of that mean, W*H*F floats each, pixel-interleaved, so
 * that samples go in and bcd_hip_denoise_guided comes out without leaving the device.  The weight sum and the squared-weight sum are the
 * beauty's.  The shared state, the layers, their formats and every entry point above behave as on an accumulator without features,
 * except that the plain and the _layers adds are refused.
 *   Rule: every add takes the samples' feature channels beside the beauty's colours.  Each pixel is owned by one thread and receives its
 *     contributions in stream order with the beauty's weight (for splats w * f, one multiplication), float32, no contraction, no float
 *     atomics:   s1_k += w * x_k;   s2_k += (w * x_k) * x_k;   the operations of addSample on the first colour channel.
 *   Snapshot, per pixel and channel, from the beauty's wsum and w2sum:
 *         inv = 1.f / wsum;   mean = inv * s1;   cv = s2 * inv;   cv -= mean * mean;
 *         r = w2sum / (wsum * wsum);   bias = 1.f / (1 - r);   v = cv * bias;   vm = v * r;   variance = (vm > 0.f) ? vm : 0.f;
 *     mean and v have the bits of mean[0] and cov[0] of a SamplesAccumulator (the host class, bcd_hip_accum_*) fed the same stream with
 *     R = x_k.  vm is the variance of the weighted mean (unit weights: v / n), the `variances` of bcd_hip_guide.  The clamp stores +0 for
 *     whatever is not a positive number -- negative round-off, NaN, a zero of either sign: an infinite depth gives mean = inf and
 *     variance 0 (inf against inf is a skipped NaN term of the guide distance, inf against finite a counted infinite one); a pixel with
 *     one sample gives its value and 0 * inf = NaN -> 0; a pixel without samples gives mean NaN and variance 0.  s2 / n - mean^2
 *     cancels in float32: a channel of magnitude M resolves variances down to about 1e-7 M^2, so normalise depth (and any channel of
 *     large magnitude) to order 1 before accumulating it.
 *   create_features: nb_layers in [0, BCD_HIP_ACCUM_MAX_LAYERS], nb_features in [1, BCD_HIP_ACCUM_MAX_FEATURES], otherwise EINVAL;
 *           everything else is create / create_layers.  With max_batch_samples > 0 no later add allocates (the feature kernels read the
 *           caller's buffers and need no scratch).  nb_features: 0 for an accumulator made by create or create_layers.
 *   add_dense_features / add_scattered_features / add_splatted_features: the arguments of the _layers form, then d_features: a DEVICE
 *           pointer to [sample][F] floats, laid out like the beauty's samples of that call (dense: ((line - row_begin) * W + col) * spp + i;
 *           scattered and splatted: [n][F]).  The layer list is NULL exactly when the accumulator has no layers.  Dropped samples are
 *           dropped for the features too and counted once.  Batches split into chunks as the other forms do; no bit depends on the
 *           split, nor on the alignment of d_features (aligned buffers are read with wider loads).
 *   feature_statistics: d_features, d_variances: W*H*F floats each; d_variances may be NULL.  Enqueued on the context's stream, no
 *           synchronisation, the state unchanged.
 *   reset clears the feature planes; merge needs equal nb_features on both sides (EINVAL otherwise) and adds the feature planes too, one
 *           fp32 add per float on either of its paths; plan, statistics, moments, layer_statistics and the v1 state and layer block
 *           calls act as on an accumulator without features.
 *   Feature block: the serialised feature planes, a block of its own beside the v1 state and the layer block: a 64-byte little-endian
 *           header -- magic "BCDACCFT" 0, version (1) 8, header_bytes (64) 12, width 16, height 20, nb_features 24, nb_planes =
 *           2 * nb_features 28, 32 zero reserved bytes 32 -- then the planes as they sit in HBM; exactly 64 + 8 * nb_features * W * H bytes.
 *   features_state_info: host only (no device, no context): EINVAL unless magic, version, header_bytes, nb_features in [1, 8], positive
 *           sizes below 2^31 pixels, nb_planes, the exact size and zero reserved bytes hold.  out may be NULL.
 *   features_state_bytes / export_features / import_features / merge_features_state: as their layer counterparts, through the same
 *           staging chunks.  export synchronises.
 *   Refusals, EINVAL with a message before any device work, the state untouched and the context usable: nb_features or nb_layers out of
 *           range; a plain or _layers add on an accumulator with features (it would move the weight sums without the features); a
 *           _features add, feature_statistics or a feature block call on an accumulator without features; a null d_features; a layer
 *           list without layers, no list with them, a null entry; a malformed block, another frame size, another channel count;
 *           feature_statistics with a null d_features or outputs that overlap. */
#define BCD_HIP_ACCUM_MAX_FEATURES BCD_HIP_GUIDE_MAX_CHANNELS
int  bcd_hip_accum_create_features(bcd_hip_ctx *ctx, int W, int H, int nb_bins, float gamma, float max_value, int64_t max_batch_samples, int nb_layers,
                                   int nb_features, bcd_hip_accum **acc);
int  bcd_hip_accum_nb_features(bcd_hip_accum *acc, int *nb_features);
int  bcd_hip_accum_add_dense_features(bcd_hip_accum *acc, const float *d_samples, const float *d_weights, int row_begin, int rows, int spp, int channels,
                                      const float *const *d_layer_samples, int layer_channels, const float *d_features);
int  bcd_hip_accum_add_scattered_features(bcd_hip_accum *acc, const int32_t *d_pixel, const float *d_rgb, const float *d_weights, int64_t n,
                                          const float *const *d_layer_rgb, const float *d_features);
int  bcd_hip_accum_add_splatted_features(bcd_hip_accum *acc, const float *d_xy, const float *d_rgb, const float *d_weights, int64_t n,
                                         const float *const *d_layer_rgb, const float *d_features);
int  bcd_hip_accum_feature_statistics(bcd_hip_accum *acc, float *d_features, float *d_variances);
typedef struct bcd_hip_accum_features_header {
    char     magic[8];       /* the 8 bytes BCDACCFT, no terminator */
    uint32_t version;        /* 1 */
    uint32_t header_bytes;   /* 64: offset of the first plane */
    int32_t  width, height, nb_features;
    uint32_t nb_planes;      /* 2 * nb_features */
    uint8_t  reserved[32];   /* zero */
} bcd_hip_accum_features_header;
#define BCD_HIP_ACCUM_FEATURES_VERSION 1
#define BCD_HIP_ACCUM_FEATURES_HEADER_BYTES 64
int  bcd_hip_accum_features_state_info(const void *h_features, int64_t bytes, bcd_hip_accum_features_header *out);
int  bcd_hip_accum_features_state_bytes(bcd_hip_accum *acc, int64_t *bytes);
int  bcd_hip_accum_export_features(bcd_hip_accum *acc, void *h_features, int64_t capacity);
int  bcd_hip_accum_import_features(bcd_hip_accum *acc, const void *h_features, int64_t bytes);
int  bcd_hip_accum_merge_features_state(bcd_hip_accum *acc, const void *h_features, int64_t bytes);
/* checkAndPutToZeroNegativeInfNaNValues   src/cli/main.cpp:389-420 */
int bcd_hip_zero_bad_values(bcd_hip_ctx *ctx, float *d_img, int64_t n);

/* self-test: the scale-free division used by the pair-distance kernel against the compiler's IEEE division on
 * `samples` hashed operand pairs drawn from its guarded range; *mismatches must come back 0 */
int bcd_hip_selftest_division(bcd_hip_ctx *ctx, uint32_t seed, int64_t samples, int64_t *mismatches);
/* self-test of the pair-distance kernels on given inputs: the production variant (fast division; the uniform power-of-two sample-count
 * formula when it applies) against the compiler's division with the general formula; *mismatches = entries of the T / C planes that
 * differ bitwise (0 expected unless a range / count flag was raised: *variant bits 4..); *variant & 15: 1 = fast, 2 = fast + uniform */
int bcd_hip_selftest_distance_kernels(bcd_hip_ctx *ctx, const float *d_hist, const float *d_nsamples, int W, int H, int D, int search_radius,
                                      int *variant, int64_t *mismatches);

/* Measurement (bench.py `roofline.valu`): the arithmetic the production distance kernel performs on this frame, from a counting instantiation
 * of the same kernel -- lane_bins: (pixel pair, bin) terms evaluated = the reference's own count of bins with b1 + b2 > 1 over the half-plane
 * displacements (src/core/DenoisingUnit.cpp:379-381); wave_bins: bins a wavefront issues because at least one of its 64 pairs needs them;
 * wave_groups: groups of four bins entered -- and kernel_ms: the production instantiation on the same input (HIP events, best of reps). */
int bcd_hip_selftest_bin_work(bcd_hip_ctx *ctx, const float *d_hist, const float *d_nsamples, int W, int H, int D, int search_radius, int reps,
                              int64_t *lane_bins, int64_t *wave_bins, int64_t *wave_groups, float *kernel_ms);

/* self-test of the approximate pair-distance kernel (k_pairdist_rw) on given inputs: *max_rel_dev = largest relative deviation of a
 * patch distance d(p, p + delta) computed from the approximate planes from the one computed from the exact planes, over all pairs of
 * main pixels (bound 5e-4, measured 2.4e-4; must stay below 2^-10 = 9.8e-4, BCD_APPROX_DELTA, the half-width of the band that is
 * re-evaluated exactly); *count_mismatches = pairs whose
 * integer bin counts differ (must be 0); *flags: low nibble 2 = the uniform kernel ran, 3 = the RATIO form (general sample counts: the production kernel for
 * them since round 6), the kernels' flag word above it (bit 2, value 4 << 4: the RATIO form's absolute-error check declined) */
int bcd_hip_selftest_approx_distance(bcd_hip_ctx *ctx, const float *d_hist, const float *d_nsamples, int W, int H, int D, int search_radius,
                                     float *max_rel_dev, int64_t *count_mismatches, int *flags);

/* self-test: the compaction of the processed pixels into the two lists of the estimate call, on its own.  Of the pixels of lines [main_row_begin,
 * main_row_end) with state 1 (processed), d_strong receives the indices line * W + col of those with d_count >= 3 (2 patch_radius + 1)^2 + 1 and d_weak
 * the others, each list in no particular order (room for (main_row_end - main_row_begin) * W entries each); counts_out[0..1] = the two list lengths,
 * counts_out[2..3] = the 64-bit sum of d_count over both lists (low word first).  d_skip_word (optional): a device word; when it is not zero the launch
 * writes nothing -- the lists keep what they held and all four counts come back 0. */
int bcd_hip_selftest_active_lists(bcd_hip_ctx *ctx, const uint8_t *d_state, const int32_t *d_count, int W, int H, int patch_radius, int main_row_begin,
                                  int main_row_end, const int64_t *d_skip_word, int32_t *d_strong, int32_t *d_weak, int32_t counts_out[4]);

/* ---- the host-buffer upload path piece by piece (self-tests; what the host-buffer entry points run, not copies of it) ---- */
/* The sparse histogram upload on its own: n host floats through the context's uploader (created as bcd_hip_denoise_host_ex creates it) to d_dst -- any
 * alignment; a destination that is not 16-byte aligned travels as a plain copy -- on the upload stream, synchronised before the call returns.
 * new_frame != 0 starts a frame first (byte counters cleared, the "this frame is dense" decision forgotten); piece_floats: the length of a piece, a
 * multiple of 4, 0 = the 12 Mi floats of the host path (the length is set for this call alone).  *raw_bytes, *sent_bytes: the frame's counters so far.
 * The packed form of a piece of n floats is 66 words per block of 2048 floats (64 mask words, the offset and the count of the block's values) plus
 * the values whose bit pattern is not zero; a piece with more than 60 % of them travels as it is, and so does the rest of its frame. */
int bcd_hip_selftest_sparse_upload(bcd_hip_ctx *ctx, const float *h_src, int64_t n, float *d_dst, int new_frame, int64_t piece_floats,
                                   int64_t *raw_bytes, int64_t *sent_bytes);
/* The streamed upload of bcd_hip_denoise_host_ex on its own (frames of >= 256 lines on the approximate-planes path; BCD_HIP_EUNSUPPORTED otherwise): the
 * frame arrives in row chunks, the lines that have arrived are prefiltered (spike_factor > 0) and the approximate distance planes of the tile rows
 * whose lines are complete are launched.  stop_after_chunks = k >= 0: only chunks 0 .. k-1 are uploaded and scheduled (< 0: all); poison != 0: every
 * device buffer the schedule reads or writes (uploaded copies, filtered copies, planes) holds 0xFF bytes before the first transfer.  Copied out
 * afterwards: d_planes (binary16, delta-major: bcd_delta_count(b) planes of W*H), d_counts (one byte per entry, same layout), the four images the
 * planes were computed on (the filtered copies with the prefilter, else the uploaded ones), and -- d_hist_uploaded, optional -- the uploaded histograms. */
typedef struct bcd_hip_host_stream_result {
    int32_t rows_filtered;   /* prefiltered lines [0, rows_filtered); 0 without the prefilter */
    int32_t tile_rows_done;  /* plane tile rows (4 lines each) [0, tile_rows_done) */
    int32_t chunk_lines;     /* lines per chunk */
    int32_t chunks_done;
    int32_t range_flag;      /* the distance kernel's flags: bit 0 a value out of range, bit 1 a pixel carries another sample count than uni_n,
                              * bit 2 (all chunks in) the RATIO form's verdict declined */
    float   uni_n;           /* the uniform sample count the planes were launched for (0: general sample counts) */
    int32_t ratio_form;      /* general sample counts: 1 = by the RATIO form of the kernel (what a resident frame gets), 0 = by the reference's operations */
} bcd_hip_host_stream_result;
int bcd_hip_selftest_host_stream(bcd_hip_ctx *ctx, const float *h_colors, const float *h_nsamples, const float *h_histograms, const float *h_covariances,
                                 int W, int H, int D, const bcd_hip_params *prm, float spike_factor, int stop_after_chunks, int poison,
                                 void *d_planes, uint8_t *d_counts, float *d_colors_out, float *d_nsamples_out, float *d_histograms_out,
                                 float *d_covariances_out, float *d_hist_uploaded, bcd_hip_host_stream_result *res);
/* the approximate distance planes of a resident frame in ONE launch of a full-frame launcher (uni_n: the uniform power-of-two sample count, 0 = general
 * sample counts: by the reference's operations, or -- ratio_form != 0 -- by the RATIO form with its verdict for threshold tau), written to d_planes /
 * d_counts (layout as above; entries whose neighbour lies outside the image are not written); *range_flag as above.  What the partitioned launches of
 * the streamed upload must equal bit for bit. */
int bcd_hip_approx_planes(bcd_hip_ctx *ctx, const float *d_hist, const float *d_nsamples, int W, int H, int D, int search_radius, float uni_n,
                          int ratio_form, float tau, void *d_planes, uint8_t *d_counts, int *range_flag);

/* the eigensolver of the Bayesian steps on its own (Eigen::SelfAdjointEigenSolver of DenoisingUnit.cpp:589,617 for 27 x 27 matrices):
 * d_A = n symmetric matrices, 28 x 28 floats each, row-major, row / column 27 zero; d_eig[n][28] = eigenvalues (unordered, entry 27 = 0),
 * d_V[n][28][28] = eigenvectors in columns, same order (rows 0..26 written); *ms = kernel time (may be NULL).  Parity / timing aid. */
int bcd_hip_eig27_batch(bcd_hip_ctx *ctx, const float *d_A, int n, float *d_eig, float *d_V, float *ms);
/* bcd_hip_eig27_batch always stops at off^2 <= 1e-12 diag^2 (the strict rule; bcd_hip_set_strict_eigensolver does not reach it).  This one selects:
 * production_rule != 0 stops where the estimate chain stops by default, off^2 <= 2e-9 diag^2 -- WITHOUT the first-order correction the finish kernels
 * apply to the residual (it is not returned), so V diag(eig) V^T is then only accurate to sqrt(2e-9) |A|_F; 0 is bcd_hip_eig27_batch. */
int bcd_hip_eig27_batch_rule(bcd_hip_ctx *ctx, const float *d_A, int n, float *d_eig, float *d_V, float *ms, int production_rule);

/* the prepare and eigensolver phases of a full estimate, as two kernels and as the fused kernel, on the same list: d_list holds main-pixel indices
 * (line * W + column, |S| >= 28, masks of search radius 6), `capacity` is the number of records the chunk is sized for and list_len the list's length:
 * list_len < 0: the kernels process `capacity` items; otherwise the length is read on the DEVICE and min(capacity, list_len) items are processed (the
 * path of a chunk launched ahead of the host's count).  cu_share_pct (1..100): share of the CU slots the grids are sized for.  Both runs start from
 * records filled with one byte pattern; *differing_words = number of 32-bit words of the records (A after the solver, V, C, noise + mean, eigenvalues)
 * and of the redo list's counter in which they differ afterwards.  The same device functions on the same inputs in the same order: 0. */
int bcd_hip_selftest_prepare_solve(bcd_hip_ctx *ctx, const float *d_colors, const float *d_pixcov, const uint32_t *d_mask, const int32_t *d_list,
                                   int capacity, int list_len, int W, int H, int search_radius, int cu_share_pct, int64_t *differing_words);

/* ---- host utilities (no device work) ----------------------------------------------------------- */
/* the visiting order implied by (random_order, seed): main-pixel linear indices line*W+col in
 * visiting order, written to h_order[(W-2w)*(H-2w)].  random_order == 0 is the reference's
 * single-thread scanline order (Denoiser.cpp:136-146). */
int bcd_hip_visit_order(int W, int H, int patch_radius, int random_order, uint32_t seed, int32_t *h_order);
/* order 2 (strips): the `seed` argument of bcd_hip_visit_order / bcd_hip_active_set carries the frame geometry instead of a seed */
uint32_t bcd_hip_strip_order_seed(int W, int H, int patch_radius, int search_radius);
/* seed used for scale s of a multiscale run started with seed0 */
uint32_t bcd_hip_scale_seed(uint32_t seed0, int scale);

#ifdef __cplusplus
}
#endif
#endif
