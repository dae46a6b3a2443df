// bcd_ctx.h -- internal to the host orchestration files (bcd_api.hip, bcd_host.hip, bcd_accum.hip, bcd_selection.hip, bcd_selftest.hip, bcd_spike.hip,
// bcd_temporal.hip, bcd_temporal_layers.hip, bcd_sequence.hip): the context, the per-scale workspace with its counter block, the error-handling macros and the helpers more
// than one of those files needs.  Nothing declared here is part of the C ABI (include/bcd_hip.h): the helpers have hidden visibility.
#pragma once
#include "../../include/bcd_hip.h"
#include "bcd_common.h"
#include "bcd_launch.h"

#include <condition_variable>
#include <cstddef>
#include <cmath>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

static_assert(BCD_MAX_LAYERS == BCD_HIP_MAX_LAYERS, "the layer tables of the kernels hold what the C ABI admits");
static_assert(BCD_GUIDE_MAX_CHANNELS == BCD_HIP_GUIDE_MAX_CHANNELS, "the floors table of the guide kernel holds what the C ABI admits");

constexpr int MAX_SCALES = 16;
constexpr int ROUND_BATCH = 16;
constexpr int MAX_EVENT_PAIRS = 4096;
// the estimate chunk: full-estimate items whose records (bcd_bayes27_record_bytes() each) are in flight at a time: 262144 pixels = 2.6 GB of records
// (round 6: 2^18 instead of 2^17 -- half as many drains of the three persistent kernels on a -m 0 frame: 60.9 -> 60.2-60.5 ms at 1080p; sizes aligned to
// the eigensolver's 6 144 matrices per round of the grid made no difference)
constexpr int ESTIMATE_CHUNK = 1 << 18;

// (hidden: what the host files instantiate on these types stays out of the dynamic symbol table, as when they were file-local)
#pragma GCC visibility push(hidden)

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

// the colour layers of a bcd_hip_denoise_layers call BEYOND the first, at one scale: the first layer travels through the arguments bcd_hip_denoise has
struct LayerView {
    int n = 0;
    const float *col[BCD_MAX_LAYERS], *cov[BCD_MAX_LAYERS];
    float *out[BCD_MAX_LAYERS];
};

// The counter block of a workspace: 64 words on the device (Work::counters) and a pinned host mirror of the same layout (Work::h_counters).
//
// | words  | device                                                                  | host mirror                                                      |
// |--------|-------------------------------------------------------------------------|------------------------------------------------------------------|
// | 0..15  | undecided pixels per marking launch of a batch (k_sum_counter_lines)    | the same, copied per batch                                       |
// | 16, 17 | list lengths: full estimate (strong), fallback (weak)                   | the same                                                         |
// | 18..19 | sum of |S| (64 bit)                                                     | the same                                                         |
// | 20..22 | work counters of the generic estimate kernel                            | --                                                               |
// | 23     | spectral-inverse (redo) count                                           | the same; layers_follow leaves the sum over the layers here      |
// | 24..39 | 32..33: scratch of the self-tests                                       | 24 + k: running redo total after follower layer k (up to 16)     |
// | 40..43 | range / count flag, uniform-count scan, "another sample count",         | the same                                                         |
// |        | borderline pairs (k_sum_counter_lines reads [0], [2], [3] of them)      |                                                                  |
// | 44     | --                                                                      | the first pixel's sample count (scan_uniform_count)              |
// | 48..53 | marking total (64 bit), or the three 64-bit counters of the bin-work    | 48..49: marking total                                            |
// |        | self-test                                                               |                                                                  |
//
// The kernels see two groups relative to a base pointer: `lists` (d_c[0..7], from word 16) and `flags` (d_flag[0..3], from word 40).
struct Counters {
    int32_t undecided[ROUND_BATCH];
    struct Lists {
        int32_t n_strong, n_weak;
        int64_t sim_total;        // sum of |S|
        int32_t generic_work[3];  // DEVICE ONLY: work counters of the generic estimate kernel
        int32_t spectral;         // full estimates that took the spectral inverse (the redo list's length)
    } lists;
    struct SelftestScratch { int32_t below[8]; unsigned long long result; };
    union {
        int32_t layer_redo_total[BCD_MAX_LAYERS]; // HOST ONLY: [k] = `spectral` after follower layer k (a frame: BCD_MAX_LAYERS - 1 in use; a kept selection: all)
        SelftestScratch selftest;                 // DEVICE ONLY: result word(s) of the self-tests
    };
    struct Flags {
        int32_t range;            // the distance kernels' range / count flag (bit 1: not one sample count, bit 2: the RATIO form declined)
        int32_t scan;             // != 0: k_uniform_n found two sample counts
        int32_t other_count;      // a pixel carries another sample count than the uniform kernel was launched for (plain-store flag)
        int32_t borderline;       // borderline pairs listed (may exceed the list's capacity)
    } flags;
    float first_count;            // HOST ONLY: the first pixel's sample count
    int32_t unused_45[3];
    union {
        long long marking_total;        // all-reduced count of undecided pixels of a marking batch (+ 2^40: the masks did not pass)
        unsigned long long bin_work[3]; // DEVICE ONLY: bcd_hip_selftest_bin_work
    };
    int32_t unused_54[10];
};
constexpr int COUNTER_WORDS = (int)(sizeof(Counters) / sizeof(int32_t));
#define COUNTER_WORD(member) ((int)(offsetof(Counters, member) / sizeof(int32_t)))
static_assert(COUNTER_WORDS == 64, "the counter block is 64 ints");
static_assert(COUNTER_WORD(lists) == 16 && COUNTER_WORD(lists.spectral) == 23 && sizeof(Counters::Lists) == 8 * sizeof(int32_t), "d_c[0..7] of the list and estimate kernels");
static_assert(COUNTER_WORD(flags) == 40 && COUNTER_WORD(flags.other_count) == 42 && COUNTER_WORD(flags.borderline) == 43 && sizeof(Counters::Flags) == 4 * sizeof(int32_t),
              "d_flag[0..3] of the distance, mask and k_sum_counter_lines kernels");
static_assert(COUNTER_WORD(marking_total) == 48 && COUNTER_WORD(selftest.result) == 32, "words the kernels are handed");
static_assert(offsetof(Counters, lists.sim_total) % 8 == 0 && offsetof(Counters, selftest.result) % 8 == 0 && offsetof(Counters, marking_total) % 8 == 0 &&
                  offsetof(Counters, bin_work) % 8 == 0, "64-bit counters are 8-byte aligned");
static_assert(COUNTER_WORD(layer_redo_total) + BCD_MAX_LAYERS <= COUNTER_WORD(flags), "the per-layer running totals end below the flag words");
static_assert(COUNTER_WORD(first_count) > COUNTER_WORD(flags.borderline), "the first pixel's count does not alias a flag word");

// the lists of a kept selection (bcd_selection.hip), handed to layers_follow in place of the workspace's own
struct KeptLists {
    const int32_t *strong, *weak; // full-estimate items, fallback pixels
    const int32_t *d_len;         // on the device: their lengths (n_strong, n_weak), for the kernels that read them there
    int n_strong;
};

#pragma GCC visibility pop

// everything one scale's pipeline needs: a multiscale run drives one Work per scale concurrently (own stream, own host
// thread), because the scales are independent until the merge and the coarse ones cannot fill 256 CUs on their own
struct Work {
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    DevBuf T, Cn, mask, fwd, nsim, state, strong, weak, counters, cnt_lines, work_q, pixcov, sum, cnt, gscratch, dep, tmp_lo, border, ratio_stats; // grow-only
    DevBuf lay_pixcov, lay_sum, lay_tmp_lo; // extra colour layers (bcd_hip_denoise_layers): per-pixel covariances, sums, merge scratch -- one slice per layer
    DevBuf gate_mask, gate_nsim;   // the feature masks and their counts of a guided selection (guide_gate), ANDed into `mask` / `nsim`
    int border_capacity = 0;       // entries of `border` offered to the last fast similarity pass (0: the exact kernels ran)
    int rounds_hint = 0;           // marking launches the last problem needed
    int last_batch = 0;            // launches of the batch active_step_enqueue left in flight
    bool dep_ready = false;        // dependency lists of the current marking problem are in `dep` (reset by active_init)
    const void *dep_mask = nullptr, *dep_state = nullptr; // ... extracted for these buffers (another problem on the same context rebuilds them)
    Counters *h_counters = nullptr; // pinned
    Counters *d_counters() const { return static_cast<Counters *>(counters.p); } // (after ensure(ctx, wk.counters, sizeof(Counters)))
    bool initialised = false;      // set once every stream / event / pinned buffer below exists
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool; // pair-distance kernel timing
    int ev_used = 0;
    hipEvent_t ev_stage[4] = { nullptr, nullptr, nullptr, nullptr };
    hipEvent_t ev_done = nullptr;
    hipEvent_t ev_built = nullptr; // this scale's pyramid level is complete
    hipStream_t aux = nullptr;     // side stream: the fallback-pixel kernel runs beside the (latency-bound) full estimate kernel
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_pixcov = nullptr; // the per-pixel covariances (side stream, beside the distance kernel) are complete
    hipEvent_t ev_counts = nullptr; // the list lengths of bayes() are on the host
    // (round 6) full-estimate items of the last frame of this geometry on this workspace: the next frame's first chunk of estimate kernels is launched for
    // that many (+ 1/8) BEFORE the host knows the new count
    int strong_hint = 0, strong_hint_W = 0, strong_hint_H = 0;
    // approximate distance planes computed ahead of similarity() by a caller that streams the frame in (bcd_hip_denoise_host_ex): valid for
    // exactly this problem; similarity() consumes the note
    struct { bool ready = false; const float *hist = nullptr, *ns = nullptr; int W = 0, H = 0, D = 0, b = 0; float tau = 0.f, uni_n = 0.f; bool ratio = false; /* by the RATIO form */ bool margin = false; /* one margin plane for this tau */ } planes;
    // uniform-sample-count speculation of the approximate distance kernel (similarity()): did the last frames on this workspace fail it?
    bool nonuniform = false;
    bool speculated = false;       // the current pass launched the uniform kernel on the first pixel's count, unchecked by the host
    // the RATIO form of the distance kernel raised its absolute-error flag on frames of these sizes on this workspace: the reference's operations serve them (a small
    // set, oldest replaced: serialised scales share one workspace, a caller may alternate frame sizes)
    struct { int W = 0, H = 0; } ratio_declined[4];
    int ratio_declined_next = 0;
    bool ratio_is_declined(int W, int H) const { for (const auto &k : ratio_declined) if (k.W == W && k.H == H) return true; return false; }
    bool ratio_used = false;          // the current pass ran the RATIO form of the distance kernel (general sample counts)
    int ratio_W = 0, ratio_H = 0;        // ... on a frame of this size
    // (round 4) k_scale_begin cleared these at the head of the scale's stream: the first user takes them as they are, a repeated use (second
    // similarity attempt, second marking batch, second chunk of a long list) clears its own as before
    bool clean_flags = false, clean_lines = false, clean_dc = false, clean_wq = false;
    // the redo kernel of the register-resident finish (k_bayes27w<2> over the -- normally empty -- list of items whose sweep inverse failed its
    // checks) is only launched when the list's counter, read with the scale's last synchronisation, says so
    struct { bool pending = false; int first = 0, n = 0, cus = 0; } redo;
};

struct bcd_hip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    bool profiling = false;
    bool concurrent_scales = true;
    bool fast_similarity = true; // approximate distance planes + exact re-evaluation at the threshold (k_similarity_fast.hip)
    bool margin_planes = true;   // ... as one signed margin plane E = T - tau C (k_similarity.hip); false (BCD_HIP_TC_PLANES=1): the T and C planes
    int num_cus = 256;
    int cu_share_pct = 100;  // bcd_hip_set_cu_share
    // share of the CU slots the coarse scales' persistent estimate kernels take inside bcd_hip_denoise (bayes()); adjusted from call to
    // call on the same geometry so that the coarse scales end shortly before the finest one (see bcd_hip_denoise)
    int coarse_share = 25;
    int64_t share_key = 0;          // geometry the current value was tuned on
    std::mutex err_mutex;
    std::string err;
    bcd_hip_scale_stats stats[MAX_SCALES];
    Work main;               // bound to `stream`
    Work extra[MAX_SCALES];  // lazily created streams for scales 1.. of a multiscale run
    DevBuf tmp_lo;
    DevBuf pyr[MAX_SCALES][5]; // colours, nsamples, hist, cov, out
    DevBuf lay_host[3];            // host-buffer entry point of the layers: device copies of the extra layers' colours, covariances, outputs
    DevBuf lay_host_f[2];          // ... and, when the spike prefilter covers them, the second set of slices: their colours and covariances gathered through the map
    DevBuf spike_map;              // the source map of the spike prefilter (bcd_hip_spike_filter_layers without a map of the caller's, the host-buffer layers): W*H int32
    // the in-place gather (spike_gather_inplace): the moved count and the list cursor (two int32), the (destination, source) pairs, the staged source values
    DevBuf spike_count, spike_list, spike_stage;
    DevBuf lay_pyr[MAX_SCALES][3]; // extra colour layers: colours, cov, out of every layer at that pyramid level, one slice per layer
    int32_t layer_spectral[MAX_SCALES][BCD_MAX_LAYERS]; // per scale and layer of the last layered call: full estimates that took the spectral inverse
    int layer_count = 0;                                // layers of that call (0: none yet)
    bcd_hip_selection *keep = nullptr;                  // bcd_hip_denoise_layers_keep in progress: every scale leaves its selection here (mono_accumulate)
    // bcd_hip_denoise_moments in progress: every scale selects from its guide's colours and per-pixel covariances (similarity_moments); no histogram is read
    struct { bool on = false; float var_floor = 0.f; } moments;
    // bcd_hip_denoise_guided in progress: every scale gates its selection with the masks of its level of the feature pyramid (guide_gate)
    struct {
        bool on = false;
        int F = 0;
        const float *f[MAX_SCALES] = {}, *v[MAX_SCALES] = {}; // per pyramid level: features, variances (null: none)
        float floors[BCD_GUIDE_MAX_CHANNELS] = {};
        float tau = 0.f;
    } guide;
    DevBuf guide_pyr[MAX_SCALES][2]; // levels 1.. of the features and their variances
    DevBuf guide_host[2];            // host-buffer entry point: device copies of the features and their variances
    // bcd_hip_denoise_temporal (bcd_temporal.hip): frame 0 is the frame itself, 1.. its neighbours.  Grow-only, like every buffer here
    struct {
        DevBuf pyr[BCD_MAX_NEIGHBOURS + 1][MAX_SCALES][4]; // levels 1.. of every frame: colours, sample counts, histograms, covariances
        DevBuf out[MAX_SCALES];                            // the outputs of the levels 1..
        DevBuf pixcov[BCD_MAX_NEIGHBOURS + 1];             // per-pixel covariances of every frame at the scale in progress
        DevBuf mask[BCD_MAX_NEIGHBOURS + 1];               // [1..]: the cross masks of the scale in progress
        DevBuf count_nb;                                   // |S_f| of the neighbour in progress
        DevBuf host[BCD_MAX_NEIGHBOURS + 1][4], host_out;  // host-buffer entry point: device copies
        // bcd_hip_denoise_temporal_layers (bcd_temporal_layers.hip): the colour layers of every frame, one slice per layer in each buffer.  The sample counts
        // and histograms of the levels 1.. are pyr[f][s][1] and [2] above
        DevBuf lay_pyr[BCD_MAX_NEIGHBOURS + 1][MAX_SCALES][2]; // levels 1.. of every frame: colours, covariances of its layers
        DevBuf lay_out[MAX_SCALES];                            // the layers' outputs of the levels 1..
        DevBuf lay_pixcov[BCD_MAX_NEIGHBOURS + 1];             // per-pixel covariances of every frame's layers at the scale in progress
        DevBuf lay_sum, lay_tmp_lo;                            // the layers' sums of the scale in progress, the merge's scratch
        DevBuf lay_host[BCD_MAX_NEIGHBOURS + 1][2], lay_host_out; // host-buffer entry point: device copies of the layers' colours, covariances, outputs
        // the motion calls ("Motion"): a neighbour with a motion field is warped at full resolution before its pyramid is built
        DevBuf warp[BCD_MAX_NEIGHBOURS + 1][4];                // [1..]: the warped colours, sample counts, histograms, covariances of that neighbour
        DevBuf lay_warp[BCD_MAX_NEIGHBOURS + 1][2];            // [1..]: the warped colours, covariances of its layers, one slice per layer
        DevBuf valid[BCD_MAX_NEIGHBOURS + 1][MAX_SCALES];      // [1..]: its validity bytes at every level
        DevBuf pvalid;                                         // patch validity of the neighbour and scale in progress
        DevBuf motion_host[BCD_MAX_NEIGHBOURS + 1];            // host-buffer entry points: device copies of the motion fields
        // bcd_hip_denoise_temporal_guided ("Features"): [..][0] features, [..][1] their variances; frame 0's levels 1.. are ctx->guide_pyr
        DevBuf guide_pyr[BCD_MAX_NEIGHBOURS + 1][MAX_SCALES][2]; // [1..]: levels 1.. of every neighbour's feature images
        DevBuf guide_warp[BCD_MAX_NEIGHBOURS + 1][2];            // [1..]: the warped feature images of a neighbour that has a motion field
        DevBuf guide_host[BCD_MAX_NEIGHBOURS + 1][2];            // host-buffer entry point: device copies of every frame's feature images
        // the call in progress: per frame and pyramid level the feature and variance images (v null: none); F, floors and threshold are ctx->guide's.
        // temporal_select gates the in-frame and the cross masks of a scale when `on`
        struct {
            bool on = false;
            const float *f[BCD_MAX_NEIGHBOURS + 1][MAX_SCALES] = {}, *v[BCD_MAX_NEIGHBOURS + 1][MAX_SCALES] = {};
        } guide;
        // bcd_hip_denoise_temporal_host_ex in progress with a factor ("Prefilter"): the host calls filter every frame's uploaded copies in place behind their uploads
        float prefilter = 0.f;
        int64_t guide_cross_passes = 0; // cross feature passes launched so far (temporal_guide_gate: one per gated neighbour and scale); a sequence reports its share
    } temporal;
    DevBuf host_stage[9];      // host-buffer entry points: device copies of the four inputs, the output, the prefiltered inputs (grow-only)
    hipEvent_t ev_pyramid = nullptr;
    hipStream_t upload_stream = nullptr;        // host-buffer entry points: uploads run beside the kernels of the lines that have arrived
    hipStream_t upload_stream2 = nullptr;       // ... colours and covariances beside the histogram pieces (helper thread)
    hipEvent_t ev_upload2 = nullptr;
    std::vector<hipEvent_t> ev_upload;
    bool stream_uploads = true;                 // BCD_HIP_STREAM_UPLOADS=0: upload everything, then compute
    // (round 4) the histogram image crosses PCIe without its zeros (bcd_sparse_upload.hip); BCD_HIP_SPARSE_UPLOAD=0: plain copies
    bool sparse_uploads = true;
    BcdSparseUploader *sparse = nullptr;
    long long upload_raw_bytes = 0, upload_sent_bytes = 0; // histogram image of the last host-buffer frame: as it is / as it travelled
    // progress reporting (IDenoiser::setProgressCallback; Denoiser.cpp:181-192 of the reference): every scale adds its share when
    // its marking is done and when its estimate is done; calls are serialised and monotone
    bcd_hip_progress_fn progress_fn = nullptr;
    void *progress_user = nullptr;
    std::mutex progress_mutex;
    double progress_done = 0.0, progress_total = 0.0;
    // bcd_hip_denoise_begin / _wait (round 6): one frame of this context in flight on a worker thread of its own, so that a caller can keep a second
    // context busy meanwhile (frames of a sequence, AOV passes: the distance kernels of one frame fill the chip under the latency-bound tail of another)
    struct Async {
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        bool has_job = false, in_flight = false, quit = false;
        int rc = 0;
        const float *col = nullptr, *ns = nullptr, *hist = nullptr, *cov = nullptr;
        float *out = nullptr;
        int W = 0, H = 0, D = 0, S = 0;
        bcd_hip_params prm;
    } async;
};

// ---- helpers shared between the host files: not part of the dynamic symbol table
#pragma GCC visibility push(hidden)

void set_err(bcd_hip_ctx *ctx, const std::string &msg); // (bcd_api.hip)

// every entry point that allocates or launches runs on the context's device and leaves the caller's current device as it was
struct DeviceGuard {
    int prev = -1, dev;
    bool ok = true;
    explicit DeviceGuard(const bcd_hip_ctx *ctx) : dev(ctx ? ctx->device : -1)
    {
        if (dev < 0) return;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (dev >= 0 && prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
};
#define DEVICE_GUARD(ctx)                                                                                             \
    DeviceGuard guard__(ctx);                                                                                         \
    if (!guard__.ok) { set_err((ctx), "hipSetDevice failed"); return BCD_HIP_EDEVICE; }

#define HIPCHK(ctx, expr)                                                                                             \
    do {                                                                                                              \
        hipError_t e__ = (expr);                                                                                      \
        if (e__ != hipSuccess) {                                                                                      \
            set_err((ctx), std::string(#expr) + ": " + hipGetErrorString(e__));                                       \
            return BCD_HIP_EDEVICE;                                                                                   \
        }                                                                                                             \
    } while (0)

#define RCCHK(expr)                                                                                                   \
    do {                                                                                                              \
        int rc__ = (expr);                                                                                            \
        if (rc__ != BCD_HIP_OK) return rc__;                                                                          \
    } while (0)

// ---- defined in bcd_api.hip
int ensure(bcd_hip_ctx *ctx, DevBuf &b, size_t bytes);
int bad(bcd_hip_ctx *ctx, const char *msg);
int check_params(bcd_hip_ctx *ctx, int W, int H, int D, const bcd_hip_params *prm);
bool fast_similarity_applies(const bcd_hip_ctx *ctx, int D, int w, float tau);
int scan_uniform_count(bcd_hip_ctx *ctx, Work &wk, const float *d_ns, size_t npix, float *uni_n);
float stage_ms(Work &wk, int a, int b);
int denoise_impl(bcd_hip_ctx *ctx, const float *d_colors, const float *d_ns, const float *d_hist, const float *d_cov, int W, int H, int D, int nb_scales,
                 const bcd_hip_params *prm, float *d_out, const LayerView *lv0);
int work_init(bcd_hip_ctx *ctx, Work &w, hipStream_t stream);
int fork_aux(bcd_hip_ctx *ctx, Work &wk); // the side stream waits for what the workspace's stream holds so far
int check_layers_call(bcd_hip_ctx *ctx, const float *d_ns, const float *d_hist, int W, int H, int D, int nb_scales, const bcd_hip_params *prm, const bcd_hip_layer *layers,
                      int nb_layers, bool no_hist = false);
int denoise_layers_checked(bcd_hip_ctx *ctx, const float *d_ns, const float *d_hist, int W, int H, int D, int nb_scales, const bcd_hip_params *prm,
                           const bcd_hip_layer *layers, int nb_layers);
int layers_follow(bcd_hip_ctx *ctx, Work &wk, const LayerView &lv, const uint32_t *d_mask, const int32_t *d_nsim, const uint8_t *d_state, const float *const *pixcov,
                  float *const *sum, int W, int H, int w, int b, float min_eig, const int32_t *d_count, int32_t *spectral, const KeptLists *kept = nullptr);
int build_level_layers(bcd_hip_ctx *ctx, const LayerView &fine, const LayerView &coarse, const float *ns_fine, int W, int H, hipStream_t st);
int merge_layers_on(bcd_hip_ctx *ctx, Work &wk, DevBuf &scratch, const LayerView &hi, int W, int H, const LayerView &lo); // (scratch: grown to one reduced slice per layer)
// the guide of a bcd_hip_denoise_guided call: its refusals (no device work), then -- on the context's stream -- its pyramid and ctx->guide; guide_end switches it off
int check_guide(bcd_hip_ctx *ctx, const bcd_hip_guide *g, int search_radius);
int guide_begin(bcd_hip_ctx *ctx, const bcd_hip_guide *g, const float *d_features, const float *d_variances, int W, int H, int nb_scales);
inline void guide_end(bcd_hip_ctx *ctx) { ctx->guide.on = false; }
// one level of a feature pyramid from the W x H level above it (guide_begin, temporal_guide_begin, the push of a sequence): the features averaged, the
// variances (d_var null: none) averaged and multiplied by 0.25f
int guide_build_level(bcd_hip_ctx *ctx, const float *d_feat, const float *d_var, int W, int H, int F, float *d_feat_out, float *d_var_out, hipStream_t st);
// the gate of a guided selection with ctx->guide's channels, floors and threshold, behind a selection pass on wk.stream: the feature masks of (d_features,
// d_variances) into wk.gate_mask / wk.gate_nsim, then d_mask &= them and d_count = the bits that remain (the code path of a guided scale)
int guide_gate_masks(bcd_hip_ctx *ctx, Work &wk, const float *d_features, const float *d_variances, int W, int H, int w, int b, uint32_t *d_mask, int32_t *d_count);
// an event pair for the distance kernel of a pass outside bcd_api.hip (bcd_hip_kernel_time); both null once the pool is used up
int distance_timing_events(bcd_hip_ctx *ctx, Work &wk, hipEvent_t *e0, hipEvent_t *e1);
// similarity_moments for a caller outside bcd_api.hip: the in-frame masks and counts of the moment selection on wk.stream (d_pixcov complete on that stream)
int moments_masks(bcd_hip_ctx *ctx, Work &wk, const float *d_colors, const float *d_pixcov, int W, int H, int w, int b, float tau, float var_floor, uint32_t *d_mask,
                  int32_t *d_count);

// every DevBuf of an array of them, of any shape, freed and emptied: free_bufs(a, sizeof a)
inline void free_bufs(void *first, size_t bytes)
{
    DevBuf *b = static_cast<DevBuf *>(first);
    for (size_t i = 0; i < bytes / sizeof(DevBuf); ++i) {
        if (b[i].p) (void)hipFree(b[i].p);
        b[i] = DevBuf();
    }
}

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?  The one overlap predicate of the argument checks
inline bool bytes_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na, b0 = (uintptr_t)b, b1 = b0 + nb;
    return a0 < b1 && b0 < a1;
}

// ---- defined in bcd_temporal.hip: what the frame calls, the layered calls (bcd_temporal_layers.hip) and the sequence (bcd_sequence.hip) share
void temporal_free(bcd_hip_ctx *ctx); // (bcd_hip_ctx_destroy)
// does [out, out + bytes) overlap one of a frame's images (a null image: not looked at)?
bool overlaps_frame_images(const void *out, size_t bytes, const void *col, const void *ns, const void *hist, const void *cov, size_t npix, int D);
// what the selection of a scale reads of one frame: sample counts and histograms at this level; valid: null, or the validity bytes of a warped neighbour
// feat, var: null, or -- in a bcd_hip_denoise_temporal_guided call -- the frame's feature and variance images at this level (var null: no variances)
// col, pixcov: null, or -- in a bcd_hip_denoise_temporal_moments call ("Moments") -- the guide layer's colours and per-pixel covariances at this level; hist is
// null then.  pixcov is what per_pixel_cov() produces: temporal_select enqueues it ahead of the in-frame pass in that mode
// transpose_from, mask_dst: null, or -- in a pop of a sequence (bcd_sequence.hip, "Sequences") -- the kept cross masks of the pair with the roles swapped, from
// which this neighbour's masks come by k_masks_transpose in place of a cross pass, and the buffer that takes this neighbour's masks in place of
// ctx->temporal.mask[f] (the sequence keeps them there).  With both null every call takes the branches it took before they existed.  In guide mode the kept
// masks are the gated ones, so a neighbour with transpose_from passes no feature gate (the transposition distributes over the AND, which is idempotent)
struct TemporalSelFrame {
    const float *ns, *hist; const uint8_t *valid; const float *feat = nullptr, *var = nullptr; const float *col = nullptr, *pixcov = nullptr;
    const uint32_t *transpose_from = nullptr; uint32_t *mask_dst = nullptr;
};
// with a guided temporal call in progress (temporal_guide_begin), the feature images of frame f at level `scale`; else nothing
inline void temporal_guide_level(const bcd_hip_ctx *ctx, int f, int scale, TemporalSelFrame *sel)
{
    const auto &g = ctx->temporal.guide;
    if (g.on) { sel->feat = g.f[f][scale]; sel->var = g.v[f][scale]; }
}
struct TemporalPath { int32_t path = 0, borderline = 0; }; // of the in-frame pass (bcd_hip_similarity_last_path)
// The selection stage of one scale, frames[0] the frame itself, from stage event 0 to stage event 2: the stats header of ctx->stats[scale], the in-frame masks
// (wk.mask, wk.nsim) by bcd_hip_similarity_masks, per neighbour f the cross planes, k_masks_cross into ctx->temporal.mask[f], the gate of a warped neighbour and
// the count sum, then the marking (wk.state).  per_pixel_cov() enqueues the caller's per-pixel covariances between stage events 0 and 1.
// Guide mode (frames[0].feat given, "Features"): the in-frame masks pass guide_gate_masks behind bcd_hip_similarity_masks, and every neighbour's cross masks
// are ANDed with its cross feature mask (k_pairdist_guide_cross into the plane buffers, k_masks_cross with tau_g into wk.gate_mask) ahead of the count sum.
// Moments mode (ctx->moments.on, "Moments"): per_pixel_cov() comes first, the in-frame masks come from similarity_moments on frames[0].col / .pixcov (path 3)
// and every cross pass from the moment cross launchers on frames[f].col / .pixcov; no histogram is read.
int temporal_select(bcd_hip_ctx *ctx, const TemporalSelFrame *frames, int nf, int W, int H, int D, const bcd_hip_params *prm, int scale,
                    const std::function<int()> &per_pixel_cov, TemporalPath *path);
// the estimate stage over the members of several frames (patch radius 1, search radius 6) on wk.stream, synchronised at its end: temporal_lists, the fallback
// kernel over all frames, one chain of full estimates on the frame's own colours and in-frame masks; the list lengths and the sum of |S| are in
// wk.h_counters->lists when it returns
int bayes_temporal(bcd_hip_ctx *ctx, Work &wk, const BcdFrameTable &t, const int32_t *d_nsim_total, const uint8_t *d_state, int W, int H, int b, float min_eig,
                   float *d_sum, int32_t *d_count);
// ---- defined in bcd_temporal_layers.hip: the layered estimate stage, shared with the pops of a sequence (bcd_sequence.hip)
// one scale's estimate inputs: [f][k] = frame f (0: the frame itself), layer k
struct LayerFrames {
    int nf = 0, L = 0;
    const float *col[BCD_MAX_NEIGHBOURS + 1][BCD_MAX_LAYERS], *pixcov[BCD_MAX_NEIGHBOURS + 1][BCD_MAX_LAYERS];
    const uint32_t *mask[BCD_MAX_NEIGHBOURS + 1];
};
// bayes_temporal for L layers on one selection (see its definition); redo[k]: the items of layer k that took the redo list
int bayes_temporal_layers(bcd_hip_ctx *ctx, Work &wk, const LayerFrames &lf, const int32_t *d_nsim_total, const uint8_t *d_state, int W, int H, int b, float min_eig,
                          float *const *d_sum, int32_t *d_count, int32_t *redo);
// the tail of a scale (the stream is synchronised): the figures of wk.h_counters->lists and of the in-frame pass, and with profiling the four timers
void temporal_stats_tail(bcd_hip_ctx *ctx, int scale, const TemporalPath &path);
// The refusals a call with neighbour frames makes of its geometry, in this order: the scale count, the temporal radius of a sequence (sequence_radius null: a
// frame call), with neighbours the patch and search radius, the image size against the scale count
int check_temporal_geometry(bcd_hip_ctx *ctx, int W, int H, int nb_scales, const bcd_hip_params *prm, bool neighbours, const int *sequence_radius);
// one frame at one pyramid level, as temporal_build_level and temporal_scale see it
struct TemporalFrame {
    TemporalSelFrame sel = { nullptr, nullptr, nullptr }; // by the caller: ns, hist (null: "Moments"), valid, feat, var, transpose_from, mask_dst (temporal_scale adds col, pixcov)
    const float *col[BCD_MAX_LAYERS] = {}, *cov[BCD_MAX_LAYERS] = {}; // the colours and covariances of its layers
    float *pixcov = nullptr; // the per-pixel covariances of its layers, one slice per layer: temporal_scale computes them from cov, or a sequence's push has
};
// Level s of a frame from its W x H level s - 1, on st: sample counts and histograms summed (hist null: none), the colours averaged and the covariances
// weighted by the counts -- of one layer by the reducers of bcd_hip_denoise (its colours first), of a layered estimate by build_level_layers.  `coarse`
// holds the destinations
int temporal_build_level(bcd_hip_ctx *ctx, const TemporalFrame &fine, const TemporalFrame &coarse, int L, bool layered, int W, int H, int D, hipStream_t st);
// one scale of a call with neighbour frames, as its caller tabulates it
struct TemporalScale {
    int nf = 0, L = 1;
    bool layered = false;       // the estimate of bayes_temporal_layers (L > 1, or "Moments"), else bayes_temporal on one layer of histograms
    bool pixcov_ready = false;  // the frames' per-pixel covariances are complete (the pushes of a sequence), else they are computed from fr[f].cov
    TemporalFrame fr[BCD_MAX_NEIGHBOURS + 1]; // [0]: the frame itself
    float *sum = nullptr;       // the sums, one slice per layer
    float *out[BCD_MAX_LAYERS] = {};
    uint32_t *self_copy = nullptr; // null, or what takes a copy of the in-frame masks (self[s] of a sequence)
};
// The one scale stage: temporal_select, the cleared accumulators, the estimate and finalisation of the kind sc.layered names, temporal_stats_tail and, layered,
// ctx->layer_spectral[scale].  A neighbour's masks are in sc.fr[f].sel.mask_dst, or in ctx->temporal.mask[f] where that is null
int temporal_scale(bcd_hip_ctx *ctx, const TemporalScale &sc, int W, int H, int D, const bcd_hip_params *prm, int scale);
// The lists of an estimate over several frames on wk.stream: the buffers, the cleared counters, k_active_lists on the states and the TOTAL |S|, the copy of the list
// lengths and the sum of |S| to wk.h_counters->lists (not waited for).  -> the CU slots of the chain, the grid of the fallback kernel
struct TemporalLists { int cus, weak_grid; };
int temporal_lists(bcd_hip_ctx *ctx, Work &wk, const int32_t *d_nsim_total, const uint8_t *d_state, int64_t npix, TemporalLists *out);
// The full estimates of one image over wk.strong[0 .. n_strong): per chunk of ESTIMATE_CHUNK records the work-queue clear, the temporal prepare kernel on every
// frame of `t`, then the solver and finish kernels on t's frame 0 into d_sum (and d_count, unless null: a further layer).  The redo counter runs on.
int temporal_full_chain(bcd_hip_ctx *ctx, Work &wk, const BcdFrameTable &t, float *d_sum, int32_t *d_count, int n_strong, int cus, int W, int H, int b, float min_eig);
// The motion set-up of neighbour f (1..) that has a field: its four images warped into ctx->temporal.warp[f] (-> warped: colours, sample counts, histograms,
// covariances) with the validity bytes of level 0, `more` (null: none) further layers by k_warp_layers, the validity levels 1 .. S - 1, and column f of the table
// valid[s * nf + f]
int temporal_warp_neighbour(bcd_hip_ctx *ctx, int f, int nf, const float *col, const float *ns, const float *hist, const float *cov, const float *motion, int W, int H,
                            int D, int S, const BcdWarpLayerTable *more, int nb_more, const uint8_t **valid, const float *warped[4]);
inline bool any_field(const float *const *motion, int n)
{
    for (int f = 0; motion && f < n; ++f) if (motion[f]) return true;
    return false;
}
int temporal_upload_motion(bcd_hip_ctx *ctx, const float *const *h_motion, int nb_neighbours, int W, int H, const float **dev); // (whole uploads; dev[f] NULL for a NULL field)
// the refusals the motion calls add: the list itself, and a field that overlaps one of `outs` (each W*H*3 floats)
int check_motion_list(bcd_hip_ctx *ctx, const float *const *motion, int nb_neighbours, int W, int H, float *const *outs, int nb_outs);
// "Features": the set-up of a guided temporal call on the main stream, every pointer a device pointer: ctx->guide's channels, floors and threshold and the
// frame's feature pyramid (guide_begin; ctx->guide.on stays false), per neighbour the warp of its feature images when it has a motion field (k_warp_features,
// which writes the validity bytes temporal_warp_neighbour writes again), its pyramid by guide_begin's rule, and ctx->temporal.guide.  temporal_guide_end
// switches the mode off
int temporal_guide_begin(bcd_hip_ctx *ctx, const bcd_hip_guide *g, const bcd_hip_guide_images *nb, int nb_neighbours, const float *const *motion, int W, int H, int nb_scales);
inline void temporal_guide_end(bcd_hip_ctx *ctx) { ctx->temporal.guide.on = false; }

// ---- defined in bcd_spike.hip: the spike prefilter in place ("In place"), on ctx->stream; each synchronises once, for the moved count
// (h_moved: null, or where it goes).  Neither checks an argument: the public entry points and the animation paths have
// the in-place gather of t's n images through d_map
int spike_gather_inplace(bcd_hip_ctx *ctx, const int32_t *d_map, size_t npix, BcdSpikeInplaceTable &t, int n, int32_t *h_moved);
// one resident frame: the map of d_col[0] into d_map (null: ctx->spike_map), then the sample counts, the histograms (null: none) and the L layers gathered
int spike_filter_frame_inplace(bcd_hip_ctx *ctx, float *d_ns, float *d_hist, int W, int H, int D, float factor, float *const *d_col, float *const *d_cov, int L,
                               int32_t *d_map, int32_t *h_moved);

// ---- defined in bcd_selection.hip
// one scale of a bcd_hip_denoise_layers_keep call, at the end of its chain (the stream is synchronised, wk.h_counters->lists holds the list lengths, `st` is
// filled): device-to-device copies on the scale's stream into ctx->keep
int selection_store(bcd_hip_ctx *ctx, Work &wk, int scale, const float *d_ns, int W, int H, int b, const int32_t *d_count, const bcd_hip_scale_stats &st);

// ---- defined in bcd_host.hip (shared with the self-tests of the upload path in bcd_selftest.hip)
struct HostStreamProgress {
    int chunk_lines = 0, chunks = 0;           // lines per row chunk, chunks uploaded and scheduled
    int rows_filtered = 0, tile_rows_done = 0; // prefiltered lines [0, rows_filtered) (0 without the prefilter), plane tile rows [0, tile_rows_done)
    float uni_n = 0.f;                         // the uniform sample count the planes were launched for (0: general sample counts)
    bool ratio = false;                        // general sample counts by the RATIO form of the kernel (as similarity() would choose), else the reference's operations
    bool margin = false;                       // the planes are margin planes for the call's threshold
};
int host_upload_stream(bcd_hip_ctx *ctx);
int host_sparse_uploader(bcd_hip_ctx *ctx);
int host_stream_frame(bcd_hip_ctx *ctx, const float *const h_src[4], float *const d[9], int W, int H, int D, int b, float tau, bool prefilter, float spike_factor,
                      int stop_after_chunks, bool poison, HostStreamProgress *out, bool margin);
// does bcd_hip_denoise_host_ex stream a frame of this geometry in (row chunks, planes ahead of the last chunk)?
inline bool host_frame_streams(const bcd_hip_ctx *ctx, int H, int D, const bcd_hip_params *prm)
{
    return ctx->stream_uploads && fast_similarity_applies(ctx, D, prm->patch_radius, prm->hist_dist_threshold) && H >= 256;
}

// bytes of the count planes of a scale.  ONE place: the host-buffer entry point computes planes ahead of similarity(), and a larger request there
// would free them (round 6: it happened when one of the two grew, found by the environment-switch test on a fresh context)
inline size_t count_plane_bytes(size_t npix, int nd) { return npix * (size_t)nd; }
// ... and of its binary16 planes (the approximate T plane, or the margin plane, which has no count plane beside it)
inline size_t half_plane_bytes(size_t npix, int nd) { return npix * (size_t)nd * 2; }

// a user of the workspace's counters / flags / work queues / sub-counter lines outside the scale chain (self-tests, the eigensolver entry point): whatever
// k_scale_begin left clean is not clean any more
inline void touch(Work &wk) { wk.clean_flags = wk.clean_lines = wk.clean_dc = wk.clean_wq = false; }

// a sample count the uniform form of the distance kernels serves: a power of two in [1, 65536] (k_pairdist drops the sample-count products exactly)
inline bool is_pow2_sample_count(float n)
{
    int e = 0;
    return n >= 1.f && n <= 65536.f && frexpf(n, &e) == 0.5f;
}

#pragma GCC visibility pop
