// bcd_selftest.hip -- self-tests and measurement entry points of the C ABI (bcd_hip_selftest_*, bcd_hip_eig27_batch*): they run single kernels of the
// chain on the context's main workspace, outside the scale drivers of bcd_api.hip.
#include "bcd_ctx.h"
#include "bayes27_record.h"

#include <algorithm>
#include <cstring>

namespace {

// a device allocation that lives as long as its scope
struct DevAlloc {
    void *p = nullptr;
    DevAlloc() = default;
    DevAlloc(const DevAlloc &) = delete;
    DevAlloc &operator=(const DevAlloc &) = delete;
    ~DevAlloc() { if (p) (void)hipFree(p); }
};

} // namespace

extern "C" {

int bcd_hip_selftest_distance_kernels(bcd_hip_ctx *ctx, const float *d_hist, const float *d_ns, int W, int H, int D, int search_radius,
                                      int *variant, int64_t *mismatches)
{
    if (!ctx || !d_hist || !d_ns || !mismatches || W <= 0 || H <= 0 || D <= 0 || search_radius < 1) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    touch(ctx->main);
    Work &wk = ctx->main;
    const size_t npix = (size_t)W * H;
    const int nd = bcd_delta_count(search_radius);
    RCCHK(ensure(ctx, wk.T, npix * nd * sizeof(float)));
    RCCHK(ensure(ctx, wk.Cn, count_plane_bytes(npix, nd)));
    RCCHK(ensure(ctx, wk.counters, sizeof(Counters)));
    DevAlloc T2, C2;
    HIPCHK(ctx, hipMalloc(&T2.p, npix * nd * sizeof(float)));
    if (hipMalloc(&C2.p, npix * nd) != hipSuccess) { set_err(ctx, "hipMalloc"); return BCD_HIP_EDEVICE; }
    auto run = [&]() -> int {
        Counters::Flags *d_flag = &wk.d_counters()->flags;
        unsigned long long *d_cnt = &wk.d_counters()->selftest.result;
        HIPCHK(ctx, hipMemsetAsync(&d_flag->range, 0, 2 * sizeof(int), wk.stream)); // (range and scan)
        HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, sizeof(*d_cnt), wk.stream));
        float uni_n = 0.f;
        RCCHK(scan_uniform_count(ctx, wk, d_ns, npix, &uni_n));
        // (entries whose neighbour lies outside the image are never written: clear both sets first)
        HIPCHK(ctx, hipMemsetAsync(wk.T.p, 0, npix * nd * sizeof(float), wk.stream));
        HIPCHK(ctx, hipMemsetAsync(wk.Cn.p, 0, npix * nd, wk.stream));
        HIPCHK(ctx, hipMemsetAsync(T2.p, 0, npix * nd * sizeof(float), wk.stream));
        HIPCHK(ctx, hipMemsetAsync(C2.p, 0, npix * nd, wk.stream));
        // production choice (fast division, uniform-count formula when it applies) against the compiler's division + general formula
        HIPCHK(ctx, bcd_launch_pairdist(d_hist, d_ns, W, H, D, search_radius, (float *)wk.T.p, (uint8_t *)wk.Cn.p, 1, &d_flag->range, uni_n, wk.stream));
        HIPCHK(ctx, bcd_launch_pairdist(d_hist, d_ns, W, H, D, search_radius, (float *)T2.p, (uint8_t *)C2.p, 0, &d_flag->range, 0.f, wk.stream));
        HIPCHK(ctx, bcd_launch_compare_planes((const float *)wk.T.p, (const uint8_t *)wk.Cn.p, (const float *)T2.p, (const uint8_t *)C2.p, (int64_t)(npix * nd), d_cnt, wk.stream));
        unsigned long long h = 0;
        int flag = 0;
        HIPCHK(ctx, hipMemcpyAsync(&h, d_cnt, sizeof(h), hipMemcpyDeviceToHost, wk.stream));
        HIPCHK(ctx, hipMemcpyAsync(&flag, &d_flag->range, sizeof(int), hipMemcpyDeviceToHost, wk.stream));
        HIPCHK(ctx, hipStreamSynchronize(wk.stream));
        *mismatches = (int64_t)h;
        if (variant) *variant = (uni_n > 0.f ? 2 : 1) | (flag << 4); // 1 = fast division, 2 = + uniform counts; bits 4.. = range / count flags raised
        return BCD_HIP_OK;
    };
    const int rc = run();
    if (rc != BCD_HIP_OK) set_err(ctx, "distance kernel self-test failed to run");
    return rc;
}

// Measurement (bench.py `roofline.valu`): what the production distance kernel computes on this frame -- the (pixel pair, bin) terms it
// evaluates (exactly the reference's count of bins with b1 + b2 > 1 over the half plane), the bins a wavefront issues because one of its 64
// pairs needs them, the groups of four bins it enters -- from a counting instantiation of the kernel, and the duration of the PRODUCTION
// instantiation on the same input (HIP events, best of `reps`).
int bcd_hip_selftest_bin_work(bcd_hip_ctx *ctx, const float *d_hist, const float *d_ns, int W, int H, int D, int search_radius, int reps,
                              int64_t *lane_bins, int64_t *wave_bins, int64_t *wave_groups, float *kernel_ms)
{
    if (!ctx || !d_hist || !d_ns || !lane_bins || !wave_bins || !wave_groups || !kernel_ms || W <= 0 || H <= 0 || search_radius < 1 || reps < 1) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    touch(ctx->main);
    if (!bcd_pairdist_rw_supported(D)) { set_err(ctx, "no approximate kernel for this histogram depth"); return BCD_HIP_EUNSUPPORTED; }
    Work &wk = ctx->main;
    const size_t npix = (size_t)W * H;
    const int nd = bcd_delta_count(search_radius);
    RCCHK(ensure(ctx, wk.T, npix * nd * sizeof(float)));
    RCCHK(ensure(ctx, wk.Cn, count_plane_bytes(npix, nd)));
    RCCHK(ensure(ctx, wk.counters, sizeof(Counters)));
    Counters::Flags *d_flag = &wk.d_counters()->flags;
    unsigned long long *d_work = wk.d_counters()->bin_work;
    HIPCHK(ctx, hipMemsetAsync(d_flag, 0, sizeof(*d_flag), wk.stream));
    HIPCHK(ctx, hipMemsetAsync(d_work, 0, 3 * sizeof(unsigned long long), wk.stream));
    // the uniform kernel on the first pixel's count if every pixel carries it (the kernel checks), else the general formula -- like similarity()
    float uni_n = -1.f;
    HIPCHK(ctx, bcd_launch_pairdist_rw_counting(d_hist, d_ns, W, H, D, search_radius, wk.T.p, (uint8_t *)wk.Cn.p, &d_flag->range, uni_n, d_work, wk.stream));
    Counters::Flags flags = {};
    HIPCHK(ctx, hipMemcpyAsync(&flags, d_flag, sizeof(flags), hipMemcpyDeviceToHost, wk.stream));
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    if (flags.other_count != 0) { // not one power-of-two count: count again with the general formula
        uni_n = 0.f;
        HIPCHK(ctx, hipMemsetAsync(d_flag, 0, sizeof(*d_flag), wk.stream));
        HIPCHK(ctx, hipMemsetAsync(d_work, 0, 3 * sizeof(unsigned long long), wk.stream));
        HIPCHK(ctx, bcd_launch_pairdist_rw_counting(d_hist, d_ns, W, H, D, search_radius, wk.T.p, (uint8_t *)wk.Cn.p, &d_flag->range, uni_n, d_work, wk.stream));
    }
    unsigned long long h[3] = { 0, 0, 0 };
    HIPCHK(ctx, hipMemcpyAsync(h, d_work, sizeof(h), hipMemcpyDeviceToHost, wk.stream));
    hipEvent_t e0, e1;
    HIPCHK(ctx, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); set_err(ctx, "hipEventCreate"); return BCD_HIP_EDEVICE; }
    float best = -1.f;
    int rc = BCD_HIP_OK;
    for (int r = 0; r < reps + 1 && rc == BCD_HIP_OK; ++r) { // (the first one warms up)
        if (hipEventRecord(e0, wk.stream) != hipSuccess ||
            bcd_launch_pairdist_rw(d_hist, d_ns, W, H, D, search_radius, wk.T.p, (uint8_t *)wk.Cn.p, &d_flag->range, uni_n, wk.stream) != hipSuccess ||
            hipEventRecord(e1, wk.stream) != hipSuccess || hipStreamSynchronize(wk.stream) != hipSuccess) { rc = BCD_HIP_EDEVICE; break; }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        if (r > 0 && (best < 0.f || ms < best)) best = ms;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc != BCD_HIP_OK) { set_err(ctx, "bin-work self-test failed to run"); return rc; }
    *lane_bins = (int64_t)h[0]; *wave_bins = (int64_t)h[1]; *wave_groups = (int64_t)h[2]; *kernel_ms = best;
    return BCD_HIP_OK;
}

int bcd_hip_selftest_approx_distance(bcd_hip_ctx *ctx, const float *d_hist, const float *d_ns, int W, int H, int D, int search_radius,
                                     float *max_rel_dev, int64_t *count_mismatches, int *flags)
{
    if (!ctx || !d_hist || !d_ns || !max_rel_dev || !count_mismatches || W <= 0 || H <= 0 || search_radius < 1) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    touch(ctx->main);
    if (!bcd_pairdist_rw_supported(D)) { set_err(ctx, "no approximate kernel for this histogram depth"); return BCD_HIP_EUNSUPPORTED; }
    Work &wk = ctx->main;
    const size_t npix = (size_t)W * H;
    const int nd = bcd_delta_count(search_radius);
    RCCHK(ensure(ctx, wk.T, npix * nd * sizeof(float)));
    RCCHK(ensure(ctx, wk.Cn, count_plane_bytes(npix, nd)));
    RCCHK(ensure(ctx, wk.counters, sizeof(Counters)));
    DevAlloc T2, C2;
    HIPCHK(ctx, hipMalloc(&T2.p, npix * nd * sizeof(float)));
    if (hipMalloc(&C2.p, npix * nd) != hipSuccess) { set_err(ctx, "hipMalloc"); return BCD_HIP_EDEVICE; }
    auto run = [&]() -> int {
        Counters::Flags *d_flag = &wk.d_counters()->flags;
        unsigned int *d_res = reinterpret_cast<unsigned int *>(&wk.d_counters()->selftest.result); // [0] largest relative deviation (float bits), [1] count mismatches
        HIPCHK(ctx, hipMemsetAsync(d_flag, 0, sizeof(*d_flag), wk.stream));
        HIPCHK(ctx, hipMemsetAsync(d_res, 0, 2 * sizeof(unsigned int), wk.stream));
        float uni_n = 0.f;
        RCCHK(scan_uniform_count(ctx, wk, d_ns, npix, &uni_n));
        HIPCHK(ctx, hipMemsetAsync(wk.T.p, 0, npix * nd * sizeof(float), wk.stream));
        HIPCHK(ctx, hipMemsetAsync(wk.Cn.p, 0, npix * nd, wk.stream));
        HIPCHK(ctx, hipMemsetAsync(T2.p, 0, npix * nd * sizeof(float), wk.stream));
        HIPCHK(ctx, hipMemsetAsync(C2.p, 0, npix * nd, wk.stream));
        // approximate planes (production variant: the uniform kernel, or -- general sample counts -- the RATIO form with its verdict in flag bit 2) against the
        // exact planes (compiler's division, general formula)
        if (uni_n == 0.f && ensure(ctx, wk.ratio_stats, 128 * sizeof(unsigned int)) != BCD_HIP_OK) return BCD_HIP_ENOMEM;
        if (uni_n != 0.f) HIPCHK(ctx, bcd_launch_pairdist_rw(d_hist, d_ns, W, H, D, search_radius, wk.T.p, (uint8_t *)wk.Cn.p, &d_flag->range, uni_n, wk.stream));
        else HIPCHK(ctx, bcd_launch_pairdist_rw_ratio(d_hist, d_ns, W, H, D, search_radius, wk.T.p, (uint8_t *)wk.Cn.p, &d_flag->range, 1.f, (unsigned int *)wk.ratio_stats.p, wk.stream));
        HIPCHK(ctx, bcd_launch_pairdist(d_hist, d_ns, W, H, D, search_radius, (float *)T2.p, (uint8_t *)C2.p, 0, &d_flag->range, 0.f, wk.stream));
        HIPCHK(ctx, bcd_launch_max_rel_dev((const float *)wk.T.p, (const float *)T2.p, (const uint8_t *)wk.Cn.p, (const uint8_t *)C2.p, W, H, search_radius, d_res, wk.stream));
        unsigned int h[2] = { 0u, 0u };
        int flag = 0;
        HIPCHK(ctx, hipMemcpyAsync(h, d_res, sizeof(h), hipMemcpyDeviceToHost, wk.stream));
        HIPCHK(ctx, hipMemcpyAsync(&flag, &d_flag->range, sizeof(int), hipMemcpyDeviceToHost, wk.stream));
        HIPCHK(ctx, hipStreamSynchronize(wk.stream));
        memcpy(max_rel_dev, &h[0], sizeof(float));
        *count_mismatches = (int64_t)h[1];
        if (flags) *flags = (uni_n > 0.f ? 2 : 3) | (flag << 4); // low nibble: 2 = uniform kernel, 3 = RATIO form; above: the kernels' flag word (4: the RATIO form declined)
        return BCD_HIP_OK;
    };
    const int rc = run();
    if (rc != BCD_HIP_OK) set_err(ctx, "approximate-distance self-test failed to run");
    return rc;
}

int bcd_hip_eig27_batch(bcd_hip_ctx *ctx, const float *d_A, int n, float *d_eig, float *d_V, float *ms)
{
    return bcd_hip_eig27_batch_rule(ctx, d_A, n, d_eig, d_V, ms, 0);
}

int bcd_hip_eig27_batch_rule(bcd_hip_ctx *ctx, const float *d_A, int n, float *d_eig, float *d_V, float *ms, int production_rule)
{
    if (!ctx || !d_A || !d_eig || !d_V || n <= 0) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    touch(ctx->main);
    Work &wk = ctx->main;
    RCCHK(ensure(ctx, wk.counters, sizeof(Counters)));
    RCCHK(ensure(ctx, wk.work_q, BCD_WORK_INTS * sizeof(int32_t)));
    int32_t *d_c = (int32_t *)wk.work_q.p; // work queues
    HIPCHK(ctx, hipMemsetAsync(d_c, 0, BCD_WORK_INTS * sizeof(int32_t), wk.stream));
    HIPCHK(ctx, hipEventRecord(wk.ev_stage[0], wk.stream));
    HIPCHK(ctx, bcd_launch_jacobi27_batch(d_A, n, d_c, std::min(ctx->num_cus * 12, (n + 1) / 2), d_eig, d_V, wk.stream, bcd_bayes27_conv2(production_rule ? 0 : 1)));
    HIPCHK(ctx, hipEventRecord(wk.ev_stage[1], wk.stream));
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    if (ms) *ms = stage_ms(wk, 0, 1);
    return BCD_HIP_OK;
}

int bcd_hip_selftest_prepare_solve(bcd_hip_ctx *ctx, const float *d_colors, const float *d_pixcov, const uint32_t *d_mask, const int32_t *d_list,
                                   int capacity, int list_len, int W, int H, int search_radius, int cu_share_pct, int64_t *differing_words)
{
    if (!ctx || !d_colors || !d_pixcov || !d_mask || !d_list || !differing_words || capacity <= 0 || W < 3 || H < 3) return bad(ctx, "bad argument");
    if (search_radius != 6) { set_err(ctx, "the fused kernel serves search radius 6"); return BCD_HIP_EUNSUPPORTED; }
    if (cu_share_pct < 1 || cu_share_pct > 100) return bad(ctx, "bad CU share");
    DEVICE_GUARD(ctx);
    touch(ctx->main);
    Work &wk = ctx->main;
    RCCHK(ensure(ctx, wk.counters, sizeof(Counters)));
    RCCHK(ensure(ctx, wk.work_q, BCD_WORK_INTS * sizeof(int32_t)));
    const size_t bytes = bcd_bayes27_record_bytes() * (size_t)capacity;
    // what is compared: everything in front of the redo list, and the list's counter
    const size_t words = RECORD27_FLOATS * (size_t)capacity + 1;
    DevAlloc rec[2], len;
    for (int i = 0; i < 2; ++i)
        if (hipMalloc(&rec[i].p, bytes) != hipSuccess) { set_err(ctx, "hipMalloc"); return BCD_HIP_ENOMEM; }
    HIPCHK(ctx, hipMalloc(&len.p, sizeof(int)));
    const int cus = std::max(1, ctx->num_cus * cu_share_pct / 100);
    unsigned long long *d_cnt = &wk.d_counters()->selftest.result;
    HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, sizeof(*d_cnt), wk.stream));
    if (list_len >= 0) HIPCHK(ctx, hipMemcpyAsync(len.p, &list_len, sizeof(int), hipMemcpyHostToDevice, wk.stream));
    for (int fused = 0; fused < 2; ++fused) {
        HIPCHK(ctx, hipMemsetAsync(rec[fused].p, 0xA5, bytes, wk.stream)); // (row 27 of V, the padding of noise + mean and records past the list's end are never written)
        HIPCHK(ctx, hipMemsetAsync(wk.work_q.p, 0, BCD_WORK_INTS * sizeof(int32_t), wk.stream));
        HIPCHK(ctx, bcd_launch_prepare_solve27(d_colors, d_pixcov, d_mask, d_list, 0, capacity, (int *)wk.work_q.p, cus, W, H, (float *)rec[fused].p, wk.stream,
                                               list_len >= 0 ? (const int *)len.p : nullptr, fused));
    }
    HIPCHK(ctx, bcd_launch_count_differing_words(rec[0].p, rec[1].p, words, d_cnt, wk.stream));
    unsigned long long h = 0;
    HIPCHK(ctx, hipMemcpyAsync(&h, d_cnt, sizeof(h), hipMemcpyDeviceToHost, wk.stream));
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    *differing_words = (int64_t)h;
    return BCD_HIP_OK;
}

int bcd_hip_selftest_division(bcd_hip_ctx *ctx, uint32_t seed, int64_t samples, int64_t *mismatches)
{
    if (!ctx || !mismatches || samples <= 0) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    touch(ctx->main);
    RCCHK(ensure(ctx, ctx->main.counters, sizeof(Counters)));
    unsigned long long *d = &ctx->main.d_counters()->selftest.result;
    HIPCHK(ctx, hipMemsetAsync(d, 0, sizeof(unsigned long long), ctx->stream));
    const int per_thread = 1024, blocks = (int)std::min<int64_t>(1 << 20, (samples + 256ll * per_thread - 1) / (256ll * per_thread));
    HIPCHK(ctx, bcd_launch_selftest_div(seed, blocks, per_thread, d, ctx->stream));
    unsigned long long h = 0;
    HIPCHK(ctx, hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *mismatches = (int64_t)h;
    return BCD_HIP_OK;
}

// ---- the list compaction behind the marking stage on its own (tests/test_gpu_marking_stage.py): the estimate call is its only other caller

int bcd_hip_selftest_active_lists(bcd_hip_ctx *ctx, const uint8_t *d_state, const int32_t *d_count, int W, int H, int patch_radius, int main_row_begin,
                                  int main_row_end, const int64_t *d_skip_word, int32_t *d_strong, int32_t *d_weak, int32_t counts_out[4])
{
    if (!ctx || !d_state || !d_count || !d_strong || !d_weak || !counts_out || W <= 0 || H <= 0 || patch_radius < 0) return bad(ctx, "bad argument");
    if (main_row_begin < 0 || main_row_end > H || main_row_begin > main_row_end) return bad(ctx, "bad main row range");
    DEVICE_GUARD(ctx);
    touch(ctx->main);
    Work &wk = ctx->main;
    static_assert(sizeof(long long) == sizeof(int64_t), "64-bit counters");
    const int K = 3 * (2 * patch_radius + 1) * (2 * patch_radius + 1);
    RCCHK(ensure(ctx, wk.counters, sizeof(Counters)));
    Counters::Lists *d_c = &wk.d_counters()->lists;
    HIPCHK(ctx, hipMemsetAsync(d_c, 0, sizeof(*d_c), wk.stream));
    HIPCHK(ctx, bcd_launch_active_lists(d_state, d_count, (int64_t)main_row_begin * W, (int64_t)main_row_end * W, K + 1, d_strong, d_weak, &d_c->n_strong, wk.stream,
                                        reinterpret_cast<const long long *>(d_skip_word)));
    HIPCHK(ctx, hipMemcpyAsync(counts_out, d_c, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, wk.stream)); // (the list lengths and the sum of |S|)
    HIPCHK(ctx, hipStreamSynchronize(wk.stream));
    return BCD_HIP_OK;
}

// ---- the host-buffer upload path piece by piece (tests/test_gpu_sparse_upload.py, tests/test_gpu_host_stream.py)

int bcd_hip_selftest_sparse_upload(bcd_hip_ctx *ctx, const float *h_src, int64_t n, float *d_dst, int new_frame, int64_t piece_floats,
                                   int64_t *raw_bytes, int64_t *sent_bytes)
{
    if (!ctx || !h_src || !d_dst || n < 0 || piece_floats < 0 || (piece_floats & 3) != 0 || !raw_bytes || !sent_bytes) return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    RCCHK(host_upload_stream(ctx));
    RCCHK(host_sparse_uploader(ctx));
    if (new_frame) bcd_sparse_frame_begin(ctx->sparse);
    bcd_sparse_set_piece(ctx->sparse, (size_t)piece_floats);
    const hipError_t e = bcd_sparse_upload(ctx->sparse, d_dst, h_src, (size_t)n, ctx->upload_stream);
    bcd_sparse_set_piece(ctx->sparse, 0); // (the host path keeps the default)
    const hipError_t e2 = hipStreamSynchronize(ctx->upload_stream);
    HIPCHK(ctx, e);
    HIPCHK(ctx, e2);
    long long raw = 0, sent = 0;
    bcd_sparse_frame_bytes(ctx->sparse, &raw, &sent);
    *raw_bytes = raw; *sent_bytes = sent;
    return BCD_HIP_OK;
}

// the flag words of the distance kernels as the upload self-tests return them: bit 0 range, bit 1 "a pixel carries another sample count"
static int read_plane_flags(bcd_hip_ctx *ctx, Work &wk, int *out)
{
    Counters::Flags flags = {};
    HIPCHK(ctx, hipMemcpyAsync(&flags, &wk.d_counters()->flags, sizeof(flags), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *out = (flags.range & ~2) | (flags.other_count ? 2 : 0);
    return BCD_HIP_OK;
}

int bcd_hip_selftest_host_stream(bcd_hip_ctx *ctx, const float *h_colors, const float *h_ns, const float *h_hist, const float *h_cov, int W, int H, int D,
                                 const bcd_hip_params *prm, float spike_factor, int stop_after_chunks, int poison, void *d_planes, uint8_t *d_counts,
                                 float *d_colors_out, float *d_ns_out, float *d_hist_out, float *d_cov_out, float *d_hist_uploaded,
                                 bcd_hip_host_stream_result *res)
{
    if (!ctx) return BCD_HIP_EINVAL;
    if (!h_colors || !h_ns || !h_hist || !h_cov || !d_planes || !d_counts || !d_colors_out || !d_ns_out || !d_hist_out || !d_cov_out || !res) return bad(ctx, "null pointer");
    RCCHK(check_params(ctx, W, H, D, prm));
    DEVICE_GUARD(ctx);
    const bool prefilter = spike_factor > 0.f;
    if (prefilter && (W < 3 || H < 3)) return bad(ctx, "image smaller than 3x3");
    if (!host_frame_streams(ctx, H, D, prm)) { set_err(ctx, "bcd_hip_denoise_host_ex would not stream this frame in"); return BCD_HIP_EUNSUPPORTED; }
    touch(ctx->main);
    const size_t np = (size_t)W * H;
    const size_t sz[4] = { np * 3, np, np * D, np * 6 };
    const float *src[4] = { h_colors, h_ns, h_hist, h_cov };
    // the device copies bcd_hip_denoise_host_ex uses
    float *d[9];
    for (int i = 0; i < 4; ++i) { RCCHK(ensure(ctx, ctx->host_stage[i], sz[i] * sizeof(float))); d[i] = (float *)ctx->host_stage[i].p; }
    d[4] = nullptr;
    for (int i = 0; i < 4; ++i) {
        d[5 + i] = d[i];
        if (prefilter) { RCCHK(ensure(ctx, ctx->host_stage[5 + i], sz[i] * sizeof(float))); d[5 + i] = (float *)ctx->host_stage[5 + i].p; }
    }
    const int b = prm->search_radius, nd = bcd_delta_count(b);
    HostStreamProgress done;
    const int rc = host_stream_frame(ctx, src, d, W, H, D, b, prm->hist_dist_threshold, prefilter, spike_factor, stop_after_chunks, poison != 0, &done, false /* the T / C planes this entry point returns */);
    // (also after a failure: nothing of this call stays in flight on the upload streams)
    hipError_t e = ctx->upload_stream ? hipStreamSynchronize(ctx->upload_stream) : hipSuccess;
    if (ctx->upload_stream2) { const hipError_t e2 = hipStreamSynchronize(ctx->upload_stream2); if (e == hipSuccess) e = e2; }
    RCCHK(rc);
    HIPCHK(ctx, e);
    Work &wk = ctx->main;
    float *outs[4] = { d_colors_out, d_ns_out, d_hist_out, d_cov_out };
    for (int i = 0; i < 4; ++i) HIPCHK(ctx, hipMemcpyAsync(outs[i], d[5 + i], sz[i] * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    if (d_hist_uploaded) HIPCHK(ctx, hipMemcpyAsync(d_hist_uploaded, d[2], sz[2] * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_planes, wk.T.p, np * nd * 2, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_counts, wk.Cn.p, np * nd, hipMemcpyDeviceToDevice, ctx->stream));
    int flag = 0;
    RCCHK(read_plane_flags(ctx, wk, &flag));
    res->rows_filtered = done.rows_filtered; res->tile_rows_done = done.tile_rows_done; res->chunk_lines = done.chunk_lines; res->chunks_done = done.chunks;
    res->range_flag = flag; res->uni_n = done.uni_n; res->ratio_form = done.ratio ? 1 : 0;
    return BCD_HIP_OK;
}

int bcd_hip_approx_planes(bcd_hip_ctx *ctx, const float *d_hist, const float *d_ns, int W, int H, int D, int search_radius, float uni_n, int ratio_form, float tau,
                          void *d_planes, uint8_t *d_counts, int *range_flag)
{
    if (!ctx || !d_hist || !d_ns || !d_planes || !d_counts || !range_flag || W <= 0 || H <= 0 || search_radius < 1 || !(uni_n >= 0.f) || (ratio_form && uni_n != 0.f))
        return bad(ctx, "bad argument");
    DEVICE_GUARD(ctx);
    touch(ctx->main);
    if (!bcd_pairdist_rw_supported(D)) { set_err(ctx, "no approximate kernel for this histogram depth"); return BCD_HIP_EUNSUPPORTED; }
    Work &wk = ctx->main;
    RCCHK(ensure(ctx, wk.counters, sizeof(Counters)));
    Counters::Flags *d_flag = &wk.d_counters()->flags;
    HIPCHK(ctx, hipMemsetAsync(d_flag, 0, sizeof(*d_flag), ctx->stream));
    if (ratio_form) {
        RCCHK(ensure(ctx, wk.ratio_stats, 128 * sizeof(unsigned int)));
        HIPCHK(ctx, bcd_launch_pairdist_rw_ratio(d_hist, d_ns, W, H, D, search_radius, d_planes, d_counts, &d_flag->range, tau, (unsigned int *)wk.ratio_stats.p, ctx->stream));
    } else HIPCHK(ctx, bcd_launch_pairdist_rw(d_hist, d_ns, W, H, D, search_radius, d_planes, d_counts, &d_flag->range, uni_n, ctx->stream));
    return read_plane_flags(ctx, wk, range_flag);
}

} // extern "C"
