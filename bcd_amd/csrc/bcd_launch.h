// bcd_launch.h -- the launchers implemented in the k_*.hip files and in bcd_sparse_upload.hip, as the host orchestration files (bcd_api.hip,
// bcd_host.hip, bcd_accum.hip, bcd_selftest.hip) call them.  The parameter names are those of the definitions, and default arguments live here only.
// The files of the estimate chain -- k_bayes27.hip, k_jacobi27.hip, k_bayes_temporal.hip and k_bayes.hip -- include this header, so the compiler
// checks their launchers' definitions against these declarations.  The other kernel files do not: k_similarity_fast.hip must stay byte for byte what
// it is, because bench.py keys its recorded profiles on that file's hash, and the rest have not been converted; a launcher of theirs whose signature
// changes is changed here by hand.
#pragma once
#include "bcd_common.h"

#include <stddef.h>

// ---- k_similarity.hip
size_t bcd_pairdist_lds_bytes(int D, int b);
hipError_t bcd_launch_pairdist(const float *hist, const float *ns, int W, int H, int D, int b, float *T, uint8_t *Cn, int fast, int *d_range_flag, float uni_n,
                               hipStream_t st);
hipError_t bcd_launch_uniform_n(const float *ns, int64_t npix, int *d_out, hipStream_t st);
hipError_t bcd_launch_compare_planes(const float *Ta, const uint8_t *Ca, const float *Tb, const uint8_t *Cb, int64_t n, unsigned long long *out, hipStream_t st);
hipError_t bcd_launch_selftest_div(uint32_t seed, int blocks, int per_thread, unsigned long long *d_mismatches, hipStream_t st);
hipError_t bcd_launch_masks(const float *T, const uint8_t *Cn, int W, int H, int w, int b, float tau, uint32_t *mask, int32_t *count, uint32_t *fwd_scratch,
                            hipStream_t st, const BcdBorderline *ap, const float *hist, const float *ns, int D);
hipError_t bcd_launch_masks_finish(int W, int H, int b, float tau, uint32_t *mask, int32_t *count, uint32_t *fwd_scratch, hipStream_t st, const BcdBorderline *ap,
                                   const float *hist, const float *ns, int D);
hipError_t bcd_launch_window_distances(const float *T, const uint8_t *Cn, int W, int H, int w, int b, int r, int c, float *out, hipStream_t st);

// ---- k_similarity_cross.hip
hipError_t bcd_launch_pairdist_cross(const float *histA, const float *nsA, const float *histB, const float *nsB, int W, int H, int D, int b, float *T, uint8_t *Cn,
                                     hipStream_t st);
hipError_t bcd_launch_masks_cross(const float *T, const uint8_t *Cn, int W, int H, int w, int b, float tau, uint32_t *mask, int32_t *count, hipStream_t st);
hipError_t bcd_launch_add_counts(int32_t *nsim, const int32_t *add, int64_t npix, hipStream_t st);
hipError_t bcd_launch_window_distances_cross(const float *T, const uint8_t *Cn, int W, int H, int w, int b, int r, int c, float *out, hipStream_t st);

// ---- k_masks_transpose.hip (includes this header)
hipError_t bcd_launch_masks_transpose(const uint32_t *in, int W, int H, int b, uint32_t *out, int32_t *count, hipStream_t st);
hipError_t bcd_launch_mask_popcount(const uint32_t *mask, int64_t npix, int words, int32_t *count, hipStream_t st);

// ---- k_warp.hip (includes this header)
hipError_t bcd_launch_warp_frame(const float *col, const float *ns, const float *hist, const float *cov, const float *mv, int W, int H, int D, float *ocol, float *ons,
                                 float *ohist, float *ocov, uint8_t *valid, hipStream_t st);
hipError_t bcd_launch_warp_layers(const BcdWarpLayerTable &t, int layers, const float *mv, int W, int H, uint8_t *valid, hipStream_t st);
hipError_t bcd_launch_warp_features(const float *feat, const float *var, int F, const float *mv, int W, int H, float *ofeat, float *ovar, uint8_t *valid, hipStream_t st);
hipError_t bcd_launch_valid_down(const uint8_t *valid, int W, int H, uint8_t *out, hipStream_t st);
hipError_t bcd_launch_valid_patch(const uint8_t *valid, int W, int H, int w, uint8_t *pvalid, hipStream_t st);
hipError_t bcd_launch_masks_gate_valid(uint32_t *mask, int32_t *count, const uint8_t *pvalid, int W, int H, int w, int b, hipStream_t st);

// ---- k_motion_compose.hip (includes this header)
hipError_t bcd_launch_motion_compose(const float *a, const float *b, int W, int H, float *out, hipStream_t st);

// ---- k_bayes_temporal.hip, and the launcher of k_bayes27.hip that runs behind its prepare kernel
hipError_t bcd_launch_prepare27t(const BcdFrameTable &t, const int32_t *list, int first_item, int nb_items, int *d_work, int num_cus, int W, int b, float *records,
                                 hipStream_t st);
hipError_t bcd_launch_bayes_weak_temporal(const BcdFrameTable &t, const int32_t *list, const int32_t *d_nlist, int blocks, int W, int b, float *sum, int32_t *cnt,
                                          hipStream_t st);
hipError_t bcd_launch_bayes_weak_temporal_layers(const BcdFrameLayerTable &t, const int32_t *list, const int32_t *d_nlist, int blocks, int W, int b, int32_t *cnt,
                                                 hipStream_t st);
hipError_t bcd_launch_solve_finish27(const float *colors, const float *pixcov, const uint32_t *mask, const int32_t *list, int first_item, int nb_items, int *d_work,
                                     int num_cus, int W, int H, float min_eig, float *records, float *sum, int32_t *cnt, int *d_spectral, hipStream_t st);

// ---- k_similarity_moments.hip
hipError_t bcd_launch_pairdist_moments(const float *colors, const float *pixcov, int W, int H, int b, float var_floor, float *T, uint8_t *Cn, hipStream_t st);

// ---- k_similarity_guide.hip
hipError_t bcd_pairdist_guide_launchable(int F, int has_var, int b);
hipError_t bcd_launch_pairdist_guide(const float *features, const float *variances, int F, const float *floors, int W, int H, int b, float *T, uint8_t *Cn,
                                     hipStream_t st);
hipError_t bcd_launch_gate_masks(uint32_t *mask, const uint32_t *gate, int32_t *nsim, int W, int H, int b, hipStream_t st);
hipError_t bcd_launch_scale_inplace(float *x, float a, int64_t n, hipStream_t st);

// ---- k_similarity_guide_cross.hip
int bcd_pairdist_guide_cross_band(int F, int has_var, int b); // displacement lines per staging; 0: a geometry the kernel does not serve
hipError_t bcd_launch_pairdist_guide_cross(const float *featA, const float *varA, const float *featB, const float *varB, int F, const float *floors, int W, int H,
                                           int b, float *T, uint8_t *Cn, hipStream_t st);

// ---- k_similarity_moments_cross.hip
int bcd_pairdist_moments_cross_band(int b);              // displacement lines per staging; 0: a search radius the kernel does not serve
int bcd_masks_moments_cross_fused_applies(int w, int b); // the form without planes: patch radius 1, search radius 1 .. 6
hipError_t bcd_launch_pairdist_moments_cross(const float *colA, const float *pixcovA, const float *colB, const float *pixcovB, int W, int H, int b, float var_floor,
                                             float *T, uint8_t *Cn, hipStream_t st);
hipError_t bcd_launch_masks_moments_cross_fused(const float *colA, const float *pixcovA, const float *colB, const float *pixcovB, int W, int H, int b, float tau,
                                                float var_floor, uint32_t *mask, int32_t *count, hipStream_t st);

// ---- k_similarity_fast.hip
int bcd_pairdist_rw_supported(int D);
int bcd_pairdist_rw_tile_lines();
// margin_tau > 0: the margin form -- one signed binary16 plane E = sum over the live bins of (d^2 / s - margin_tau) in T, Cn is not written; 0: the T / C planes
// (the RATIO form always writes T / C planes)
hipError_t bcd_launch_pairdist_rw(const float *hist, const float *ns, int W, int H, int D, int b, void *T /* binary16 planes */, uint8_t *Cn, int *d_range_flag,
                                  float uni_n, hipStream_t st, float margin_tau = 0.f);
hipError_t bcd_launch_pairdist_rw_rows(const float *hist, const float *ns, int W, int H, int D, int b, void *T /* binary16 planes */, uint8_t *Cn, int *d_range_flag,
                                       float uni_n, int tile_row_begin, int tile_row_end, hipStream_t st, float margin_tau = 0.f);
hipError_t bcd_launch_pairdist_rw_ratio(const float *hist, const float *ns, int W, int H, int D, int b, void *T /* binary16 planes */, uint8_t *Cn, int *d_range_flag,
                                        float tau, unsigned int *stats, hipStream_t st);
hipError_t bcd_launch_ratio_begin(unsigned int *stats, hipStream_t st);
hipError_t bcd_launch_pairdist_rw_ratio_rows(const float *hist, const float *ns, int W, int H, int D, int b, void *T /* binary16 planes */, uint8_t *Cn, int *d_range_flag,
                                             unsigned int *stats, int tile_row_begin, int tile_row_end, hipStream_t st);
hipError_t bcd_launch_ratio_verdict(const unsigned int *stats, float tau, int *d_range_flag, hipStream_t st);
hipError_t bcd_launch_pairdist_rw_counting(const float *hist, const float *ns, int W, int H, int D, int b, void *T, uint8_t *Cn, int *d_range_flag, float uni_n,
                                           unsigned long long *work_count, hipStream_t st);
hipError_t bcd_launch_max_rel_dev(const float *Ta, const float *Tb, const uint8_t *Ca, const uint8_t *Cb, int W, int H, int b, unsigned int *out, hipStream_t st);

// ---- bcd_sparse_upload.hip
struct BcdSparseUploader;
BcdSparseUploader *bcd_sparse_create();
void bcd_sparse_destroy(BcdSparseUploader *u);
void bcd_sparse_frame_begin(BcdSparseUploader *u);
void bcd_sparse_frame_bytes(const BcdSparseUploader *u, long long *raw, long long *sent);
void bcd_sparse_set_piece(BcdSparseUploader *u, size_t floats);
hipError_t bcd_sparse_upload(BcdSparseUploader *u, float *dst, const float *src, size_t n, hipStream_t st);

// ---- k_pointwise.hip
hipError_t bcd_launch_pixel_cov(const float *cov, const float *ns, int64_t npix, float *out, hipStream_t st);
hipError_t bcd_launch_pixel_cov_clear(const float *cov, const float *ns, int64_t npix, float *out, float *sum, int32_t *cnt, hipStream_t st);
hipError_t bcd_launch_scale_begin(int *a, int na, int keep0, int keep1, int *b, int nb, int *c, int nc, hipStream_t st);
hipError_t bcd_launch_finalize(const float *sum, const int32_t *cnt, int64_t npix, float *out, hipStream_t st);
hipError_t bcd_launch_finalize_band(const float *sum, const int32_t *cnt, int W, int rows, int halo, const float *up_sum, const int32_t *up_cnt, const float *dn_sum,
                                    const int32_t *dn_cnt, float *out, hipStream_t st);
hipError_t bcd_launch_zero_bad(float *img, int64_t n, hipStream_t st);
hipError_t bcd_launch_downscale(int mode, const float *in, int W, int H, int D, float *out, hipStream_t st);
hipError_t bcd_launch_downscale_cov(const float *cov, const float *ns, int W, int H, float *out, hipStream_t st);
hipError_t bcd_launch_interpolate(int mode, const float *lo, int w, int h, int D, float *hi, int W, int H, hipStream_t st);
hipError_t bcd_launch_merge_interpolate(const float *a, const float *b, int w, int h, int D, float *hi, int W, int H, hipStream_t st);
hipError_t bcd_launch_spike(const float *col, const float *ns, const float *hist, const float *cov, int W, int H, int D, float factor, float *ocol, float *ons,
                            float *ohist, float *ocov, hipStream_t st);
hipError_t bcd_launch_spike_rows(const float *col, const float *ns, const float *hist, const float *cov, int W, int H, int D, float factor, float *ocol, float *ons,
                                 float *ohist, float *ocov, int row_begin, int row_end, hipStream_t st);
hipError_t bcd_launch_accumulate_samples(const float *samples, const float *weights, int64_t npix, int spp, int nbins, float gamma, float maxval, float *ons,
                                         float *omean, float *ocov, float *ohist, hipStream_t st);
hipError_t bcd_launch_layers_pixel_cov_clear(const BcdLayerTable &t, int layers, const float *ns, int64_t npix, float *pixcov, float *sum, hipStream_t st);
// ... the covariances alone (a push of a sequence; the pops clear the sums).  t.a[k] and pixcov 8 B aligned
hipError_t bcd_launch_layers_pixel_cov(const BcdLayerTable &t, int layers, const float *ns, int64_t npix, float *pixcov, hipStream_t st);
hipError_t bcd_launch_layers_finalize(const BcdLayerTable &t, int layers, const int32_t *cnt, int64_t npix, hipStream_t st);
hipError_t bcd_launch_layers_downscale_avg(const BcdLayerTable &t, int layers, int W, int H, hipStream_t st);
hipError_t bcd_launch_layers_downscale_cov(const BcdLayerTable &t, int layers, const float *ns, int W, int H, hipStream_t st);
hipError_t bcd_launch_layers_merge(const BcdLayerTable &t, int layers, int w, int h, int W, int H, hipStream_t st);

// ---- k_spike.hip
hipError_t bcd_launch_spike_map(const float *col, int W, int H, float factor, int32_t *map, int32_t *d_moved, hipStream_t st);
hipError_t bcd_launch_spike_apply(const BcdSpikeTable &t, int n, const int32_t *map, int W, int H, int depth, hipStream_t st);

// ---- k_spike_inplace.hip
hipError_t bcd_launch_spike_moved_count(const int32_t *map, uint32_t npix, int32_t *d_count, hipStream_t st);
hipError_t bcd_launch_spike_compact(const int32_t *map, uint32_t npix, int32_t *d_cursor, int2 *list, uint32_t capacity, hipStream_t st);
size_t bcd_spike_stage_floats(BcdSpikeInplaceTable &t, int n, uint32_t moved);
hipError_t bcd_launch_spike_stage(const BcdSpikeInplaceTable &t, int n, const int2 *list, uint32_t moved, float *stage, hipStream_t st);

// ---- k_active.hip
hipError_t bcd_launch_active_init(const int32_t *nsim, int W, int H, int w, int row_begin, int row_end, float skip_prob, uint32_t seed, int row_offset, uint8_t *state,
                                  hipStream_t st);
hipError_t bcd_launch_active_round(const uint32_t *mask, const int32_t *nsim, uint8_t *state, int W, int H, int b, int min_strong, int random_order, uint32_t seed,
                                   int row_begin, int row_end, int row_offset, int *undecided, hipStream_t st);
hipError_t bcd_launch_mark_deps(const uint32_t *mask, const int32_t *nsim, uint8_t *state, uint32_t *dep, int W, int H, int b, int min_strong, int random_order,
                                uint32_t seed, int row_begin, int row_end, int row_offset, int *undecided, hipStream_t st);
hipError_t bcd_launch_mark_round(const uint32_t *dep, uint8_t *state, int W, int H, int b, int row_begin, int row_end, int iters, int *undecided, hipStream_t st);
hipError_t bcd_launch_sum_counter_lines(const int *lines, int rounds, int *out, hipStream_t st, long long *total_out = nullptr, const int *flags = nullptr,
                                        int border_capacity = 0);
hipError_t bcd_launch_active_lists(const uint8_t *state, const int32_t *nsim, int64_t p_begin, int64_t p_end, int min_strong, int32_t *strong_list, int32_t *weak_list,
                                   int32_t *counters, hipStream_t st, const long long *skip_if);

// ---- k_bayes.hip
size_t bcd_bayes_lds_bytes(int w, int b);
size_t bcd_bayes_scratch_bytes_per_block(int w, int b);
hipError_t bcd_launch_bayes_strong(const float *colors, const float *pixcov, const uint32_t *mask, const int32_t *list, const int32_t *d_nlist, int *d_work, int blocks,
                                   int W, int H, int w, int b, float min_eig, float *sum, int32_t *cnt, float *gscratch, size_t gscratch_bytes, hipStream_t st);
hipError_t bcd_launch_bayes_weak(const float *colors, const uint32_t *mask, const int32_t *list, const int32_t *d_nlist, int blocks, int W, int H, int w, int b,
                                 float *sum, int32_t *cnt, hipStream_t st);
hipError_t bcd_launch_bayes_weak_tiles(const float *colors, const uint32_t *mask, const uint8_t *state, const int32_t *nsim, int min_strong, int W, int H, int b,
                                       float *sum, int32_t *cnt, hipStream_t st, int row_begin, int row_end, const long long *skip_if);
hipError_t bcd_launch_bayes_weak_tiles_layers(const BcdLayerTable &t, int layers, const uint32_t *mask, const uint8_t *state, const int32_t *nsim, int min_strong,
                                              int W, int H, int b, hipStream_t st, int row_begin, int row_end);

// ---- k_jacobi27.hip
void bcd_bayes27_set_strict_eigensolver(int on);
float bcd_bayes27_conv2(int strict);
float bcd_bayes27_chain_conv2(); // the rule the estimate chain runs with: the setter's, else the environment's
hipError_t bcd_launch_jacobi27_batch(const float *A, int n, int *d_work, int blocks, float *eig, float *V, hipStream_t st, float conv2 = 1e-12f, float *Aout = nullptr,
                                     const int *d_n = nullptr, int first_item = 0);

// ---- k_bayes27.hip
// the estimate chain's environment switches, read once per process; every one selects a comparison form that the README documents.  strict_eigen and
// prepare_solve_split also have setters, which override the environment (bcd_bayes27_set_strict_eigensolver, bcd_bayes27_set_fused_prepare_solve)
struct BcdBayes27Switches {
    bool finish_lds;          // BCD_HIP_FINISH_LDS=1           the finish through LDS matrices instead of the register-resident kernel
    bool jacobi_pairs;        // BCD_HIP_JACOBI_PAIRS=1         the eigensolver that moves its rows through LDS every round
    bool prepare_gather;      // BCD_HIP_PREPARE_GATHER=1       b = 12: members gathered from memory instead of an LDS window
    bool prepare_solve_split; // BCD_HIP_PREPARE_SOLVE_SPLIT=1  b = 6: prepare and solve as two launches
    bool strict_eigen;        // BCD_HIP_STRICT_EIGEN=1         the eigensolver's fully converged stopping rule
};
const BcdBayes27Switches &bcd_bayes27_switches();
size_t bcd_bayes27_lds_bytes(int b);
size_t bcd_bayes27_record_bytes();
void bcd_bayes27_set_fused_prepare_solve(int on);
int bcd_bayes27_fused_prepare_solve();
// the prepare and eigensolver phases of a chunk on their own (default search radius; records laid out as by bcd_launch_bayes27), fused or as two launches
hipError_t bcd_launch_prepare_solve27(const float *colors, const float *pixcov, const uint32_t *mask, const int32_t *list, int first_item, int nb_items,
                                      int *d_work, int num_cus, int W, int H, float *records, hipStream_t st, const int *d_nb_items, int fused);
hipError_t bcd_launch_count_differing_words(const void *a, const void *b, size_t words, unsigned long long *d_count, hipStream_t st);
// d_spectral: += items whose inverse took the spectral branch; defer_redo != 0: the caller reads *d_spectral after its next synchronisation and calls
// bcd_launch_bayes27_redo if it is > 0; d_nb_items (optional): the list's length on the device, nb_items then being the capacity of `records`
hipError_t bcd_launch_bayes27(const float *colors, const float *pixcov, const uint32_t *mask, const int32_t *list, int first_item, int nb_items, int *d_work,
                              int num_cus, int W, int H, int b, float min_eig, float *records, float *sum, int32_t *cnt, int *d_spectral, hipStream_t st,
                              int defer_redo, const int *d_nb_items);
hipError_t bcd_launch_bayes27_redo(const float *colors, const float *pixcov, const uint32_t *mask, const int32_t *list, int first_item, int nb_items, int *d_work,
                                   int num_cus, int W, int H, int b, float min_eig, float *records, float *sum, int32_t *cnt, hipStream_t st);

// ---- k_accumulate.hip
size_t bcd_accum_snapshot_lds(int D);
hipError_t bcd_launch_accum_dense(const float *samples, const float *weights, int64_t p0, int64_t npix, int64_t N, int k, int channels, int nbins, float gamma,
                                  float maxval, float *st, hipStream_t s);
hipError_t bcd_launch_accum_dense_layers(const BcdAccumLayerIn &in, int nb_layers, const float *weights, int64_t p0, int64_t npix, int64_t N, int k, int channels,
                                         float *layers, hipStream_t s);
hipError_t bcd_launch_accum_segments_layers(const uint32_t *keys, const uint32_t *vals, int64_t n, int64_t N, const BcdAccumLayerIn &in, int nb_layers,
                                            const float *weights, float *layers, hipStream_t s);
hipError_t bcd_launch_accum_snapshot_layers(const float *st, const float *layers, int64_t N, const BcdAccumLayerOut &out, int nb_layers, hipStream_t s);
hipError_t bcd_launch_accum_keys(const int32_t *pix, int64_t n, int64_t N, uint32_t *keys, uint32_t *vals, unsigned long long *dropped, hipStream_t s);
hipError_t bcd_accum_sort(void *tmp, size_t *tmp_bytes, const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout, int64_t n, int end_bit,
                          hipStream_t s);
hipError_t bcd_launch_accum_segments(const uint32_t *keys, const uint32_t *vals, int64_t n, int64_t N, const float *rgb, const float *weights, int nbins, float gamma,
                                     float maxval, float *st, hipStream_t s);
hipError_t bcd_launch_accum_snapshot(const float *st, int64_t N, int D, float *ons, float *omean, float *ocov, float *ohist, hipStream_t s);
hipError_t bcd_launch_accum_moments(const float *st, int64_t N, float *ons, float *omean, float *ocov, hipStream_t s);
int bcd_splat_ring_cells(int nx, int ny);
int bcd_splat_max_staged(int ts);
// filter: rx, ry, inv_rx, inv_ry; geom: ts, kx, ky, nx, ny; T: the table on the device
hipError_t bcd_launch_splat_keys(const float *xy, int64_t n, int W, int H, const float *filter, const int *geom, const float *T, uint32_t *keys, uint32_t *vals,
                                 unsigned long long *dropped, hipStream_t s);
hipError_t bcd_launch_splat_cells(const uint32_t *keys, int64_t n, int64_t NE, void *cells, hipStream_t s);
hipError_t bcd_launch_splat(const void *cells, const uint32_t *vals, const float *xy, const float *rgb, const float *weights, int W, int H, const float *filter,
                            const int *geom, const float *T, int cap, int nbins, float gamma, float maxval, float *st, hipStream_t s, bool layer = false);
size_t bcd_plan_red_bytes();
hipError_t bcd_plan_scan_bytes(int64_t N, size_t *bytes);
hipError_t bcd_launch_accum_plan(const float *st, int64_t N, float eps, float min_samples, float tau, int K, int64_t B, uint64_t offset, float *err, int32_t *counts,
                                 int32_t *pixels, int64_t capacity, int64_t *summary, void *red, uint64_t *C, int32_t *ends, void *tmp, size_t tmp_bytes,
                                 hipStream_t s);
hipError_t bcd_launch_accum_merge(float *dst, const float *src, int64_t n, int num_cus, hipStream_t s);
hipError_t bcd_launch_accum_counter(unsigned long long *dst, const unsigned long long *src, unsigned long long add, int keep, hipStream_t s);

// ---- k_accum_features.hip (F: feature channels, 1 .. 8; ft: the 2 F feature planes; feat: F consecutive floats per sample)
hipError_t bcd_launch_feat_dense(const float *feat, int F, const float *weights, int64_t p0, int64_t npix, int64_t N, int k, float *ft, hipStream_t s);
hipError_t bcd_launch_feat_segments(const uint32_t *keys, const uint32_t *vals, int64_t n, int64_t N, const float *feat, int F, const float *weights, float *ft,
                                    hipStream_t s);
int bcd_feat_splat_max_staged(int ts, int F);
hipError_t bcd_launch_feat_splat(const void *cells, const uint32_t *vals, const float *xy, const float *feat, int F, const float *weights, int W, int H,
                                 const float *filter, const int *geom, const float *T, int cap, float *ft, hipStream_t s);
hipError_t bcd_launch_feat_snapshot(const float *st, const float *ft, int64_t N, int F, float *omean, float *ovar, hipStream_t s);
