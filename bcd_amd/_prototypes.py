"""The C ABI of include/bcd_hip.h as ctypes sees it: the Structure mirrors of the header's structs and PROTOTYPES, one (restype, argtypes) entry per
entry point, in the header's order and under its section comments.  hip.lib() applies the table once, when it loads the library; no call site
declares a prototype or wraps a scalar.  tests/test_abi_prototypes.py derives both again from the header and compares.

A parameter maps by this rule, without exception:
    int, int32_t -> c_int        uint32_t -> c_uint32        int64_t -> c_int64        uint64_t -> c_uint64
    long long -> c_longlong      float -> c_float            bcd_hip_progress_fn -> PROGRESS_FN
    pointer to a scalar, void, char, another pointer or an opaque handle (bcd_hip_ctx, _accum, _selection, _multi; * and **) -> c_void_p
    pointer to a struct with a mirror below -> POINTER(mirror); to a struct without one (bcd_hip_warped_layer) -> c_void_p
    array parameter (int32_t counts_out[4]) -> as a pointer
A structure field maps as a parameter does, with int32_t written c_int32, uint8_t -> c_uint8, char -> c_char, an array as type * n and a nested struct
as its mirror.  Every pointer field is c_void_p, except the four that are assigned ctypes arrays or pointers, which c_void_p fields do not take:
Guide.floors (POINTER(c_float)), FrameLayers.layers (POINTER(FrameLayer)), StageFrameLayers.d_colors and .d_pixel_cov (POINTER(c_void_p)).
A return type: int -> c_int, void -> None, const char * -> c_char_p, uint32_t -> c_uint32.
c_void_p takes None, an address, a c_void_p, byref(x), a ctypes array or pointer; POINTER(mirror) takes None, byref(mirror) and an array of
mirrors -- a device address of a struct goes through ctypes.cast."""
import ctypes as C


class Params(C.Structure):
    """mirrors bcd::DenoiserParameters (include/bcd/core/IDenoiser.h:20-44 of the reference)"""
    _c_name_ = "bcd_hip_params"
    _fields_ = [("hist_dist_threshold", C.c_float), ("patch_radius", C.c_int32), ("search_radius", C.c_int32),
                ("min_eigen_value", C.c_float), ("use_random_pixel_order", C.c_int32),
                ("marked_skip_probability", C.c_float), ("order_seed", C.c_uint32)]


class ScaleStats(C.Structure):
    _c_name_ = "bcd_hip_scale_stats"
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("main_pixels", C.c_int64), ("processed", C.c_int64),
                ("fallback", C.c_int64), ("similar_total", C.c_int64), ("active_rounds", C.c_int32),
                ("ms_similarity", C.c_float), ("ms_active", C.c_float), ("ms_bayes", C.c_float), ("ms_total", C.c_float),
                ("similarity_path", C.c_int32), ("borderline_pairs", C.c_int32), ("cu_share", C.c_int32), ("spectral_inverses", C.c_int32)]


MAX_LAYERS = 16  # BCD_HIP_MAX_LAYERS


class Layer(C.Structure):
    _c_name_ = "bcd_hip_layer"
    _fields_ = [("d_colors", C.c_void_p), ("d_covariances", C.c_void_p), ("d_out", C.c_void_p)]


class SelectionScale(C.Structure):
    _c_name_ = "bcd_hip_selection_scale"
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("processed", C.c_int64), ("fallback", C.c_int64), ("similar_total", C.c_int64),
                ("similarity_path", C.c_int32), ("reserved", C.c_int32)]


SELECTION_MAX_SCALES = 16  # BCD_HIP_SELECTION_MAX_SCALES


class SelectionInfo(C.Structure):
    _c_name_ = "bcd_hip_selection_info"
    _fields_ = [("valid", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("D", C.c_int32), ("nb_scales", C.c_int32), ("params", Params),
                ("device_bytes", C.c_int64), ("scale", SelectionScale * SELECTION_MAX_SCALES)]


class Guide(C.Structure):
    """auxiliary feature buffers that gate the similar-patch selection"""
    _c_name_ = "bcd_hip_guide"
    _fields_ = [("features", C.c_void_p), ("variances", C.c_void_p), ("nb_channels", C.c_int32), ("floors", C.POINTER(C.c_float)), ("threshold", C.c_float)]


class Frame(C.Structure):
    """one neighbour frame of bcd_hip_denoise_temporal[_host]"""
    _c_name_ = "bcd_hip_frame"
    _fields_ = [("d_colors", C.c_void_p), ("d_nsamples", C.c_void_p), ("d_histograms", C.c_void_p), ("d_covariances", C.c_void_p), ("reserved", C.c_void_p)]


class StageFrame(C.Structure):
    """one frame of bcd_hip_bayes_accumulate_temporal"""
    _c_name_ = "bcd_hip_stage_frame"
    _fields_ = [("d_colors", C.c_void_p), ("d_pixel_cov", C.c_void_p), ("d_mask", C.c_void_p)]


class SequenceInfo(C.Structure):
    """what bcd_hip_sequence_info reports"""
    _c_name_ = "bcd_hip_sequence_info"
    _fields_ = [("frames_pushed", C.c_int64), ("frames_popped", C.c_int64), ("device_bytes", C.c_int64), ("bytes_uploaded", C.c_int64),
                ("pyramids_built", C.c_int64), ("cross_computed", C.c_int64), ("cross_transposed", C.c_int64)]


class FrameLayer(C.Structure):
    """one colour layer of a neighbour frame of bcd_hip_denoise_temporal_layers[_host]"""
    _c_name_ = "bcd_hip_frame_layer"
    _fields_ = [("d_colors", C.c_void_p), ("d_covariances", C.c_void_p)]


class FrameLayers(C.Structure):
    """one neighbour frame of bcd_hip_denoise_temporal_layers[_host]"""
    _c_name_ = "bcd_hip_frame_layers"
    _fields_ = [("d_nsamples", C.c_void_p), ("d_histograms", C.c_void_p), ("layers", C.POINTER(FrameLayer)), ("reserved", C.c_void_p)]


class StageFrameLayers(C.Structure):
    """one frame of bcd_hip_bayes_accumulate_temporal_layers"""
    _c_name_ = "bcd_hip_stage_frame_layers"
    _fields_ = [("d_colors", C.POINTER(C.c_void_p)), ("d_pixel_cov", C.POINTER(C.c_void_p)), ("d_mask", C.c_void_p)]


class WarpedFrame(C.Structure):
    """the destination of bcd_hip_warp_frame"""
    _c_name_ = "bcd_hip_warped_frame"
    _fields_ = [("d_colors", C.c_void_p), ("d_nsamples", C.c_void_p), ("d_histograms", C.c_void_p), ("d_covariances", C.c_void_p)]


class GuideImages(C.Structure):
    """the feature and variance images of one neighbour frame of bcd_hip_denoise_temporal_guided[_host] ("Features")"""
    _c_name_ = "bcd_hip_guide_images"
    _fields_ = [("features", C.c_void_p), ("variances", C.c_void_p)]


class SequenceMode(C.Structure):
    """the mode of bcd_hip_sequence_create_mode ("Modes"); feature_floors: the address of a HOST array of nb_features floats"""
    _c_name_ = "bcd_hip_sequence_mode"
    _fields_ = [("nb_layers", C.c_int32), ("moments", C.c_int32), ("var_floor", C.c_float), ("nb_features", C.c_int32), ("feature_variances", C.c_int32),
                ("feature_floors", C.c_void_p), ("feature_threshold", C.c_float), ("reserved", C.c_void_p)]


class SequenceFrame(C.Structure):
    """one frame of bcd_hip_sequence_push_frame[_host]; layers: the address of nb_layers FrameLayer records"""
    _c_name_ = "bcd_hip_sequence_frame"
    _fields_ = [("nsamples", C.c_void_p), ("histograms", C.c_void_p), ("layers", C.c_void_p), ("features", C.c_void_p), ("variances", C.c_void_p),
                ("reserved", C.c_void_p)]


class SequenceModeInfo(C.Structure):
    """what bcd_hip_sequence_mode_info reports"""
    _c_name_ = "bcd_hip_sequence_mode_info"
    _fields_ = [("nb_layers", C.c_int32), ("moments", C.c_int32), ("nb_features", C.c_int32), ("feature_variances", C.c_int32),
                ("cross_feature_passes", C.c_int64), ("reserved", C.c_int64)]


class BandJob(C.Structure):
    _c_name_ = "bcd_hip_band_job"
    _fields_ = [("d_colors", C.c_void_p), ("d_nsamples", C.c_void_p), ("d_histograms", C.c_void_p), ("d_covariances", C.c_void_p),
                ("W", C.c_int32), ("H", C.c_int32), ("D", C.c_int32), ("main_row_begin", C.c_int32), ("main_row_end", C.c_int32),
                ("order_seed", C.c_uint32), ("d_sum", C.c_void_p), ("d_count", C.c_void_p)]


class MultiStats(C.Structure):
    _c_name_ = "bcd_hip_multi_stats"
    _fields_ = [("n_ranks", C.c_int32), ("transport", C.c_int32), ("frames", C.c_int64), ("marking_rounds", C.c_int32 * 8), ("compute_ms", C.c_float)]


MULTI_ID_BYTES = 128  # BCD_HIP_MULTI_ID_BYTES


class HostOptions(C.Structure):
    _c_name_ = "bcd_hip_host_options"
    _fields_ = [("spike_factor", C.c_float), ("zero_bad_values", C.c_int32)]


class HostLayer(C.Structure):
    _c_name_ = "bcd_hip_host_layer"
    _fields_ = [("h_colors", C.c_void_p), ("h_covariances", C.c_void_p), ("h_out", C.c_void_p)]


class LayersHostOptions(C.Structure):
    _c_name_ = "bcd_hip_layers_host_options"
    _fields_ = [("spike_factor", C.c_float), ("zero_bad_values", C.c_int32), ("filter_layers", C.c_int32)]


class StageLayer(C.Structure):
    """one layer of bcd_hip_bayes_accumulate_layers"""
    _c_name_ = "bcd_hip_stage_layer"
    _fields_ = [("d_colors", C.c_void_p), ("d_pixel_cov", C.c_void_p), ("d_sum", C.c_void_p)]


class SpikeLayer(C.Structure):
    _c_name_ = "bcd_hip_spike_layer"
    _fields_ = [("d_colors", C.c_void_p), ("d_covariances", C.c_void_p), ("d_colors_out", C.c_void_p), ("d_covariances_out", C.c_void_p)]


class SpikeLayerInplace(C.Structure):
    _c_name_ = "bcd_hip_spike_layer_inplace"
    _fields_ = [("d_colors", C.c_void_p), ("d_covariances", C.c_void_p)]


class TemporalHostOptions(C.Structure):
    _c_name_ = "bcd_hip_temporal_host_options"
    _fields_ = [("spike_factor", C.c_float), ("reserved", C.c_void_p)]


class PlanParams(C.Structure):
    """adaptive sample planning, bcd_hip_accum_plan"""
    _c_name_ = "bcd_hip_plan_params"
    _fields_ = [("threshold", C.c_float), ("eps", C.c_float), ("min_samples", C.c_float), ("max_per_pixel", C.c_int32)]


class PlanSummary(C.Structure):
    _c_name_ = "bcd_hip_plan_summary"
    _fields_ = [("planned", C.c_int64), ("active", C.c_int64), ("unsampled", C.c_int64), ("max_error", C.c_float)]


class StateHeader(C.Structure):
    """the 64-byte header of a serialised accumulator state (format v1, include/bcd_hip.h)"""
    _c_name_ = "bcd_hip_accum_state_header"
    _fields_ = [("magic", C.c_char * 8), ("version", C.c_uint32), ("header_bytes", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32),
                ("nb_bins", C.c_int32), ("gamma", C.c_float), ("max_value", C.c_float), ("nb_planes", C.c_uint32),
                ("samples_added", C.c_int64), ("dropped", C.c_int64), ("reserved", C.c_uint8 * 8)]


STATE_HEADER_BYTES = 64  # BCD_HIP_ACCUM_STATE_HEADER_BYTES, BCD_HIP_ACCUM_LAYERS_HEADER_BYTES, BCD_HIP_ACCUM_FEATURES_HEADER_BYTES
ACCUM_MAX_LAYERS = MAX_LAYERS - 1  # BCD_HIP_ACCUM_MAX_LAYERS


class LayersHeader(C.Structure):
    """the 64-byte header of a serialised layer block (version 1, include/bcd_hip.h)"""
    _c_name_ = "bcd_hip_accum_layers_header"
    _fields_ = [("magic", C.c_char * 8), ("version", C.c_uint32), ("header_bytes", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32),
                ("nb_layers", C.c_int32), ("nb_planes", C.c_uint32), ("reserved", C.c_uint8 * 32)]


ACCUM_MAX_FEATURES = 8  # BCD_HIP_ACCUM_MAX_FEATURES (= BCD_HIP_GUIDE_MAX_CHANNELS)


class FeaturesHeader(C.Structure):
    """the 64-byte header of a serialised feature block (version 1, include/bcd_hip.h)"""
    _c_name_ = "bcd_hip_accum_features_header"
    _fields_ = [("magic", C.c_char * 8), ("version", C.c_uint32), ("header_bytes", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32),
                ("nb_features", C.c_int32), ("nb_planes", C.c_uint32), ("reserved", C.c_uint8 * 32)]


class HostStreamResult(C.Structure):
    _c_name_ = "bcd_hip_host_stream_result"
    _fields_ = [("rows_filtered", C.c_int32), ("tile_rows_done", C.c_int32), ("chunk_lines", C.c_int32), ("chunks_done", C.c_int32),
                ("range_flag", C.c_int32), ("uni_n", C.c_float), ("ratio_form", C.c_int32)]


PROGRESS_FN = C.CFUNCTYPE(None, C.c_float, C.c_void_p)  # bcd_hip_progress_fn

I, U32, I64, U64, LL, F, P, STR = C.c_int, C.c_uint32, C.c_int64, C.c_uint64, C.c_longlong, C.c_float, C.c_void_p, C.c_char_p
S = C.POINTER

PROTOTYPES = {
    # ---- context
    "bcd_hip_ctx_create": (I, [P, I, P]),
    "bcd_hip_ctx_destroy": (None, [P]),
    "bcd_hip_last_error": (STR, [P]),
    "bcd_hip_device_count": (I, []),
    "bcd_hip_default_params": (None, [S(Params)]),
    "bcd_hip_set_profiling": (I, [P, I]),
    "bcd_hip_set_concurrent_scales": (I, [P, I]),
    "bcd_hip_set_fast_similarity": (I, [P, I]),
    "bcd_hip_set_margin_planes": (I, [P, I]),
    "bcd_hip_set_strict_eigensolver": (I, [I]),
    "bcd_hip_set_fused_prepare_solve": (I, [I]),
    "bcd_hip_set_cu_share": (I, [P, I]),
    "bcd_hip_set_progress_callback": (I, [P, PROGRESS_FN, P]),
    "bcd_hip_get_stats": (I, [P, I, S(ScaleStats)]),
    "bcd_hip_kernel_time": (I, [P, P, P]),
    "bcd_hip_reset_kernel_time": (I, [P]),
    # ---- whole path, device-resident inputs (what bench.py times)
    "bcd_hip_denoise": (I, [P, P, P, P, P, I, I, I, I, S(Params), P]),
    "bcd_hip_denoise_begin": (I, [P, P, P, P, P, I, I, I, I, S(Params), P]),
    "bcd_hip_denoise_wait": (I, [P]),
    # ---- several colour layers, one similar-patch selection
    "bcd_hip_denoise_layers": (I, [P, P, P, I, I, I, I, S(Params), S(Layer), I]),
    "bcd_hip_layer_spectral_inverses": (I, [P, I, I, P]),
    # ---- a frame's selection, kept
    "bcd_hip_selection_create": (I, [P, P]),
    "bcd_hip_selection_destroy": (None, [P]),
    "bcd_hip_denoise_layers_keep": (I, [P, P, P, I, I, I, I, S(Params), S(Layer), I, P]),
    "bcd_hip_selection_denoise": (I, [P, P, S(Layer), I]),
    "bcd_hip_selection_info": (I, [P, S(SelectionInfo)]),
    "bcd_hip_selection_read": (I, [P, I, P, P, P, P]),
    # ---- similar patches from means and covariances, without histograms
    "bcd_hip_similarity_masks_moments": (I, [P, P, P, I, I, I, I, F, F, P, P]),
    "bcd_hip_window_distances_moments": (I, [P, P, P, I, I, I, I, F, I, I, P]),
    "bcd_hip_denoise_moments": (I, [P, P, I, I, I, S(Params), F, S(Layer), I, P]),
    # ---- the selection gated by auxiliary feature buffers
    "bcd_hip_similarity_masks_guide": (I, [P, S(Guide), I, I, I, I, P, P]),
    "bcd_hip_window_distances_guide": (I, [P, S(Guide), I, I, I, I, I, I, P]),
    "bcd_hip_gate_masks": (I, [P, P, P, P, I, I, I]),
    "bcd_hip_denoise_guided": (I, [P, P, P, I, I, I, I, S(Params), F, S(Layer), I, S(Guide), P]),
    # ---- similar patches from a neighbouring frame of a sequence
    "bcd_hip_denoise_temporal": (I, [P, P, P, P, P, S(Frame), I, I, I, I, I, S(Params), P]),
    "bcd_hip_denoise_temporal_host": (I, [P, P, P, P, P, S(Frame), I, I, I, I, I, S(Params), P]),
    "bcd_hip_bayes_accumulate_temporal": (I, [P, S(StageFrame), I, P, P, I, I, I, I, F, P, P]),
    "bcd_hip_similarity_masks_cross": (I, [P, P, P, P, P, I, I, I, I, I, F, P, P]),
    "bcd_hip_window_distances_cross": (I, [P, P, P, P, P, I, I, I, I, I, I, I, P]),
    # ---- a sequence denoised through a sliding window that reuses cross masks ("Sequences")
    "bcd_hip_transpose_masks_cross": (I, [P, P, I, I, I, P, P]),
    "bcd_hip_sequence_create": (I, [P, I, I, I, I, I, S(Params), P]),
    "bcd_hip_sequence_push": (I, [P, P, P, P, P]),
    "bcd_hip_sequence_push_host": (I, [P, P, P, P, P]),
    "bcd_hip_sequence_end": (I, [P]),
    "bcd_hip_sequence_ready": (I, [P]),
    "bcd_hip_sequence_pop": (I, [P, P, P]),
    "bcd_hip_sequence_pop_host": (I, [P, P, P]),
    "bcd_hip_sequence_set_reuse": (I, [P, I]),
    "bcd_hip_sequence_last_masks": (I, [P, I, I, P, P]),
    "bcd_hip_sequence_info": (I, [P, S(SequenceInfo)]),
    "bcd_hip_sequence_reset": (I, [P]),
    "bcd_hip_sequence_destroy": (None, [P]),
    # ---- the colour layers of a frame denoised with its neighbour frames ("Layers")
    "bcd_hip_denoise_temporal_layers": (I, [P, P, P, S(FrameLayers), I, I, I, I, I, S(Params), S(Layer), I]),
    "bcd_hip_denoise_temporal_layers_host": (I, [P, P, P, S(FrameLayers), I, I, I, I, I, S(Params), S(Layer), I]),
    "bcd_hip_bayes_accumulate_temporal_layers": (I, [P, S(StageFrameLayers), I, I, P, P, I, I, I, I, F, P, P, P]),
    # ---- motion: neighbour frames reprojected by a motion field before the cross passes ("Motion")
    "bcd_hip_denoise_temporal_motion": (I, [P, P, P, P, P, S(Frame), I, P, I, I, I, I, S(Params), P]),
    "bcd_hip_denoise_temporal_motion_host": (I, [P, P, P, P, P, S(Frame), I, P, I, I, I, I, S(Params), P]),
    "bcd_hip_denoise_temporal_layers_motion": (I, [P, P, P, S(FrameLayers), I, P, I, I, I, I, S(Params), S(Layer), I]),
    "bcd_hip_denoise_temporal_layers_motion_host": (I, [P, P, P, S(FrameLayers), I, P, I, I, I, I, S(Params), S(Layer), I]),
    "bcd_hip_warp_frame": (I, [P, S(Frame), P, I, I, I, S(WarpedFrame), P]),
    "bcd_hip_warp_layers": (I, [P, S(FrameLayer), I, P, I, I, P, P]),
    "bcd_hip_valid_downscale": (I, [P, P, I, I, P]),
    "bcd_hip_gate_masks_valid": (I, [P, P, P, P, I, I, I, I]),
    # ---- features: the cross-frame selection gated by auxiliary feature buffers ("Features")
    "bcd_hip_denoise_temporal_guided": (I, [P, P, P, S(FrameLayers), I, P, I, I, I, I, S(Params), S(Layer), I, S(Guide), S(GuideImages)]),
    "bcd_hip_denoise_temporal_guided_host": (I, [P, P, P, S(FrameLayers), I, P, I, I, I, I, S(Params), S(Layer), I, S(Guide), S(GuideImages)]),
    "bcd_hip_similarity_masks_guide_cross": (I, [P, S(Guide), S(GuideImages), I, I, I, I, P, P]),
    "bcd_hip_window_distances_guide_cross": (I, [P, S(Guide), S(GuideImages), I, I, I, I, I, I, P]),
    "bcd_hip_warp_features": (I, [P, S(GuideImages), I, P, I, I, P, P, P]),
    # ---- moments: the cross-frame selection from means and covariances, without histograms ("Moments")
    "bcd_hip_similarity_masks_moments_cross": (I, [P, P, P, P, P, I, I, I, I, F, F, I, P, P]),
    "bcd_hip_window_distances_moments_cross": (I, [P, P, P, P, P, I, I, I, I, F, I, I, P]),
    "bcd_hip_denoise_temporal_moments": (I, [P, P, S(FrameLayers), I, P, I, I, I, S(Params), F, S(Layer), I, S(Guide), S(GuideImages)]),
    "bcd_hip_denoise_temporal_moments_host": (I, [P, P, S(FrameLayers), I, P, I, I, I, S(Params), F, S(Layer), I, S(Guide), S(GuideImages)]),
    # ---- sequences in a mode: colour layers, the moment selection, the feature gate ("Modes")
    "bcd_hip_sequence_create_mode": (I, [P, I, I, I, I, I, S(Params), S(SequenceMode), P]),
    "bcd_hip_sequence_push_frame": (I, [P, S(SequenceFrame)]),
    "bcd_hip_sequence_push_frame_host": (I, [P, S(SequenceFrame)]),
    "bcd_hip_sequence_pop_layers": (I, [P, P, I, P]),
    "bcd_hip_sequence_pop_layers_host": (I, [P, P, I, P]),
    "bcd_hip_sequence_mode_info": (I, [P, S(SequenceModeInfo)]),
    # ---- the spike prefilter in every frame of temporal calls and sequences ("Prefilter")
    "bcd_hip_denoise_temporal_host_ex": (I, [P, P, P, S(FrameLayers), I, P, I, I, I, I, S(Params), F, S(Layer), I, S(Guide), S(GuideImages), S(TemporalHostOptions)]),
    "bcd_hip_sequence_set_prefilter": (I, [P, F]),
    "bcd_hip_sequence_prefilter_info": (I, [P, P, P]),
    # ---- sequences that take per-step motion fields ("Sequences with motion")
    "bcd_hip_compose_motion": (I, [P, P, P, I, I, P]),
    "bcd_hip_sequence_push_frame_motion": (I, [P, S(SequenceFrame), P, P]),
    "bcd_hip_sequence_push_frame_motion_host": (I, [P, S(SequenceFrame), P, P]),
    "bcd_hip_sequence_motion_info": (I, [P, P, P]),
    # (row bands, for multi-GPU tiling)
    "bcd_hip_denoise_band": (I, [P, P, P, P, P, I, I, I, I, I, S(Params), U32, P, P]),
    "bcd_hip_denoise_bands": (I, [P, S(BandJob), I, S(Params)]),
    # ---- one frame over several GPUs of a node (what bcd::Denoiser::setDevices / bcd_cli --devices use)
    "bcd_hip_multi_create": (I, [P, P, I]),
    "bcd_hip_multi_destroy": (None, [P]),
    "bcd_hip_multi_last_error": (STR, [P]),
    "bcd_hip_multi_get_stats": (I, [P, S(MultiStats)]),
    "bcd_hip_multi_set_progress_callback": (I, [P, PROGRESS_FN, P]),
    "bcd_hip_multi_set_frame_timeout": (I, [P, I]),
    "bcd_hip_multi_set_comm_trace": (I, [P, I]),
    "bcd_hip_multi_get_comm_trace": (I, [P, I, P, I]),
    "bcd_hip_multi_denoise_host": (I, [P, P, P, P, P, I, I, I, I, S(Params), P]),
    "bcd_hip_multi_unique_id": (I, [P]),
    "bcd_hip_multi_rccl_info": (I, [P, I]),
    "bcd_hip_multi_create_rank": (I, [P, I, I, I, P, I]),
    "bcd_hip_multi_rank_configure": (I, [P, I, I, I, I, S(Params), P, P, P, P]),
    "bcd_hip_multi_rank_upload": (I, [P, P, P, P, P]),
    "bcd_hip_multi_rank_step": (I, [P]),
    "bcd_hip_multi_rank_download": (I, [P, P]),
    "bcd_hip_multi_rank_renew_ids": (I, [P, P, I]),
    "bcd_hip_multi_set_loopback": (I, [P, I]),
    "bcd_hip_multi_selftest_transport": (I, [I, LL, P, I]),
    # ---- whole path, host buffers (what bcd::Denoiser / bcd_cli call): H2D + denoise + D2H
    "bcd_hip_denoise_host": (I, [P, P, P, P, P, I, I, I, I, S(Params), P]),
    "bcd_hip_denoise_host_ex": (I, [P, P, P, P, P, I, I, I, I, S(Params), S(HostOptions), P]),
    "bcd_hip_denoise_layers_host": (I, [P, P, P, I, I, I, I, S(Params), S(HostOptions), S(HostLayer), I]),
    "bcd_hip_denoise_layers_host_ex": (I, [P, P, P, I, I, I, I, S(Params), S(LayersHostOptions), S(HostLayer), I]),
    "bcd_hip_denoise_moments_host": (I, [P, P, I, I, I, S(Params), S(LayersHostOptions), F, S(HostLayer), I]),
    "bcd_hip_denoise_guided_host": (I, [P, P, P, I, I, I, I, S(Params), S(LayersHostOptions), F, S(HostLayer), I, S(Guide)]),
    "bcd_hip_last_upload_bytes": (I, [P, P, P]),
    "bcd_hip_selftest_pack32": (I, [P, P, P, P]),
    # ---- stages (device pointers) -- exposed for parity tests and multi-GPU composition
    "bcd_hip_scale_begin": (I, [P, P, P, I, I, P, P, P]),
    "bcd_hip_pixel_cov": (I, [P, P, P, I, I, P]),
    "bcd_hip_similarity_masks": (I, [P, P, P, I, I, I, I, I, F, P, P]),
    "bcd_hip_similarity_masks_deferred": (I, [P, P, P, I, I, I, I, I, F, P, P]),
    "bcd_hip_similarity_masks_verdict": (I, [P, P]),
    "bcd_hip_similarity_masks_exact": (I, [P, P, P, I, I, I, I, I, F, P, P]),
    "bcd_hip_similarity_last_path": (I, [P, P, P, P]),
    "bcd_hip_window_distances": (I, [P, P, P, I, I, I, I, I, I, I, P]),
    "bcd_hip_active_set": (I, [P, P, P, I, I, I, I, I, I, F, I, U32, P, P]),
    "bcd_hip_active_init": (I, [P, P, I, I, I, I, I, F, U32, I, P]),
    "bcd_hip_active_step": (I, [P, P, P, I, I, I, I, I, I, I, U32, I, I, P, P]),
    "bcd_hip_active_step_enqueue": (I, [P, P, P, I, I, I, I, I, I, I, U32, I, P, P, I]),
    "bcd_hip_active_step_collect": (I, [P, P, P]),
    "bcd_hip_bayes_accumulate": (I, [P, P, P, P, P, P, I, I, I, I, F, P, P]),
    "bcd_hip_bayes_last_redo_count": (I, [P, P]),
    "bcd_hip_bayes_accumulate_layers": (I, [P, S(StageLayer), I, P, P, P, I, I, I, I, F, P, P]),
    "bcd_hip_layers_pixel_cov": (I, [P, P, I, P, I, I, P, P]),
    "bcd_hip_layers_finalize": (I, [P, P, P, I, P, I64]),
    "bcd_hip_layers_downscale_avg": (I, [P, P, P, I, I, I]),
    "bcd_hip_layers_downscale_cov": (I, [P, P, P, I, P, I, I]),
    "bcd_hip_layers_merge": (I, [P, P, P, I, I, I]),
    "bcd_hip_bayes_accumulate_rows": (I, [P, P, P, P, P, P, I, I, I, I, F, P, P, I, I, P, P, P]),
    "bcd_hip_finalize": (I, [P, P, P, I64, P]),
    "bcd_hip_finalize_band": (I, [P, P, P, I, I, I, P, P, P, P, P]),
    "bcd_hip_downscale_sum": (I, [P, P, I, I, I, P]),
    "bcd_hip_downscale_avg": (I, [P, P, I, I, I, P]),
    "bcd_hip_downscale_cov": (I, [P, P, P, I, I, P]),
    "bcd_hip_interpolate": (I, [P, P, I, I, I, P, I, I]),
    "bcd_hip_merge": (I, [P, P, I, I, P, I]),
    "bcd_hip_spike_filter": (I, [P, P, P, P, P, I, I, I, F, P, P, P, P]),
    # ---- the spike prefilter through a source map
    "bcd_hip_spike_map": (I, [P, P, I, I, F, P, P]),
    "bcd_hip_spike_apply": (I, [P, P, I, I, I, P, P, I]),
    "bcd_hip_spike_filter_layers": (I, [P, P, P, I, I, I, F, P, P, S(SpikeLayer), I, P, P]),
    "bcd_hip_spike_apply_inplace": (I, [P, P, I, I, P, P, I, P]),
    "bcd_hip_spike_filter_layers_inplace": (I, [P, P, P, I, I, I, F, S(SpikeLayerInplace), I, P, P]),
    # (SamplesAccumulator: a whole frame at once, then the persistent device accumulator)
    "bcd_hip_accumulate_samples": (I, [P, P, P, I, I, I, I, F, F, P, P, P, P]),
    "bcd_hip_accum_create": (I, [P, I, I, I, F, F, I64, P]),
    "bcd_hip_accum_destroy": (None, [P]),
    "bcd_hip_accum_reset": (I, [P]),
    "bcd_hip_accum_add_dense": (I, [P, P, P, I, I, I, I]),
    "bcd_hip_accum_add_scattered": (I, [P, P, P, P, I64]),
    "bcd_hip_accum_statistics": (I, [P, P, P, P, P]),
    "bcd_hip_accum_moments": (I, [P, P, P, P]),
    "bcd_hip_accum_info": (I, [P, P, P]),
    # (splatting through a pixel reconstruction filter)
    "bcd_hip_accum_set_filter": (I, [P, F, F, I, P]),
    "bcd_hip_accum_add_splatted": (I, [P, P, P, P, I64]),
    "bcd_hip_filter_table": (I, [I, F, F, F, I, P]),
    # (adaptive sample planning)
    "bcd_hip_default_plan_params": (None, [S(PlanParams)]),
    "bcd_hip_accum_plan": (I, [P, S(PlanParams), I64, U64, P, P, P, I64, S(PlanSummary)]),
    # (accumulator states: export, import, merge)
    "bcd_hip_accum_state_info": (I, [P, I64, S(StateHeader)]),
    "bcd_hip_accum_state_bytes": (I, [P, P]),
    "bcd_hip_accum_export": (I, [P, P, I64]),
    "bcd_hip_accum_import": (I, [P, P, I64]),
    "bcd_hip_accum_merge_state": (I, [P, P, I64]),
    "bcd_hip_accum_merge": (I, [P, P]),
    # (colour layers beside the beauty)
    "bcd_hip_accum_create_layers": (I, [P, I, I, I, F, F, I64, I, P]),
    "bcd_hip_accum_nb_layers": (I, [P, P]),
    "bcd_hip_accum_add_dense_layers": (I, [P, P, P, I, I, I, I, P, I]),
    "bcd_hip_accum_add_scattered_layers": (I, [P, P, P, P, I64, P]),
    "bcd_hip_accum_add_splatted_layers": (I, [P, P, P, P, I64, P]),
    "bcd_hip_accum_layer_statistics": (I, [P, P, P]),
    "bcd_hip_accum_layers_state_info": (I, [P, I64, S(LayersHeader)]),
    "bcd_hip_accum_layers_state_bytes": (I, [P, P]),
    "bcd_hip_accum_export_layers": (I, [P, P, I64]),
    "bcd_hip_accum_import_layers": (I, [P, P, I64]),
    "bcd_hip_accum_merge_layers_state": (I, [P, P, I64]),
    # (auxiliary feature channels beside the beauty)
    "bcd_hip_accum_create_features": (I, [P, I, I, I, F, F, I64, I, I, P]),
    "bcd_hip_accum_nb_features": (I, [P, P]),
    "bcd_hip_accum_add_dense_features": (I, [P, P, P, I, I, I, I, P, I, P]),
    "bcd_hip_accum_add_scattered_features": (I, [P, P, P, P, I64, P, P]),
    "bcd_hip_accum_add_splatted_features": (I, [P, P, P, P, I64, P, P]),
    "bcd_hip_accum_feature_statistics": (I, [P, P, P]),
    "bcd_hip_accum_features_state_info": (I, [P, I64, S(FeaturesHeader)]),
    "bcd_hip_accum_features_state_bytes": (I, [P, P]),
    "bcd_hip_accum_export_features": (I, [P, P, I64]),
    "bcd_hip_accum_import_features": (I, [P, P, I64]),
    "bcd_hip_accum_merge_features_state": (I, [P, P, I64]),
    "bcd_hip_zero_bad_values": (I, [P, P, I64]),
    # (self-tests and measurement aids)
    "bcd_hip_selftest_division": (I, [P, U32, I64, P]),
    "bcd_hip_selftest_distance_kernels": (I, [P, P, P, I, I, I, I, P, P]),
    "bcd_hip_selftest_bin_work": (I, [P, P, P, I, I, I, I, I, P, P, P, P]),
    "bcd_hip_selftest_approx_distance": (I, [P, P, P, I, I, I, I, P, P, P]),
    "bcd_hip_selftest_active_lists": (I, [P, P, P, I, I, I, I, I, P, P, P, P]),
    # ---- the host-buffer upload path piece by piece (self-tests; what the host-buffer entry points run, not copies of it)
    "bcd_hip_selftest_sparse_upload": (I, [P, P, I64, P, I, I64, P, P]),
    "bcd_hip_selftest_host_stream": (I, [P, P, P, P, P, I, I, I, S(Params), F, I, I, P, P, P, P, P, P, P, S(HostStreamResult)]),
    "bcd_hip_approx_planes": (I, [P, P, P, I, I, I, I, F, I, F, P, P, P]),
    "bcd_hip_eig27_batch": (I, [P, P, I, P, P, P]),
    "bcd_hip_eig27_batch_rule": (I, [P, P, I, P, P, P, I]),
    "bcd_hip_selftest_prepare_solve": (I, [P, P, P, P, P, I, I, I, I, I, I, P]),
    # ---- host utilities (no device work)
    "bcd_hip_visit_order": (I, [I, I, I, I, U32, P]),
    "bcd_hip_strip_order_seed": (U32, [I, I, I, I]),
    "bcd_hip_scale_seed": (U32, [U32, I]),
}


def apply(lib):
    """declares every entry point the loaded library exports (an older or instrumented build may lack some: those are skipped)"""
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
