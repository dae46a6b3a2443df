"""ctypes binding of include/bcd_hip.h.  Fails loudly when libbcd_hip.so is missing: there is no CPU fallback.
The structures and the prototype of every entry point are declared in _prototypes.py and applied by lib(): a call site passes plain Python numbers."""
import ctypes as C
import os
import weakref

from . import _prototypes
from ._prototypes import (ACCUM_MAX_FEATURES, ACCUM_MAX_LAYERS, MAX_LAYERS, MULTI_ID_BYTES, PROGRESS_FN, SELECTION_MAX_SCALES, STATE_HEADER_BYTES, BandJob,
                          FeaturesHeader, Frame, FrameLayer, FrameLayers, Guide, GuideImages, HostLayer, HostOptions, HostStreamResult, Layer, LayersHeader, LayersHostOptions, MultiStats, Params,
                          PlanParams, PlanSummary, ScaleStats, SelectionInfo, SelectionScale, SequenceFrame, SequenceInfo, SequenceMode, SequenceModeInfo, SpikeLayer, SpikeLayerInplace, StageFrame, StageFrameLayers, StageLayer,
                          StateHeader, TemporalHostOptions, WarpedFrame)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BCD_HIP_LIB") or os.path.join(_HERE, "lib", "libbcd_hip.so")   # (BCD_HIP_LIB: tools load instrumented builds)

_F = C.POINTER(C.c_float)
_VP = C.c_void_p
_fptr = lambda a: a.ctypes.data_as(_F)    # a NumPy float32 array as a float *

SPIKE_MAX_IMAGES = 32  # images of one bcd_hip_spike_apply call
SYMBOLS = list(_prototypes.PROTOTYPES)    # every symbol include/bcd_hip.h declares (checked by tests/test_abi.py)


def delta_count(b):
    """planes of a search radius b: the half plane of displacements (bcd_delta_count)"""
    return (b + 1) + b * (2 * b + 1)


def _state_buffer(buf):
    """a contiguous uint8 numpy view of a serialised state (numpy array, bytes, bytearray, memoryview, mmap)"""
    import numpy as np
    a = buf if isinstance(buf, np.ndarray) else np.frombuffer(buf, np.uint8)
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def accum_state_info(buf):
    """the header of a serialised accumulator state as a dict (bcd_hip_accum_state_info: host only, no GPU needed); ValueError if the
    buffer is not a well-formed state of its exact size"""
    a = _state_buffer(buf)
    h = StateHeader()
    rc = lib().bcd_hip_accum_state_info(a.ctypes.data_as(_VP) if a.size else None, a.size, C.byref(h))
    if rc != 0:
        raise ValueError("not a serialised accumulator state (format v1) of %d bytes: rc=%d" % (a.size, rc))
    return {"magic": bytes(h.magic), "version": h.version, "header_bytes": h.header_bytes, "width": h.width, "height": h.height,
            "nb_bins": h.nb_bins, "gamma": h.gamma, "max_value": h.max_value, "nb_planes": h.nb_planes,
            "samples_added": h.samples_added, "dropped": h.dropped}


def accum_state_planes(buf):
    """(header dict, float32 (nb_planes, H, W) view of the planes) of a serialised state: weight sum, squared-weight sum, 3 colour sums,
    6 second moments (xx, yy, zz, yz, xz, xy), then the bins channel-major"""
    a = _state_buffer(buf)
    info = accum_state_info(a)
    planes = a[STATE_HEADER_BYTES:].view("<f4").reshape(info["nb_planes"], info["height"], info["width"])
    return info, planes


def accum_layers_state_info(buf):
    """the header of a serialised layer block as a dict (bcd_hip_accum_layers_state_info: host only, no GPU needed); ValueError if the
    buffer is not a well-formed block of its exact size"""
    a = _state_buffer(buf)
    h = LayersHeader()
    rc = lib().bcd_hip_accum_layers_state_info(a.ctypes.data_as(_VP) if a.size else None, a.size, C.byref(h))
    if rc != 0:
        raise ValueError("not a serialised accumulator layer block (version 1) of %d bytes: rc=%d" % (a.size, rc))
    return {"magic": bytes(h.magic), "version": h.version, "header_bytes": h.header_bytes, "width": h.width, "height": h.height,
            "nb_layers": h.nb_layers, "nb_planes": h.nb_planes}


def accum_layers_state_planes(buf):
    """(header dict, float32 (nb_layers, 9, H, W) view of the planes) of a serialised layer block: per layer 3 colour sums, then the 6
    second moments (xx, yy, zz, yz, xz, xy)"""
    a = _state_buffer(buf)
    info = accum_layers_state_info(a)
    return info, a[STATE_HEADER_BYTES:].view("<f4").reshape(info["nb_layers"], 9, info["height"], info["width"])


def accum_features_state_info(buf):
    """the header of a serialised feature block as a dict (bcd_hip_accum_features_state_info: host only, no GPU needed); ValueError if the
    buffer is not a well-formed block of its exact size"""
    a = _state_buffer(buf)
    h = FeaturesHeader()
    rc = lib().bcd_hip_accum_features_state_info(a.ctypes.data_as(_VP) if a.size else None, a.size, C.byref(h))
    if rc != 0:
        raise ValueError("not a serialised accumulator feature block (version 1) of %d bytes: rc=%d" % (a.size, rc))
    return {"magic": bytes(h.magic), "version": h.version, "header_bytes": h.header_bytes, "width": h.width, "height": h.height,
            "nb_features": h.nb_features, "nb_planes": h.nb_planes}


def accum_features_state_planes(buf):
    """(header dict, float32 (nb_features, 2, H, W) view of the planes) of a serialised feature block: per channel the weighted sum, then
    the weighted sum of squares"""
    a = _state_buffer(buf)
    info = accum_features_state_info(a)
    return info, a[STATE_HEADER_BYTES:].view("<f4").reshape(info["nb_features"], 2, info["height"], info["width"])


def default_plan_params(**kw):
    p = PlanParams()
    lib().bcd_hip_default_plan_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


FILTER_KINDS = {"box": 0, "tent": 1, "gaussian": 2, "blackman_harris": 3}


def _radii(radius):
    rx, ry = (radius, radius) if not hasattr(radius, "__len__") else radius
    return float(rx), float(ry)


def filter_table(kind, radius, param=2.0, table_size=16):
    """the (table_size, table_size) float32 table of a standard separable filter (bcd_hip_filter_table: host only, no GPU needed).
    kind: "box", "tent", "gaussian" (param = alpha) or "blackman_harris"; radius: a number or (radius_x, radius_y), each in (0, 3]"""
    import numpy as np
    if kind not in FILTER_KINDS:
        raise ValueError("unknown filter kind %r (one of %s)" % (kind, ", ".join(sorted(FILTER_KINDS))))
    rx, ry = _radii(radius)
    ts = int(table_size)
    out = np.empty((max(ts, 1), max(ts, 1)), np.float32)
    rc = lib().bcd_hip_filter_table(FILTER_KINDS[kind], rx, ry, param, ts, out.ctypes.data_as(_VP))
    if rc != 0:
        raise ValueError("bcd_hip_filter_table(%s, radius (%g, %g), param %g, table_size %d): rc=%d" % (kind, rx, ry, param, ts, rc))
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libbcd_hip.so is not built (%s): run `python -m bcd_amd.build`; "
                               "there is no CPU fallback" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _prototypes.apply(_lib)
    return _lib


# Kept for the test files of the commit before the prototype table, which must go on passing against this module: they reach groups of entry points
# through these helpers (once the places that declared their prototypes) and set bcd_hip_accum_plan's from PLAN_ARGTYPES, in which d_summary is a plain
# address.  Nothing in this tree uses them and new code should not: lib() has every prototype, and the table's entry is the checked one.
_state_api = _layers_api = _splat_api = _rows_api = _selection_api = lib
PLAN_ARGTYPES = _prototypes.PROTOTYPES["bcd_hip_accum_plan"][1][:-1] + [_VP]


def default_params(**kw):
    p = Params()
    lib().bcd_hip_default_params(C.byref(p))
    names = {"tau": "hist_dist_threshold", "w": "patch_radius", "b": "search_radius", "min_eig": "min_eigen_value",
             "random_order": "use_random_pixel_order", "m": "marked_skip_probability", "seed": "order_seed"}
    for k, v in kw.items():
        setattr(p, names.get(k, k), v)
    return p


class BcdHipError(RuntimeError):
    pass


def _dp(t):
    """device pointer of a contiguous torch tensor"""
    assert t.is_cuda and t.is_contiguous(), "expected a contiguous device tensor"
    return C.c_void_p(t.data_ptr())


_dptr = lambda t: _dp(t).value      # ... as an address, for a structure field
_hptr = lambda a: a.ctypes.data     # the address of a NumPy array


def _host_layer_array(layers, H, W, struct=HostLayer):
    """a list of (colours, covariances) NumPy images -> (their `struct` array with fresh outputs, the layers as contiguous float32 arrays, the outputs);
    struct: HostLayer, or Layer for the calls that declare their host layers with it (three pointers either way)"""
    import numpy as np
    layers = [(np.ascontiguousarray(c, np.float32), np.ascontiguousarray(v, np.float32)) for c, v in layers]
    outs = [np.empty((H, W, 3), np.float32) for _ in layers]
    arr = (struct * max(1, len(layers)))()
    for k, ((col, cov), out) in enumerate(zip(layers, outs)):
        if col.shape != (H, W, 3) or cov.shape != (H, W, 6):
            raise ValueError("layer %d: colours must be %dx%dx3 and covariances %dx%dx6" % (k, H, W, H, W))
        arr[k] = struct(col.ctypes.data, cov.ctypes.data, out.ctypes.data)
    return arr, layers, outs


def _mask_and_count(H, W, b, device):
    """zeroed (mask (H, W, words) int32, count (H, W) int32) device tensors of the similarity_masks family: words = ceil((2b+1)^2 / 32)"""
    import torch
    words = ((2 * b + 1) ** 2 + 31) // 32
    return torch.zeros((H, W, words), dtype=torch.int32, device=device), torch.zeros((H, W), dtype=torch.int32, device=device)


class Context:
    """bcd_hip_ctx bound to a torch device/stream."""

    def __init__(self, device=0, stream=None):
        import torch
        self.torch = torch
        self.device = device
        h = _VP()
        st = None
        if stream is not None:
            st = C.c_void_p(stream.cuda_stream)
        rc = lib().bcd_hip_ctx_create(C.byref(h), int(device), st)
        if rc != 0:
            raise BcdHipError("bcd_hip_ctx_create failed: rc=%d" % rc)
        self.h = h
        self._accumulators = weakref.WeakSet()
        self._selections = weakref.WeakSet()

    def close(self):
        if self.h:
            for a in list(self._accumulators) + list(self._selections):   # an accumulator / a selection must not outlive its context (bcd_hip.h)
                a.close()
            lib().bcd_hip_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise BcdHipError("rc=%d: %s" % (rc, lib().bcd_hip_last_error(self.h).decode()))

    # ---- whole path
    def denoise(self, col, ns, hist, cov, nscales, prm, out=None):
        torch = self.torch
        H, W, D = hist.shape
        if out is None:
            out = torch.empty((H, W, 3), dtype=torch.float32, device=hist.device)
        self._chk(lib().bcd_hip_denoise(self.h, _dp(col), _dp(ns), _dp(hist), _dp(cov), W, H, D, nscales, C.byref(prm), _dp(out)))
        return out

    def _layer_array(self, layers, outs, H, W, device):
        """the bcd_hip_layer array of a list of (colours, covariances) tensors and their outputs (fresh ones when `outs` is None)"""
        torch = self.torch
        layers = list(layers)
        if outs is None:
            outs = [torch.empty((H, W, 3), dtype=torch.float32, device=device) for _ in layers]
        outs = list(outs)
        if len(outs) != len(layers):
            raise ValueError("one output per layer expected")
        arr = (Layer * max(1, len(layers)))()
        for k, ((col, cov), out) in enumerate(zip(layers, outs)):
            if tuple(col.shape) != (H, W, 3) or tuple(cov.shape) != (H, W, 6) or tuple(out.shape) != (H, W, 3):
                raise ValueError("layer %d: colours / output must be %dx%dx3 and covariances %dx%dx6" % (k, H, W, H, W))
            arr[k].d_colors, arr[k].d_covariances, arr[k].d_out = _dp(col).value, _dp(cov).value, _dp(out).value
        return arr, layers, outs

    def denoise_layers(self, ns, hist, layers, nscales, prm, outs=None, keep=None):
        """bcd_hip_denoise_layers: `layers` is a list of (colours, covariances) tensors that share `ns` and `hist`; one selection of similar patches
        serves them all.  Returns the list of outputs (`outs`: tensors to write into, optional).  keep: a Selection (Context.selection()) that takes
        the selection of every scale with it (bcd_hip_denoise_layers_keep)"""
        H, W, D = hist.shape
        arr, layers, outs = self._layer_array(layers, outs, H, W, hist.device)
        if keep is None:
            self._chk(lib().bcd_hip_denoise_layers(self.h, _dp(ns), _dp(hist), W, H, D, nscales, C.byref(prm), arr, len(layers)))
        else:
            self._chk(lib().bcd_hip_denoise_layers_keep(self.h, _dp(ns), _dp(hist), W, H, D, nscales, C.byref(prm), arr, len(layers), keep._handle()))
        return outs

    def denoise_moments(self, ns, layers, nscales, prm, var_floor=1e-8, outs=None, keep=None):
        """bcd_hip_denoise_moments: the similar patches are selected from the colours and per-pixel covariances of layers[0] (the guide), no histogram is
        read; `layers` is a list of (colours, covariances) tensors that share `ns`, every one is denoised on the one selection.  keep: a Selection that
        takes the selection of every scale with it.  Returns the list of outputs"""
        layers = list(layers)
        H, W = (layers[0][0].shape[0], layers[0][0].shape[1]) if layers else (ns.shape[0], ns.shape[1])
        arr, layers, outs = self._layer_array(layers, outs, H, W, ns.device)
        self._chk(lib().bcd_hip_denoise_moments(self.h, _dp(ns), W, H, nscales, C.byref(prm), var_floor, arr, len(layers), keep._handle() if keep is not None else None))
        return outs

    def denoise_moments_host(self, ns, layers, nscales, prm, var_floor=1e-8, spike_factor=0.0, zero_bad_values=False, filter_layers=False):
        """bcd_hip_denoise_moments_host on NumPy images: `layers` is a list of (colours, covariances), layers[0] the guide; the options are those of
        denoise_layers_host (the spike prefilter runs without histograms).  Returns the list of outputs"""
        import numpy as np
        ns = np.ascontiguousarray(ns, np.float32)
        H, W = ns.shape[0], ns.shape[1]
        arr, layers, outs = _host_layer_array(layers, H, W)
        opt = LayersHostOptions(spike_factor, 1 if zero_bad_values else 0, 1 if filter_layers else 0)
        self._chk(lib().bcd_hip_denoise_moments_host(self.h, _fptr(ns), W, H, nscales, C.byref(prm), C.byref(opt), var_floor, arr, len(layers)))
        return outs

    def _guide(self, features, variances, floors, threshold, host=False):
        """-> (Guide, objects to keep alive): features / variances are (H, W, F) device tensors (host=True: NumPy arrays), floors F numbers"""
        import numpy as np
        if host:
            features = np.ascontiguousarray(features, np.float32)
            variances = None if variances is None else np.ascontiguousarray(variances, np.float32)
        if features.ndim != 3 or (variances is not None and tuple(variances.shape) != tuple(features.shape)):
            raise ValueError("features must be H x W x F and the variances of the same shape")
        F = int(features.shape[2])
        fl = np.ascontiguousarray(np.asarray(floors, np.float32).reshape(-1))
        if fl.size != F:
            raise ValueError("one floor per feature channel expected")
        ptr = _hptr if host else _dptr
        g = Guide(ptr(features), None if variances is None else ptr(variances), F, _fptr(fl), float(threshold))
        return g, (features, variances, fl)

    def denoise_guided(self, ns, hist, layers, nscales, prm, features, variances=None, floors=(), threshold=1.0, var_floor=1e-8, outs=None, keep=None):
        """bcd_hip_denoise_guided: denoise_layers (hist given) or denoise_moments (hist None) with the selection gated by the feature buffers:
        features (H, W, F) and optional variances (H, W, F) device tensors, floors F numbers, threshold tau_g.  keep: a Selection.  Returns the outputs"""
        layers = list(layers)
        H, W = ns.shape[0], ns.shape[1]
        D = hist.shape[2] if hist is not None else 0
        arr, layers, outs = self._layer_array(layers, outs, H, W, ns.device)
        if tuple(features.shape[:2]) != (H, W):
            raise ValueError("features must be %dx%dxF" % (H, W))
        g, alive = self._guide(features, variances, floors, threshold)
        self.torch.cuda.synchronize(self.device)                     # (the inputs may have been produced on torch's stream)
        self._chk(lib().bcd_hip_denoise_guided(self.h, _dp(ns), _dp(hist) if hist is not None else None, W, H, D, nscales, C.byref(prm), var_floor, arr,
                                               len(layers), C.byref(g), keep._handle() if keep is not None else None))
        del alive
        return outs

    def denoise_guided_host(self, ns, hist, layers, nscales, prm, features, variances=None, floors=(), threshold=1.0, var_floor=1e-8, spike_factor=0.0,
                            zero_bad_values=False, filter_layers=False):
        """bcd_hip_denoise_guided_host on NumPy images: `layers` is a list of (colours, covariances); hist None selects from means and covariances.
        Returns the list of outputs"""
        import numpy as np
        ns = np.ascontiguousarray(ns, np.float32)
        H, W = ns.shape[0], ns.shape[1]
        hist = None if hist is None else np.ascontiguousarray(hist, np.float32)
        D = hist.shape[2] if hist is not None else 0
        arr, layers, outs = _host_layer_array(layers, H, W)
        g, alive = self._guide(features, variances, floors, threshold, host=True)
        if tuple(alive[0].shape[:2]) != (H, W):
            raise ValueError("features must be %dx%dxF" % (H, W))
        opt = LayersHostOptions(spike_factor, 1 if zero_bad_values else 0, 1 if filter_layers else 0)
        self._chk(lib().bcd_hip_denoise_guided_host(self.h, _fptr(ns), _fptr(hist) if hist is not None else None, W, H, D, nscales,
                                                    C.byref(prm), C.byref(opt), var_floor, arr, len(layers), C.byref(g)))
        del alive
        return outs

    def selection(self):
        """an empty Selection of this context (bcd_hip_selection_create); denoise_layers(..., keep=sel) fills it"""
        return Selection(self)

    def layer_spectral_inverses(self, scale, layer):
        """full estimates of one layer of the last denoise_layers call that took the spectral inverse (stats().spectral_inverses is their sum)"""
        n = C.c_int32(0)
        self._chk(lib().bcd_hip_layer_spectral_inverses(self.h, scale, layer, C.byref(n)))
        return n.value

    def denoise_begin(self, col, ns, hist, cov, nscales, prm, out):
        """bcd_hip_denoise_begin: returns at once; the tensors must stay alive and untouched until denoise_wait()"""
        H, W, D = hist.shape
        self._chk(lib().bcd_hip_denoise_begin(self.h, _dp(col), _dp(ns), _dp(hist), _dp(cov), W, H, D, nscales, C.byref(prm), _dp(out)))
        self._inflight = (col, ns, hist, cov, out, prm)   # (kept alive until denoise_wait; a refused call leaves the frame in flight alone)

    def denoise_wait(self):
        self._chk(lib().bcd_hip_denoise_wait(self.h))
        out = self._inflight[4] if getattr(self, "_inflight", None) else None
        self._inflight = None
        return out

    def denoise_band(self, col, ns, hist, cov, row_begin, row_end, prm, seed, sum_, cnt):
        H, W, D = hist.shape
        self._chk(lib().bcd_hip_denoise_band(self.h, _dp(col), _dp(ns), _dp(hist), _dp(cov), W, H, D, row_begin, row_end,
                                             C.byref(prm), seed, _dp(sum_), _dp(cnt)))

    def denoise_bands(self, jobs, prm):
        """jobs: list of (col, ns, hist, cov, row_begin, row_end, seed, sum, cnt) device tensors; run concurrently"""
        arr = (BandJob * len(jobs))()
        for i, (col, ns, hist, cov, r0, r1, seed, s, c) in enumerate(jobs):
            H, W, D = hist.shape
            arr[i] = BandJob(_dp(col).value, _dp(ns).value, _dp(hist).value, _dp(cov).value, W, H, D, r0, r1, seed, _dp(s).value, _dp(c).value)
        self._chk(lib().bcd_hip_denoise_bands(self.h, arr, len(jobs), C.byref(prm)))

    def denoise_host(self, col, ns, hist, cov, nscales, prm, spike_factor=0.0, zero_bad_values=False):
        import numpy as np
        H, W, D = hist.shape
        out = np.empty((H, W, 3), np.float32)
        opt = HostOptions(spike_factor, 1 if zero_bad_values else 0)
        self._chk(lib().bcd_hip_denoise_host_ex(self.h, _fptr(col), _fptr(ns), _fptr(hist), _fptr(cov), W, H, D, nscales, C.byref(prm), C.byref(opt), _fptr(out)))
        return out

    def denoise_layers_host(self, ns, hist, layers, nscales, prm, spike_factor=0.0, zero_bad_values=False, filter_layers=False):
        """bcd_hip_denoise_layers_host_ex on NumPy images: `layers` is a list of (colours, covariances); layers[0] is the primary layer.  filter_layers:
        the spike prefilter (spike_factor > 0) covers every layer, gathered through the source map of the primary colours; without it a factor beside
        several layers is refused.  Returns the list of outputs"""
        H, W, D = hist.shape
        arr, layers, outs = _host_layer_array(layers, H, W)
        opt = LayersHostOptions(spike_factor, 1 if zero_bad_values else 0, 1 if filter_layers else 0)
        self._chk(lib().bcd_hip_denoise_layers_host_ex(self.h, _fptr(ns), _fptr(hist), W, H, D, nscales, C.byref(prm), C.byref(opt), arr, len(layers)))
        return outs

    def last_upload_bytes(self):
        """(bytes of the histogram image of the last denoise_host call, bytes of it that crossed PCIe)"""
        a, b = C.c_int64(0), C.c_int64(0)
        self._chk(lib().bcd_hip_last_upload_bytes(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def selftest_sparse_upload(self, src, dst=None, new_frame=True, piece_floats=0):
        """bcd_hip_selftest_sparse_upload: the float32 / uint32 numpy array `src` through the context's sparse uploader into the device tensor `dst`
        (same number of 4-byte elements, any alignment; default: a fresh tensor) -> (dst, (raw bytes, sent bytes) of the frame so far)"""
        import numpy as np
        torch = self.torch
        assert src.dtype.itemsize == 4 and src.flags["C_CONTIGUOUS"]
        if dst is None:
            dst = torch.empty((max(src.size, 1),), dtype=torch.float32, device="cuda:%d" % self.device)[:src.size]
        assert dst.is_cuda and dst.is_contiguous() and dst.element_size() == 4 and dst.numel() == src.size
        a, b = C.c_int64(0), C.c_int64(0)
        hp = src.ctypes.data_as(_VP) if src.size else np.zeros(1, np.float32).ctypes.data_as(_VP)
        self._chk(lib().bcd_hip_selftest_sparse_upload(self.h, hp, src.size, C.c_void_p(dst.data_ptr()), 1 if new_frame else 0, int(piece_floats),
                                                       C.byref(a), C.byref(b)))
        return dst, (a.value, b.value)

    def selftest_host_stream(self, col, ns, hist, cov, prm, spike_factor=0.0, stop_after_chunks=-1, poison=True):
        """bcd_hip_selftest_host_stream on host (numpy) images -> dict: planes (nd, H, W) float16, counts (nd, H, W) uint8, images (the four the
        planes were computed on), hist_uploaded, and the fields of bcd_hip_host_stream_result"""
        torch = self.torch
        H, W, D = hist.shape
        dev = "cuda:%d" % self.device
        nd = delta_count(prm.search_radius)
        planes = torch.empty((nd, H, W), dtype=torch.float16, device=dev)
        counts = torch.empty((nd, H, W), dtype=torch.uint8, device=dev)
        imgs = [torch.empty(a.shape, dtype=torch.float32, device=dev) for a in (col, ns, hist, cov)]
        up = torch.empty(hist.shape, dtype=torch.float32, device=dev)
        res = HostStreamResult()
        self._chk(lib().bcd_hip_selftest_host_stream(self.h, _fptr(col), _fptr(ns), _fptr(hist), _fptr(cov), W, H, D, C.byref(prm), spike_factor, int(stop_after_chunks),
                                                     1 if poison else 0, _dp(planes), _dp(counts), *[_dp(t) for t in imgs], _dp(up), C.byref(res)))
        out = {k: getattr(res, k) for k, _ in HostStreamResult._fields_}
        out.update(planes=planes, counts=counts, images=imgs, hist_uploaded=up)
        return out

    def approx_planes(self, hist, ns, b, uni_n, ratio_form=False, tau=1.0, fill=0xFF):
        """bcd_hip_approx_planes on resident tensors -> (planes (nd, H, W) float16, counts (nd, H, W) uint8, range flag); entries the kernel does not
        write (the neighbour lies outside the image) keep the `fill` byte"""
        torch = self.torch
        H, W, D = hist.shape
        nd = delta_count(b)
        planes = torch.full((nd, H, W, 2), fill, dtype=torch.uint8, device=hist.device).view(torch.float16).reshape(nd, H, W)
        counts = torch.full((nd, H, W), fill, dtype=torch.uint8, device=hist.device)
        flag = C.c_int(0)
        self.torch.cuda.synchronize(self.device)                     # (the fills ran on torch's stream)
        self._chk(lib().bcd_hip_approx_planes(self.h, _dp(hist), _dp(ns), W, H, D, int(b), uni_n, 1 if ratio_form else 0, tau, _dp(planes), _dp(counts), C.byref(flag)))
        return planes, counts, flag.value

    def set_progress_callback(self, fn):
        """fn(progress) or None; the ctypes thunk is kept alive on the context"""
        self._progress = PROGRESS_FN(lambda v, user: fn(v)) if fn else C.cast(None, PROGRESS_FN)
        self._chk(lib().bcd_hip_set_progress_callback(self.h, self._progress, None))

    # ---- stages
    def pixel_cov(self, cov, ns):
        H, W, _ = cov.shape
        out = self.torch.empty_like(cov)
        self._chk(lib().bcd_hip_pixel_cov(self.h, _dp(cov), _dp(ns), W, H, _dp(out)))
        return out

    def scale_begin(self, cov, ns):
        """bcd_hip_scale_begin -> (per-pixel covariances, sum image, count image): the accumulators are handed over filled with ones and cleared by
        the call, like every counter of the stage calls that follow on this context"""
        torch = self.torch
        H, W, _ = cov.shape
        pixcov = torch.empty_like(cov)
        s = torch.ones((H, W, 3), dtype=torch.float32, device=cov.device)
        c = torch.ones((H, W), dtype=torch.int32, device=cov.device)
        torch.cuda.synchronize(self.device)                          # (the fills ran on torch's stream)
        self._chk(lib().bcd_hip_scale_begin(self.h, _dp(cov), _dp(ns), W, H, _dp(pixcov), _dp(s), _dp(c)))
        return pixcov, s, c

    def similarity_masks(self, hist, ns, w, b, tau):
        H, W, D = hist.shape
        mask, cnt = _mask_and_count(H, W, b, hist.device)
        self._chk(lib().bcd_hip_similarity_masks(self.h, _dp(hist), _dp(ns), W, H, D, w, b, tau, _dp(mask), _dp(cnt)))
        return mask, cnt

    def similarity_masks_exact(self, hist, ns, w, b, tau):
        """bcd_hip_similarity_masks_exact: the exact planes with the compiler's division, whatever the fast path would do"""
        H, W, D = hist.shape
        mask, cnt = _mask_and_count(H, W, b, hist.device)
        self._chk(lib().bcd_hip_similarity_masks_exact(self.h, _dp(hist), _dp(ns), W, H, D, w, b, tau, _dp(mask), _dp(cnt)))
        return mask, cnt

    def similarity_last_path(self):
        """(path, borderline pairs, list capacity) of the last similarity pass on the main workspace: path 0 exact, 1 approximate, 2 RATIO form"""
        p, n, cap = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._chk(lib().bcd_hip_similarity_last_path(self.h, C.byref(p), C.byref(n), C.byref(cap)))
        return p.value, n.value, cap.value

    def window_distances(self, hist, ns, w, b, line, col):
        import numpy as np
        H, W, D = hist.shape
        out = np.empty(((2 * b + 1) ** 2,), np.float32)
        self._chk(lib().bcd_hip_window_distances(self.h, _dp(hist), _dp(ns), W, H, D, w, b, line, col, _fptr(out)))
        return out

    def similarity_masks_cross(self, hist, ns, hist_nb, ns_nb, w, b, tau, out=None):
        """bcd_hip_similarity_masks_cross: masks and |S_f| of the main pixels of a neighbour frame (hist_nb, ns_nb) similar to each main pixel of the
        frame (hist, ns), in the layouts of similarity_masks.  out: (mask (H, W, words) int32, count (H, W) int32) contiguous device tensors to fill"""
        torch = self.torch
        H, W, D = hist.shape
        if tuple(hist_nb.shape) != (H, W, D) or ns_nb.numel() != H * W or ns.numel() != H * W:
            raise ValueError("the neighbour frame must have the frame's width, height and histogram depth")
        words = ((2 * b + 1) ** 2 + 31) // 32
        if out is None:
            out = _mask_and_count(H, W, b, hist.device)
        mask, cnt = out
        if tuple(mask.shape) != (H, W, words) or tuple(cnt.shape) != (H, W) or mask.dtype != torch.int32 or cnt.dtype != torch.int32:
            raise ValueError("out must be ((H, W, words) int32, (H, W) int32)")
        torch.cuda.synchronize(self.device)                          # (the fills ran on torch's stream)
        self._chk(lib().bcd_hip_similarity_masks_cross(self.h, _dp(hist), _dp(ns), _dp(hist_nb), _dp(ns_nb), W, H, D, w, b, tau, _dp(mask), _dp(cnt)))
        return mask, cnt

    def transpose_masks_cross(self, mask, b, out=None):
        """bcd_hip_transpose_masks_cross: the cross masks of a frame pair with the roles of the frames swapped -- out(p) bit k = mask(p + delta_k) bit
        (nbits - 1 - k) inside the image, else 0 -- and their popcounts.  mask: (H, W, words) int32 as similarity_masks_cross returns it; b: 1 .. 6.
        out: (mask, count) contiguous device tensors to fill, count may be None.  Returns (mask, count)"""
        torch = self.torch
        H, W, words = mask.shape
        if out is None:
            out = (torch.zeros_like(mask), torch.zeros((H, W), dtype=torch.int32, device=mask.device))
        omask, cnt = out
        if tuple(omask.shape) != (H, W, words) or omask.dtype != torch.int32 or mask.dtype != torch.int32:
            raise ValueError("masks must be (H, W, words) int32")
        if cnt is not None and (tuple(cnt.shape) != (H, W) or cnt.dtype != torch.int32):
            raise ValueError("the counts must be (H, W) int32")
        if b >= 1 and words != ((2 * b + 1) ** 2 + 31) // 32:
            raise ValueError("a mask of search radius %d has %d words per pixel" % (b, ((2 * b + 1) ** 2 + 31) // 32))
        torch.cuda.synchronize(self.device)                          # (the fills ran on torch's stream)
        self._chk(lib().bcd_hip_transpose_masks_cross(self.h, _dp(mask), W, H, b, _dp(omask), _dp(cnt) if cnt is not None else None))
        return omask, cnt

    def compose_motion(self, a, b, out=None):
        """bcd_hip_compose_motion: the motion field frame t -> v from a (t -> u) and b (u -> v, in frame-u pixel order), (H, W, 2) float32 device tensors ->
        the composed field, integer-valued, (NaN, NaN) where a step is broken ("Sequences with motion").  out: the tensor to fill"""
        torch = self.torch
        if a.dim() != 3 or a.shape[2] != 2 or tuple(b.shape) != tuple(a.shape) or a.dtype != torch.float32 or b.dtype != torch.float32:
            raise ValueError("the motion fields must be (H, W, 2) float32 tensors of one size")
        H, W, _ = a.shape
        if out is None:
            out = torch.empty((H, W, 2), dtype=torch.float32, device=a.device)
        if out.numel() != H * W * 2 or out.dtype != torch.float32:
            raise ValueError("out must hold (H, W, 2) floats")
        torch.cuda.synchronize(self.device)                          # (the fills ran on torch's stream)
        self._chk(lib().bcd_hip_compose_motion(self.h, _dp(a), _dp(b), W, H, _dp(out)))
        return out

    def sequence(self, W, H, D, nscales, radius, prm, layers=None, moments=False, var_floor=1e-8, features=0, feature_variances=False, feature_floors=(),
                 feature_threshold=1.0):
        """a Sequence of this context: frames of W x H with D bins, denoised with their neighbours within `radius` frames through a sliding window.
        With none of the keywords: bcd_hip_sequence_create (one colour layer, histograms, no gate).  layers=L (1 .. 16), moments=True (selection from means
        and covariances with `var_floor`; D is not looked at), features=F (1 .. 8 channels of a feature gate with `feature_variances`, `feature_floors`,
        `feature_threshold`): bcd_hip_sequence_create_mode -- push / pop then take and return the layers"""
        if layers is None and not moments and not features:
            return Sequence(self, W, H, D, nscales, radius, prm)
        mode = dict(layers=1 if layers is None else int(layers), moments=bool(moments), var_floor=float(var_floor), features=int(features),
                    feature_variances=bool(feature_variances), feature_floors=tuple(float(x) for x in feature_floors), feature_threshold=float(feature_threshold))
        return Sequence(self, W, H, D, nscales, radius, prm, mode)

    def window_distances_cross(self, hist, ns, hist_nb, ns_nb, w, b, line, column):
        """bcd_hip_window_distances_cross: the (2b+1)^2 patch distances of one main pixel of the frame to its window in the neighbour frame, +inf outside"""
        import numpy as np
        H, W, D = hist.shape
        if tuple(hist_nb.shape) != (H, W, D) or ns_nb.numel() != H * W or ns.numel() != H * W:
            raise ValueError("the neighbour frame must have the frame's width, height and histogram depth")
        out = np.empty(((2 * b + 1) ** 2,), np.float32)
        self.torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_window_distances_cross(self.h, _dp(hist), _dp(ns), _dp(hist_nb), _dp(ns_nb), W, H, D, w, b, line, column, _fptr(out)))
        return out

    def similarity_masks_moments(self, col, pixcov, w, b, tau, var_floor=1e-8):
        """bcd_hip_similarity_masks_moments: masks and |S| from colours (H, W, 3) and per-pixel covariances (H, W, 6; pixel_cov), in the layouts of
        similarity_masks"""
        torch = self.torch
        H, W, _ = col.shape
        mask, cnt = _mask_and_count(H, W, b, col.device)
        torch.cuda.synchronize(self.device)                          # (the fills ran on torch's stream)
        self._chk(lib().bcd_hip_similarity_masks_moments(self.h, _dp(col), _dp(pixcov), W, H, w, b, tau, var_floor, _dp(mask), _dp(cnt)))
        return mask, cnt

    def window_distances_moments(self, col, pixcov, w, b, line, column, var_floor=1e-8):
        """bcd_hip_window_distances_moments: the (2b+1)^2 patch distances of one main pixel to its window, +inf outside"""
        import numpy as np
        H, W, _ = col.shape
        out = np.empty(((2 * b + 1) ** 2,), np.float32)
        self._chk(lib().bcd_hip_window_distances_moments(self.h, _dp(col), _dp(pixcov), W, H, w, b, var_floor, line, column, _fptr(out)))
        return out

    def similarity_masks_guide(self, features, variances, floors, threshold, w, b):
        """bcd_hip_similarity_masks_guide: the feature masks and their counts from features (H, W, F), optional variances (H, W, F), F floors and the
        threshold tau_g, in the layouts of similarity_masks"""
        torch = self.torch
        H, W, _ = features.shape
        mask, cnt = _mask_and_count(H, W, b, features.device)
        g, alive = self._guide(features, variances, floors, threshold)
        torch.cuda.synchronize(self.device)                          # (the fills ran on torch's stream)
        self._chk(lib().bcd_hip_similarity_masks_guide(self.h, C.byref(g), W, H, w, b, _dp(mask), _dp(cnt)))
        del alive
        return mask, cnt

    def window_distances_guide(self, features, variances, floors, w, b, line, column):
        """bcd_hip_window_distances_guide: the (2b+1)^2 feature patch distances of one main pixel to its window, +inf outside"""
        import numpy as np
        H, W, _ = features.shape
        out = np.empty(((2 * b + 1) ** 2,), np.float32)
        g, alive = self._guide(features, variances, floors, 1.0)
        self.torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_window_distances_guide(self.h, C.byref(g), W, H, w, b, line, column, _fptr(out)))
        del alive
        return out

    def gate_masks(self, mask, cnt, gate, b):
        """bcd_hip_gate_masks, in place: mask &= gate word by word, cnt = the bits that remain; returns (mask, cnt)"""
        H, W, words = mask.shape
        if words != ((2 * b + 1) ** 2 + 31) // 32 or tuple(gate.shape) != (H, W, words) or tuple(cnt.shape) != (H, W):
            raise ValueError("masks of %d words per pixel and one count per pixel expected" % (((2 * b + 1) ** 2 + 31) // 32))
        self.torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_gate_masks(self.h, _dp(mask), _dp(cnt), _dp(gate), W, H, b))
        return mask, cnt

    def active_set(self, mask, cnt, w, b, m, random_order, seed, row_begin=0, row_end=None):
        torch = self.torch
        H, W, _ = mask.shape
        state = torch.zeros((H, W), dtype=torch.uint8, device=mask.device)
        rounds = C.c_int32(0)
        self._chk(lib().bcd_hip_active_set(self.h, _dp(mask), _dp(cnt), W, H, w, b, row_begin, H if row_end is None else row_end,
                                           m, int(random_order), seed, _dp(state), C.byref(rounds)))
        return state, rounds.value

    def active_init(self, cnt, w, row_begin, row_end, m, seed, row_offset, state=None):
        H, W = cnt.shape
        if state is None:
            state = self.torch.zeros((H, W), dtype=self.torch.uint8, device=cnt.device)
        self._chk(lib().bcd_hip_active_init(self.h, _dp(cnt), W, H, w, row_begin, row_end, m, seed, row_offset, _dp(state)))
        return state

    def active_step(self, mask, cnt, state, w, b, row_begin, row_end, random_order, seed, row_offset, first_pass):
        H, W = cnt.shape
        u = C.c_int32(0)
        self._chk(lib().bcd_hip_active_step(self.h, _dp(mask), _dp(cnt), W, H, w, b, row_begin, row_end, int(random_order), seed,
                                            row_offset, 1 if first_pass else 0, _dp(state), C.byref(u)))
        return u.value

    def active_step_enqueue(self, mask, cnt, state, w, b, row_begin, row_end, random_order, seed, row_offset, total=None, with_verdict=False):
        """bcd_hip_active_step_enqueue: one batch of marking launches on the context's stream, without waiting.  total: an int64 device tensor of one
        element that receives the count of undecided pixels after the batch (+ 2^40 with with_verdict when the masks of the last deferred similarity
        pass are not valid).  After a synchronisation active_step_collect() returns the count"""
        H, W = cnt.shape
        self._chk(lib().bcd_hip_active_step_enqueue(self.h, _dp(mask), _dp(cnt), W, H, int(w), int(b), int(row_begin), int(row_end), int(random_order),
                                                    seed, int(row_offset), _dp(state), _dp(total) if total is not None else None,
                                                    1 if with_verdict else 0))

    def active_step_collect(self):
        """bcd_hip_active_step_collect -> (pixels of the owned lines still undecided, launches the batch needed); the context's stream must have been
        synchronised since active_step_enqueue"""
        u, n = C.c_int32(0), C.c_int32(0)
        self._chk(lib().bcd_hip_active_step_collect(self.h, C.byref(u), C.byref(n)))
        return u.value, n.value

    def selftest_active_lists(self, state, cnt, w, row_begin, row_end, skip_word=None, fill=-1):
        """bcd_hip_selftest_active_lists: the list compaction of the estimate call on its own, on the processed pixels (state 1) of lines
        [row_begin, row_end) -> (strong list, weak list: int32 tensors pre-filled with `fill` -- W * H entries each, as the engine sizes its own; the
        library needs room for the owned range only, which is what include/bcd_hip.h promises --, of which the first
        n_strong / n_weak are written; n_strong; n_weak; the 64-bit sum of cnt over both lists).  skip_word: an int64 device tensor of one element;
        when it is not zero the launch writes nothing"""
        torch = self.torch
        H, W = cnt.shape
        n = max(1, H * W)
        strong = torch.full((n,), fill, dtype=torch.int32, device=cnt.device)
        weak = torch.full((n,), fill, dtype=torch.int32, device=cnt.device)
        out = (C.c_int32 * 4)()
        torch.cuda.synchronize(self.device)                          # (the fills ran on torch's stream)
        self._chk(lib().bcd_hip_selftest_active_lists(self.h, _dp(state), _dp(cnt), W, H, int(w), int(row_begin), int(row_end),
                                                      _dp(skip_word) if skip_word is not None else None, _dp(strong), _dp(weak), out))
        total = (out[2] & 0xFFFFFFFF) | ((out[3] & 0xFFFFFFFF) << 32)
        return strong, weak, out[0], out[1], total

    def bayes_accumulate(self, col, pixcov, mask, nsim, state, w, b, min_eig, out=None):
        """out: the (sum, count) accumulators to add into (scale_begin clears a pair); default: fresh zeroed ones"""
        torch = self.torch
        H, W, _ = col.shape
        if out is None:
            s = torch.zeros((H, W, 3), dtype=torch.float32, device=col.device)
            c = torch.zeros((H, W), dtype=torch.int32, device=col.device)
        else:
            s, c = out
        self._chk(lib().bcd_hip_bayes_accumulate(self.h, _dp(col), _dp(pixcov), _dp(mask), _dp(nsim), _dp(state), W, H, w, b,
                                                 min_eig, _dp(s), _dp(c)))
        return s, c

    def bayes_accumulate_rows(self, col, pixcov, mask, nsim, state, w, b, min_eig, row_begin, row_end, out=None, skip_word=None):
        """bcd_hip_bayes_accumulate_rows: bayes_accumulate for the processed pixels of lines [row_begin, row_end) only -> (sum, count, skipped).
        out: the (sum, count) accumulators to add into; default: fresh zeroed ones.  skip_word: (an int64 device tensor of one element, an int64
        NumPy array of one element that holds the host copy of that word) makes the call speculative: when the word is not zero the kernels do
        nothing and skipped is 1"""
        torch = self.torch
        H, W, _ = col.shape
        if out is None:
            s = torch.zeros((H, W, 3), dtype=torch.float32, device=col.device)
            c = torch.zeros((H, W), dtype=torch.int32, device=col.device)
        else:
            s, c = out
        d_word = h_word = None
        skipped = C.c_int(0)
        if skip_word is not None:
            d, h = skip_word
            if d.dtype != torch.int64 or d.numel() != 1 or str(h.dtype) != "int64" or h.size != 1:
                raise ValueError("skip_word must be (a one-element int64 device tensor, a one-element int64 NumPy array)")
            d_word, h_word = _dp(d), C.c_void_p(h.ctypes.data)
        self._chk(lib().bcd_hip_bayes_accumulate_rows(self.h, _dp(col), _dp(pixcov), _dp(mask), _dp(nsim), _dp(state), W, H, int(w), int(b), min_eig,
                                                      _dp(s), _dp(c), int(row_begin), int(row_end), d_word, h_word,
                                                      C.byref(skipped) if skip_word is not None else None))
        return s, c, skipped.value

    def bayes_accumulate_temporal(self, frames, nsim_total, state, w, b, min_eig, out=None):
        """bcd_hip_bayes_accumulate_temporal: `frames` is a list of (colours, per-pixel covariances, masks) device tensors, [0] the frame itself and the
        others its neighbour frames with their cross masks; nsim_total = |S_0| + sum |S_f|.  -> (sum, count), accumulated into `out` if given"""
        torch = self.torch
        H, W, _ = frames[0][0].shape
        if out is None:
            s = torch.zeros((H, W, 3), dtype=torch.float32, device=frames[0][0].device)
            c = torch.zeros((H, W), dtype=torch.int32, device=frames[0][0].device)
        else:
            s, c = out
        arr = (StageFrame * max(len(frames), 1))()
        for i, (col, pixcov, mask) in enumerate(frames):
            if tuple(col.shape) != (H, W, 3) or tuple(pixcov.shape) != (H, W, 6) or mask.numel() != H * W * (((2 * b + 1) ** 2 + 31) // 32):
                raise ValueError("frame %d: colours (H, W, 3), per-pixel covariances (H, W, 6) and masks (H, W, words) of the frame's size are expected" % i)
            arr[i].d_colors, arr[i].d_pixel_cov, arr[i].d_mask = col.data_ptr(), pixcov.data_ptr(), mask.data_ptr()
            _dp(col), _dp(pixcov), _dp(mask)
        torch.cuda.synchronize(self.device)                          # (the fills ran on torch's stream)
        self._chk(lib().bcd_hip_bayes_accumulate_temporal(self.h, arr, len(frames), _dp(nsim_total), _dp(state), W, H, w, b, min_eig, _dp(s), _dp(c)))
        return s, c

    @staticmethod
    def _frame_array(neighbours, H, W, D, ptr, numel):
        """the bcd_hip_frame array of a list of (col, ns, hist, cov) neighbour frames of the frame's size; ptr(a) is an address, numel(a) a number of elements"""
        arr = (Frame * max(len(neighbours), 1))()
        for i, f in enumerate(neighbours):
            if tuple(f[0].shape) != (H, W, 3) or numel(f[1]) != H * W or tuple(f[2].shape) != (H, W, D) or tuple(f[3].shape) != (H, W, 6):
                raise ValueError("neighbour %d: images of the frame's width, height and histogram depth are expected" % i)
            arr[i].d_colors, arr[i].d_nsamples, arr[i].d_histograms, arr[i].d_covariances = (ptr(a) for a in f)
        return arr

    def denoise_temporal(self, col, ns, hist, cov, neighbours, nscales, prm, out=None):
        """bcd_hip_denoise_temporal: the frame (col, ns, hist, cov) denoised with similar patches from up to four neighbour frames of its sequence,
        each a (col, ns, hist, cov) tuple of device tensors of the frame's size.  No neighbour: denoise()."""
        torch = self.torch
        H, W, D = hist.shape
        neighbours = list(neighbours)
        arr = self._frame_array(neighbours, H, W, D, _dptr, torch.numel)
        if out is None:
            out = torch.empty((H, W, 3), dtype=torch.float32, device=hist.device)
        torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_denoise_temporal(self.h, _dp(col), _dp(ns), _dp(hist), _dp(cov), arr, len(neighbours), W, H, D, int(nscales), C.byref(prm), _dp(out)))
        return out

    def denoise_temporal_host(self, col, ns, hist, cov, neighbours, nscales, prm):
        """bcd_hip_denoise_temporal_host on NumPy float32 arrays -> the denoised frame (H, W, 3)"""
        import numpy as np
        as32 = lambda a: np.ascontiguousarray(a, np.float32)
        col, ns, hist, cov = (as32(a) for a in (col, ns, hist, cov))
        H, W, D = hist.shape
        keep = [tuple(as32(a) for a in f) for f in neighbours]
        arr = self._frame_array(keep, H, W, D, _hptr, np.size)
        out = np.empty((H, W, 3), np.float32)
        self._chk(lib().bcd_hip_denoise_temporal_host(self.h, col.ctypes.data, ns.ctypes.data, hist.ctypes.data, cov.ctypes.data, arr, len(keep), W, H, D, int(nscales),
                                                      C.byref(prm), out.ctypes.data))
        return out

    def bayes_accumulate_temporal_layers(self, frames, nsim_total, state, w, b, min_eig, out=None):
        """bcd_hip_bayes_accumulate_temporal_layers: `frames` is a list of ([(colours, per-pixel covariances), ...], masks), [0] the frame itself and the
        others its neighbour frames with their cross masks, every frame with the same layers in the same order; nsim_total = |S_0| + sum |S_f|.
        -> (list of sum images, the shared count image, items per layer that took the redo list); out: (sums, count) to accumulate into"""
        torch = self.torch
        frames = [(list(layers), mask) for (layers, mask) in frames]
        H, W = nsim_total.shape
        nl = len(frames[0][0]) if frames else 0
        if out is None:
            sums = [torch.zeros((H, W, 3), dtype=torch.float32, device=nsim_total.device) for _ in range(nl)]
            c = torch.zeros((H, W), dtype=torch.int32, device=nsim_total.device)
        else:
            sums, c = out
            sums = list(sums)
        arr = (StageFrameLayers * max(len(frames), 1))()
        keep = []
        for i, (layers, mask) in enumerate(frames):
            if len(layers) != nl:
                raise ValueError("frame %d: %d layers expected" % (i, nl))
            for (col, pc) in layers:
                if tuple(col.shape) != (H, W, 3) or tuple(pc.shape) != (H, W, 6):
                    raise ValueError("frame %d: colours (H, W, 3) and per-pixel covariances (H, W, 6) of the frame's size are expected" % i)
            if mask.numel() != H * W * (((2 * b + 1) ** 2 + 31) // 32):
                raise ValueError("frame %d: masks (H, W, words) of the frame's size are expected" % i)
            cols, pcs = self._ptr_list([col for col, _ in layers]), self._ptr_list([pc for _, pc in layers])
            keep += [cols, pcs]
            arr[i].d_colors, arr[i].d_pixel_cov, arr[i].d_mask = cols, pcs, _dp(mask).value
        redo = (C.c_int32 * max(1, nl))()
        torch.cuda.synchronize(self.device)                          # (the fills ran on torch's stream)
        self._chk(lib().bcd_hip_bayes_accumulate_temporal_layers(self.h, arr, len(frames), nl, _dp(nsim_total), _dp(state), W, H, w, b, min_eig,
                                                                 self._ptr_list(sums), _dp(c), redo))
        return sums, c, list(redo)[:nl]

    @staticmethod
    def _frame_layers_array(neighbours, nl, H, W, D, ptr, numel):
        """the bcd_hip_frame_layers array of a list of (ns, hist, [(colours, covariances), ...]) of the frame's size; ptr(a) is an address, numel(a) a number of
        elements"""
        arr = (FrameLayers * max(len(neighbours), 1))()
        keep = []
        for i, (ns, hist, layers) in enumerate(neighbours):
            layers = list(layers)
            if len(layers) != nl:
                raise ValueError("neighbour %d: one layer per layer of the frame expected (%d, not %d)" % (i, nl, len(layers)))
            if numel(ns) != H * W or tuple(hist.shape) != (H, W, D) or any(tuple(c.shape) != (H, W, 3) or tuple(v.shape) != (H, W, 6) for c, v in layers):
                raise ValueError("neighbour %d: images of the frame's width, height and histogram depth are expected" % i)
            la = (FrameLayer * max(nl, 1))()
            for k, (col, cov) in enumerate(layers):
                la[k].d_colors, la[k].d_covariances = ptr(col), ptr(cov)
            keep.append(la)
            arr[i].d_nsamples, arr[i].d_histograms, arr[i].layers = ptr(ns), ptr(hist), la
        return arr, keep

    def denoise_temporal_layers(self, ns, hist, layers, neighbours, nscales, prm, outs=None):
        """bcd_hip_denoise_temporal_layers: the colour layers `layers` -- a list of (colours, covariances) device tensors that share `ns` and `hist` -- denoised
        with similar patches from up to four neighbour frames, each (ns, hist, [(colours, covariances), ...]) with the same layers in the same order.  One
        selection per scale serves every layer.  -> the list of outputs"""
        torch = self.torch
        H, W, D = hist.shape
        arr, layers, outs = self._layer_array(layers, outs, H, W, hist.device)
        neighbours = list(neighbours)
        nb, keep = self._frame_layers_array(neighbours, len(layers), H, W, D, _dptr, torch.numel)
        torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_denoise_temporal_layers(self.h, _dp(ns), _dp(hist), nb, len(neighbours), W, H, D, int(nscales), C.byref(prm), arr, len(layers)))
        return outs

    def denoise_temporal_layers_host(self, ns, hist, layers, neighbours, nscales, prm):
        """bcd_hip_denoise_temporal_layers_host on NumPy float32 arrays -> the list of denoised layers (H, W, 3)"""
        import numpy as np
        as32 = lambda a: np.ascontiguousarray(a, np.float32)
        ns, hist = as32(ns), as32(hist)
        H, W, D = hist.shape
        neighbours = [(as32(n), as32(h), [(as32(c), as32(v)) for c, v in lay]) for n, h, lay in neighbours]
        arr, layers, outs = _host_layer_array(layers, H, W, Layer)
        nb, keep = self._frame_layers_array(neighbours, len(layers), H, W, D, _hptr, np.size)
        self._chk(lib().bcd_hip_denoise_temporal_layers_host(self.h, ns.ctypes.data, hist.ctypes.data, nb, len(neighbours), W, H, D, int(nscales), C.byref(prm), arr,
                                                             len(layers)))
        return outs

    # ---- motion: neighbour frames reprojected by a motion field ("Motion") ----
    @staticmethod
    def _motion_array(motions, n, H, W, ptr, size):
        """the array of nb_neighbours field pointers (None: zero motion for that neighbour); motions None: a NULL list"""
        if motions is None:
            return None
        motions = list(motions)
        if len(motions) != n:
            raise ValueError("one motion field (or None) per neighbour expected (%d, not %d)" % (n, len(motions)))
        arr = (C.c_void_p * max(1, n))()
        for i, m in enumerate(motions):
            if m is None:
                continue
            if size(m) != H * W * 2:
                raise ValueError("motion field %d: (H, W, 2) floats of the frame's size are expected" % i)
            arr[i] = ptr(m)
        return arr

    def denoise_temporal_motion(self, col, ns, hist, cov, neighbours, motions, nscales, prm, out=None):
        """bcd_hip_denoise_temporal_motion: denoise_temporal with neighbour i warped into the frame's pixel grid by motions[i] -- an (H, W, 2) float32 device
        tensor of (dx, dy) per pixel, or None for zero motion -- and the cross masks gated by the validity of the warped patches.  motions=None passes a NULL list."""
        torch = self.torch
        H, W, D = hist.shape
        neighbours = list(neighbours)
        arr = self._frame_array(neighbours, H, W, D, _dptr, torch.numel)
        mv = self._motion_array(motions, len(neighbours), H, W, _dptr, torch.numel)
        if out is None:
            out = torch.empty((H, W, 3), dtype=torch.float32, device=hist.device)
        torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_denoise_temporal_motion(self.h, _dp(col), _dp(ns), _dp(hist), _dp(cov), arr, len(neighbours), mv, W, H, D, int(nscales), C.byref(prm), _dp(out)))
        return out

    def denoise_temporal_motion_host(self, col, ns, hist, cov, neighbours, motions, nscales, prm):
        """bcd_hip_denoise_temporal_motion_host on NumPy float32 arrays -> the denoised frame (H, W, 3)"""
        import numpy as np
        as32 = lambda a: np.ascontiguousarray(a, np.float32)
        col, ns, hist, cov = (as32(a) for a in (col, ns, hist, cov))
        H, W, D = hist.shape
        keep = [tuple(as32(a) for a in f) for f in neighbours]
        arr = self._frame_array(keep, H, W, D, _hptr, np.size)
        fields = None if motions is None else [None if m is None else as32(m) for m in motions]
        mv = self._motion_array(fields, len(keep), H, W, _hptr, np.size)
        out = np.empty((H, W, 3), np.float32)
        self._chk(lib().bcd_hip_denoise_temporal_motion_host(self.h, col.ctypes.data, ns.ctypes.data, hist.ctypes.data, cov.ctypes.data, arr, len(keep), mv, W, H, D,
                                                             int(nscales), C.byref(prm), out.ctypes.data))
        return out

    def denoise_temporal_layers_motion(self, ns, hist, layers, neighbours, motions, nscales, prm, outs=None):
        """bcd_hip_denoise_temporal_layers_motion: denoise_temporal_layers with neighbour i warped by motions[i] (an (H, W, 2) device tensor or None) -> the outputs"""
        torch = self.torch
        H, W, D = hist.shape
        arr, layers, outs = self._layer_array(layers, outs, H, W, hist.device)
        neighbours = list(neighbours)
        nb, keep = self._frame_layers_array(neighbours, len(layers), H, W, D, _dptr, torch.numel)
        mv = self._motion_array(motions, len(neighbours), H, W, _dptr, torch.numel)
        torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_denoise_temporal_layers_motion(self.h, _dp(ns), _dp(hist), nb, len(neighbours), mv, W, H, D, int(nscales), C.byref(prm), arr, len(layers)))
        return outs

    def warp_frame(self, col, ns, hist, cov, motion, out=None):
        """bcd_hip_warp_frame: the four images of a neighbour gathered through `motion` ((H, W, 2) device tensor, or None: zero motion)
        -> (colours, sample counts, histograms, covariances, validity (H, W) uint8); out: the five destinations"""
        torch = self.torch
        H, W, D = hist.shape
        if out is None:
            out = [torch.empty_like(t) for t in (col, ns, hist, cov)] + [torch.empty((H, W), dtype=torch.uint8, device=hist.device)]
        src, dst = Frame(), WarpedFrame()
        src.d_colors, src.d_nsamples, src.d_histograms, src.d_covariances = (_dp(t).value for t in (col, ns, hist, cov))
        dst.d_colors, dst.d_nsamples, dst.d_histograms, dst.d_covariances = (_dp(t).value for t in out[:4])
        if motion is not None and motion.numel() != H * W * 2:
            raise ValueError("the motion field must hold (H, W, 2) floats")
        torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_warp_frame(self.h, C.byref(src), _dp(motion) if motion is not None else None, W, H, D, C.byref(dst), _dp(out[4])))
        return tuple(out)

    def warp_layers(self, layers, motion, out=None):
        """bcd_hip_warp_layers: `layers` is a list of (colours, covariances) device tensors of one neighbour -> ([(colours, covariances), ...], validity (H, W) uint8);
        out: (list of destination pairs, validity)"""
        torch = self.torch
        layers = list(layers)
        H, W, _ = layers[0][0].shape
        if out is None:
            out = ([(torch.empty_like(c), torch.empty_like(v)) for c, v in layers], torch.empty((H, W), dtype=torch.uint8, device=layers[0][0].device))
        dsts, valid = out
        src, dst = (FrameLayer * max(1, len(layers)))(), (FrameLayer * max(1, len(layers)))()
        for k, ((c, v), (oc, ov)) in enumerate(zip(layers, dsts)):
            if tuple(c.shape) != (H, W, 3) or tuple(v.shape) != (H, W, 6) or oc.numel() != H * W * 3 or ov.numel() != H * W * 6:
                raise ValueError("layer %d: colours (H, W, 3) and covariances (H, W, 6) are expected" % k)
            src[k].d_colors, src[k].d_covariances, dst[k].d_colors, dst[k].d_covariances = _dp(c).value, _dp(v).value, _dp(oc).value, _dp(ov).value
        torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_warp_layers(self.h, src, len(layers), _dp(motion) if motion is not None else None, W, H, dst, _dp(valid)))
        return dsts, valid

    def valid_downscale(self, valid):
        """bcd_hip_valid_downscale: the validity bytes (H, W) of a level -> those of the next level (H // 2, W // 2)"""
        H, W = valid.shape
        out = self.torch.empty((H // 2, W // 2), dtype=self.torch.uint8, device=valid.device)
        self.torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_valid_downscale(self.h, _dp(valid), W, H, _dp(out)))
        return out

    def gate_masks_valid(self, mask, count, valid, w, b):
        """bcd_hip_gate_masks_valid: the cross masks (H, W, words) and counts (H, W) of one neighbour gated IN PLACE by the validity bytes (H, W) of its level"""
        H, W = valid.shape
        if mask.numel() != H * W * (((2 * b + 1) ** 2 + 31) // 32) or count.numel() != H * W:
            raise ValueError("masks (H, W, words) and counts (H, W) of the validity image's size are expected")
        self.torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_gate_masks_valid(self.h, _dp(mask), _dp(count), _dp(valid), W, H, int(w), int(b)))
        return mask, count

    # ---- features: the cross-frame selection gated by auxiliary feature buffers ("Features") ----
    @staticmethod
    def _guide_images(features, variances, shape, ptr):
        """the bcd_hip_guide_images of one neighbour: features and optional variances of the frame's feature shape; ptr(a) is an address"""
        if tuple(features.shape) != tuple(shape) or (variances is not None and tuple(variances.shape) != tuple(shape)):
            raise ValueError("a neighbour's features (and variances) must have the shape of the frame's features, %r" % (tuple(shape),))
        return GuideImages(ptr(features), None if variances is None else ptr(variances))

    def _guide_images_array(self, neighbour_features, neighbour_variances, n, shape, ptr):
        feats = list(neighbour_features)
        vrs = [None] * len(feats) if neighbour_variances is None else list(neighbour_variances)
        if len(feats) != n or len(vrs) != n:
            raise ValueError("one feature image (and one variance image, or none at all) per neighbour expected")
        arr = (GuideImages * max(1, n))()
        for i, (f, v) in enumerate(zip(feats, vrs)):
            arr[i] = self._guide_images(f, v, shape, ptr)
        return arr

    def denoise_temporal_guided(self, ns, hist, layers, neighbours, nscales, prm, features, neighbour_features, variances=None, neighbour_variances=None, floors=(),
                                threshold=1.0, motions=None, outs=None):
        """bcd_hip_denoise_temporal_guided: denoise_temporal_layers_motion with the in-frame and the cross-frame selection gated by feature buffers.  features /
        variances: (H, W, F) device tensors of the frame; neighbour_features / neighbour_variances: one per neighbour (variances for every frame or for none);
        floors F numbers, threshold tau_g; motions: None (nothing is warped) or one (H, W, 2) tensor or None per neighbour -> the outputs"""
        torch = self.torch
        H, W, D = hist.shape
        arr, layers, outs = self._layer_array(layers, outs, H, W, hist.device)
        neighbours = list(neighbours)
        nb, keep = self._frame_layers_array(neighbours, len(layers), H, W, D, _dptr, torch.numel)
        mv = self._motion_array(motions, len(neighbours), H, W, _dptr, torch.numel)
        if tuple(features.shape[:2]) != (H, W):
            raise ValueError("features must be %dx%dxF" % (H, W))
        g, alive = self._guide(features, variances, floors, threshold)
        ng = self._guide_images_array(neighbour_features, neighbour_variances, len(neighbours), features.shape, _dptr)
        torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_denoise_temporal_guided(self.h, _dp(ns), _dp(hist), nb, len(neighbours), mv, W, H, D, int(nscales), C.byref(prm), arr, len(layers),
                                                        C.byref(g), ng))
        del alive, keep
        return outs

    def denoise_temporal_guided_host(self, ns, hist, layers, neighbours, nscales, prm, features, neighbour_features, variances=None, neighbour_variances=None,
                                     floors=(), threshold=1.0, motions=None):
        """bcd_hip_denoise_temporal_guided_host on NumPy float32 arrays -> the list of denoised layers (H, W, 3)"""
        import numpy as np
        as32 = lambda a: np.ascontiguousarray(a, np.float32)
        ns, hist = as32(ns), as32(hist)
        H, W, D = hist.shape
        neighbours = [(as32(n), as32(h), [(as32(c), as32(v)) for c, v in lay]) for n, h, lay in neighbours]
        arr, layers, outs = _host_layer_array(layers, H, W, Layer)
        nb, keep = self._frame_layers_array(neighbours, len(layers), H, W, D, _hptr, np.size)
        fields = None if motions is None else [None if m is None else as32(m) for m in motions]
        mv = self._motion_array(fields, len(neighbours), H, W, _hptr, np.size)
        g, alive = self._guide(features, variances, floors, threshold, host=True)
        if tuple(alive[0].shape[:2]) != (H, W):
            raise ValueError("features must be %dx%dxF" % (H, W))
        nfeat = [as32(f) for f in neighbour_features]
        nvar = None if neighbour_variances is None else [as32(v) for v in neighbour_variances]
        ng = self._guide_images_array(nfeat, nvar, len(neighbours), alive[0].shape, _hptr)
        self._chk(lib().bcd_hip_denoise_temporal_guided_host(self.h, ns.ctypes.data, hist.ctypes.data, nb, len(neighbours), mv, W, H, D, int(nscales), C.byref(prm),
                                                             arr, len(layers), C.byref(g), ng))
        del alive, keep, fields
        return outs

    def similarity_masks_guide_cross(self, features, variances, features_nb, variances_nb, floors, threshold, w, b, out=None):
        """bcd_hip_similarity_masks_guide_cross: the cross feature mask G_j and its counts between the frame's features (H, W, F) (optional variances) and a
        neighbour's, in the layouts of similarity_masks_cross.  out: (mask (H, W, words) int32, count (H, W) int32) contiguous device tensors to fill"""
        torch = self.torch
        H, W, _ = features.shape
        if out is None:
            out = _mask_and_count(H, W, b, features.device)
        mask, cnt = out
        if mask.numel() != H * W * (((2 * b + 1) ** 2 + 31) // 32) or cnt.numel() != H * W or mask.dtype != torch.int32 or cnt.dtype != torch.int32:
            raise ValueError("out must be ((H, W, words) int32, (H, W) int32)")
        g, alive = self._guide(features, variances, floors, threshold)
        ng = self._guide_images(features_nb, variances_nb, features.shape, _dptr)
        torch.cuda.synchronize(self.device)                          # (the fills ran on torch's stream)
        self._chk(lib().bcd_hip_similarity_masks_guide_cross(self.h, C.byref(g), C.byref(ng), W, H, int(w), int(b), _dp(mask), _dp(cnt)))
        del alive
        return mask, cnt

    def window_distances_guide_cross(self, features, variances, features_nb, variances_nb, floors, w, b, line, column):
        """bcd_hip_window_distances_guide_cross: the (2b+1)^2 cross feature distances of one main pixel of the frame to its window in the neighbour, +inf outside"""
        import numpy as np
        H, W, _ = features.shape
        out = np.empty(((2 * b + 1) ** 2,), np.float32)
        g, alive = self._guide(features, variances, floors, 1.0)
        ng = self._guide_images(features_nb, variances_nb, features.shape, _dptr)
        self.torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_window_distances_guide_cross(self.h, C.byref(g), C.byref(ng), W, H, int(w), int(b), int(line), int(column), _fptr(out)))
        del alive
        return out

    def warp_features(self, features, variances, motion, out=None):
        """bcd_hip_warp_features: the feature image (H, W, F) of a neighbour, and its variance image or None, gathered through `motion` ((H, W, 2) device
        tensor, or None: zero motion) -> (features, variances or None, validity (H, W) uint8); out: the three destinations (the second None without variances)"""
        torch = self.torch
        H, W, F = features.shape
        if out is None:
            out = (torch.empty_like(features), None if variances is None else torch.empty_like(variances), torch.empty((H, W), dtype=torch.uint8, device=features.device))
        of, ov, valid = out
        if of.numel() != H * W * F or (ov is not None and ov.numel() != H * W * F) or valid.numel() != H * W:
            raise ValueError("destinations of the sources' sizes and (H, W) validity bytes are expected")
        if motion is not None and motion.numel() != H * W * 2:
            raise ValueError("the motion field must hold (H, W, 2) floats")
        src = self._guide_images(features, variances, features.shape, _dptr)
        torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_warp_features(self.h, C.byref(src), F, _dp(motion) if motion is not None else None, W, H, _dp(of), _dp(ov) if ov is not None else None,
                                              _dp(valid)))
        return of, ov, valid

    # ---- moments: the cross-frame selection from means and covariances, without histograms ("Moments") ----
    def similarity_masks_moments_cross(self, col, pixcov, col_nb, pixcov_nb, w, b, tau, var_floor=1e-8, form=0, out=None):
        """bcd_hip_similarity_masks_moments_cross: the cross masks and counts between the guide layer of a frame -- colours (H, W, 3), per-pixel covariances
        (H, W, 6) -- and that of a neighbour, in the layouts of similarity_masks_cross.  form: 0 the production choice, 1 planes, 2 fused (w = 1, b <= 6).
        out: (mask (H, W, words) int32, count (H, W) int32) contiguous device tensors to fill"""
        torch = self.torch
        H, W, _ = col.shape
        if out is None:
            out = _mask_and_count(H, W, b, col.device)
        mask, cnt = out
        if mask.numel() != H * W * (((2 * b + 1) ** 2 + 31) // 32) or cnt.numel() != H * W or mask.dtype != torch.int32 or cnt.dtype != torch.int32:
            raise ValueError("out must be ((H, W, words) int32, (H, W) int32)")
        if col_nb.numel() != H * W * 3 or pixcov.numel() != H * W * 6 or pixcov_nb.numel() != H * W * 6:
            raise ValueError("colours (H, W, 3) and per-pixel covariances (H, W, 6) of one size are expected for both frames")
        torch.cuda.synchronize(self.device)                          # (the fills ran on torch's stream)
        self._chk(lib().bcd_hip_similarity_masks_moments_cross(self.h, _dp(col), _dp(pixcov), _dp(col_nb), _dp(pixcov_nb), W, H, int(w), int(b), float(tau),
                                                               float(var_floor), int(form), _dp(mask), _dp(cnt)))
        return mask, cnt

    def window_distances_moments_cross(self, col, pixcov, col_nb, pixcov_nb, w, b, line, column, var_floor=1e-8):
        """bcd_hip_window_distances_moments_cross: the (2b+1)^2 cross moment distances of one main pixel of the frame to its window in the neighbour, +inf outside"""
        import numpy as np
        H, W, _ = col.shape
        if col_nb.numel() != H * W * 3 or pixcov.numel() != H * W * 6 or pixcov_nb.numel() != H * W * 6:
            raise ValueError("colours (H, W, 3) and per-pixel covariances (H, W, 6) of one size are expected for both frames")
        out = np.empty(((2 * b + 1) ** 2,), np.float32)
        self.torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_window_distances_moments_cross(self.h, _dp(col), _dp(pixcov), _dp(col_nb), _dp(pixcov_nb), W, H, int(w), int(b), float(var_floor),
                                                               int(line), int(column), _fptr(out)))
        return out

    @staticmethod
    def _moment_frames_array(neighbours, nl, H, W, ptr, numel):
        """the bcd_hip_frame_layers array of a list of (ns, [(colours, covariances), ...]) of the frame's size, with NULL histograms"""
        arr = (FrameLayers * max(len(neighbours), 1))()
        keep = []
        for i, (ns, layers) in enumerate(neighbours):
            layers = list(layers)
            if len(layers) != nl:
                raise ValueError("neighbour %d: one layer per layer of the frame expected (%d, not %d)" % (i, nl, len(layers)))
            if numel(ns) != H * W or any(tuple(c.shape) != (H, W, 3) or tuple(v.shape) != (H, W, 6) for c, v in layers):
                raise ValueError("neighbour %d: images of the frame's width and height are expected" % i)
            la = (FrameLayer * max(nl, 1))()
            for k, (col, cov) in enumerate(layers):
                la[k].d_colors, la[k].d_covariances = ptr(col), ptr(cov)
            keep.append(la)
            arr[i].d_nsamples, arr[i].d_histograms, arr[i].layers = ptr(ns), None, la
        return arr, keep

    def denoise_temporal_moments(self, ns, layers, neighbours, nscales, prm, var_floor=1e-8, motions=None, features=None, neighbour_features=None, variances=None,
                                 neighbour_variances=None, floors=(), threshold=1.0, outs=None):
        """bcd_hip_denoise_temporal_moments: the colour layers `layers` -- (colours, covariances) device tensors that share `ns`, layers[0] the guide layer of the
        selection -- denoised with similar patches from up to four neighbour frames, each (ns, [(colours, covariances), ...]), every selection made from means and
        covariances: no histogram anywhere.  motions: None or one (H, W, 2) tensor or None per neighbour; features (with neighbour_features, and variances for every
        frame or none): the feature gate of denoise_temporal_guided -> the list of outputs"""
        torch = self.torch
        H, W = ns.shape[:2]
        arr, layers, outs = self._layer_array(layers, outs, H, W, ns.device)
        neighbours = list(neighbours)
        nb, keep = self._moment_frames_array(neighbours, len(layers), H, W, _dptr, torch.numel)
        mv = self._motion_array(motions, len(neighbours), H, W, _dptr, torch.numel)
        g = ng = alive = None
        if features is not None:
            if tuple(features.shape[:2]) != (H, W):
                raise ValueError("features must be %dx%dxF" % (H, W))
            g, alive = self._guide(features, variances, floors, threshold)
            ng = self._guide_images_array(neighbour_features if neighbour_features is not None else [], neighbour_variances, len(neighbours), features.shape, _dptr)
        torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_denoise_temporal_moments(self.h, _dp(ns), nb, len(neighbours), mv, W, H, int(nscales), C.byref(prm), float(var_floor), arr, len(layers),
                                                         None if g is None else C.byref(g), ng))
        del alive, keep
        return outs

    def denoise_temporal_moments_host(self, ns, layers, neighbours, nscales, prm, var_floor=1e-8, motions=None, features=None, neighbour_features=None, variances=None,
                                      neighbour_variances=None, floors=(), threshold=1.0):
        """bcd_hip_denoise_temporal_moments_host on NumPy float32 arrays -> the list of denoised layers (H, W, 3)"""
        import numpy as np
        as32 = lambda a: np.ascontiguousarray(a, np.float32)
        ns = as32(ns)
        H, W = ns.shape[:2]
        neighbours = [(as32(n), [(as32(c), as32(v)) for c, v in lay]) for n, lay in neighbours]
        arr, layers, outs = _host_layer_array(layers, H, W, Layer)
        nb, keep = self._moment_frames_array(neighbours, len(layers), H, W, _hptr, np.size)
        fields = None if motions is None else [None if m is None else as32(m) for m in motions]
        mv = self._motion_array(fields, len(neighbours), H, W, _hptr, np.size)
        g = ng = alive = nfeat = nvar = None
        if features is not None:
            g, alive = self._guide(features, variances, floors, threshold, host=True)
            if tuple(alive[0].shape[:2]) != (H, W):
                raise ValueError("features must be %dx%dxF" % (H, W))
            nfeat = [as32(f) for f in (neighbour_features if neighbour_features is not None else [])]
            nvar = None if neighbour_variances is None else [as32(v) for v in neighbour_variances]
            ng = self._guide_images_array(nfeat, nvar, len(neighbours), alive[0].shape, _hptr)
        self._chk(lib().bcd_hip_denoise_temporal_moments_host(self.h, ns.ctypes.data, nb, len(neighbours), mv, W, H, int(nscales), C.byref(prm), float(var_floor), arr,
                                                              len(layers), None if g is None else C.byref(g), ng))
        del alive, keep, fields, nfeat, nvar
        return outs

    def denoise_temporal_layers_motion_host(self, ns, hist, layers, neighbours, motions, nscales, prm):
        """bcd_hip_denoise_temporal_layers_motion_host on NumPy float32 arrays: denoise_temporal_layers_host with per neighbour an (H, W, 2) motion field or
        None -> the list of denoised layers (H, W, 3)"""
        import numpy as np
        as32 = lambda a: np.ascontiguousarray(a, np.float32)
        ns, hist = as32(ns), as32(hist)
        H, W, D = hist.shape
        neighbours = [(as32(n), as32(h), [(as32(c), as32(v)) for c, v in lay]) for n, h, lay in neighbours]
        arr, layers, outs = _host_layer_array(layers, H, W, Layer)
        nb, keep = self._frame_layers_array(neighbours, len(layers), H, W, D, _hptr, np.size)
        fields = None if motions is None else [None if m is None else as32(m) for m in motions]
        mv = self._motion_array(fields, len(neighbours), H, W, _hptr, np.size)
        self._chk(lib().bcd_hip_denoise_temporal_layers_motion_host(self.h, ns.ctypes.data, hist.ctypes.data, nb, len(neighbours), mv, W, H, D, int(nscales), C.byref(prm),
                                                                    arr, len(layers)))
        del keep, fields
        return outs

    # ---- the spike prefilter in every frame of a host frame call ("Prefilter") ----
    def denoise_temporal_host_ex(self, ns, hist, layers, neighbours, nscales, prm, spike_factor=None, var_floor=1e-8, motions=None, features=None,
                                 neighbour_features=None, variances=None, neighbour_variances=None, floors=(), threshold=1.0, reserved=None):
        """bcd_hip_denoise_temporal_host_ex on NumPy float32 arrays: the host frame call that takes these arguments (hist None: the moment selection, its
        neighbours (ns, [(colours, covariances), ...]); else (ns, hist, [...]); features: the feature gate; motions: the motion fields), every frame passed
        through the spike prefilter on its own when spike_factor > 0 (None: a NULL options pointer) -> the list of denoised layers (H, W, 3)"""
        import numpy as np
        as32 = lambda a: np.ascontiguousarray(a, np.float32)
        ns = as32(ns)
        H, W = ns.shape[:2]
        moments = hist is None
        D = 0
        arr, layers, outs = _host_layer_array(layers, H, W, Layer)
        if moments:
            neighbours = [(as32(f[0]), [(as32(c), as32(v)) for c, v in f[-1]]) for f in neighbours]
            nb, keep = self._moment_frames_array(neighbours, len(layers), H, W, _hptr, np.size)
        else:
            hist = as32(hist)
            D = hist.shape[2]
            neighbours = [(as32(n), as32(h), [(as32(c), as32(v)) for c, v in lay]) for n, h, lay in neighbours]
            nb, keep = self._frame_layers_array(neighbours, len(layers), H, W, D, _hptr, np.size)
        fields = None if motions is None else [None if m is None else as32(m) for m in motions]
        mv = self._motion_array(fields, len(neighbours), H, W, _hptr, np.size)
        g = ng = alive = nfeat = nvar = None
        if features is not None:
            g, alive = self._guide(features, variances, floors, threshold, host=True)
            if tuple(alive[0].shape[:2]) != (H, W):
                raise ValueError("features must be %dx%dxF" % (H, W))
            nfeat = [as32(f) for f in (neighbour_features if neighbour_features is not None else [])]
            nvar = None if neighbour_variances is None else [as32(v) for v in neighbour_variances]
            ng = self._guide_images_array(nfeat, nvar, len(neighbours), alive[0].shape, _hptr)
        opt = None if spike_factor is None else TemporalHostOptions(float(spike_factor), reserved)
        self._chk(lib().bcd_hip_denoise_temporal_host_ex(self.h, ns.ctypes.data, None if moments else hist.ctypes.data, nb, len(neighbours), mv, W, H, D, int(nscales),
                                                         C.byref(prm), float(var_floor), arr, len(layers), None if g is None else C.byref(g), ng,
                                                         None if opt is None else C.byref(opt)))
        del alive, keep, fields, nfeat, nvar
        return outs

    def denoise_temporal_stages(self, col, ns, hist, cov, neighbours, prm):
        """One scale of the denoising of a frame with similar patches from neighbouring frames of its sequence, composed from the
        stage calls: in-frame masks, cross masks of every neighbour, the marking on the in-frame masks and the total |S|, the estimate over the members of
        all frames, the finalisation.  neighbours: a list of (colours, sample counts, histograms, covariances) device tensors of the frame's size, at most
        four; patch radius 1 and search radius 6.  With no neighbour it computes what denoise(..., nscales=1, prm) computes.
        -> (denoised frame (H, W, 3), dict(processed, fallback, similar_total))"""
        torch = self.torch
        w, b, tau = prm.patch_radius, prm.search_radius, prm.hist_dist_threshold
        neighbours = list(neighbours)
        mask, nsim = self.similarity_masks(hist, ns, w, b, tau)
        frames = [(col, self.pixel_cov(cov, ns), mask)]
        self.synchronize()
        total = nsim.clone()
        for (col_nb, ns_nb, hist_nb, cov_nb) in neighbours:
            mask_nb, nsim_nb = self.similarity_masks_cross(hist, ns, hist_nb, ns_nb, w, b, tau)
            total += nsim_nb
            frames.append((col_nb, self.pixel_cov(cov_nb, ns_nb), mask_nb))
        self.synchronize()
        state, _ = self.active_set(mask, total, w, b, prm.marked_skip_probability, prm.use_random_pixel_order, prm.order_seed)
        s, c = self.bayes_accumulate_temporal(frames, total, state, w, b, prm.min_eigen_value)
        out = self.finalize(s, c)
        self.synchronize()
        processed = state == 1
        strong = processed & (total >= 3 * (2 * w + 1) ** 2 + 1)
        stats = dict(processed=int(processed.sum()), fallback=int(processed.sum()) - int(strong.sum()), similar_total=int(total[processed].sum()))
        return out, stats

    def bayes_accumulate_layers(self, layers, mask, nsim, state, w, b, min_eig):
        """bcd_hip_bayes_accumulate_layers: `layers` is a list of (colours, per-pixel covariances) tensors on one selection.
        -> (list of sum images, the shared count image, items per layer that took the redo list)"""
        torch = self.torch
        layers = list(layers)
        H, W = nsim.shape
        sums = [torch.zeros((H, W, 3), dtype=torch.float32, device=nsim.device) for _ in layers]
        c = torch.zeros((H, W), dtype=torch.int32, device=nsim.device)
        arr = (StageLayer * max(1, len(layers)))()
        for k, ((col, pc), s) in enumerate(zip(layers, sums)):
            if tuple(col.shape) != (H, W, 3) or tuple(pc.shape) != (H, W, 6):
                raise ValueError("layer %d: colours must be %dx%dx3 and per-pixel covariances %dx%dx6" % (k, H, W, H, W))
            arr[k].d_colors, arr[k].d_pixel_cov, arr[k].d_sum = _dp(col).value, _dp(pc).value, _dp(s).value
        redo = (C.c_int32 * max(1, len(layers)))()
        self._chk(lib().bcd_hip_bayes_accumulate_layers(self.h, arr, len(layers), _dp(mask), _dp(nsim), _dp(state), W, H, w, b, min_eig, _dp(c), redo))
        return sums, c, list(redo)[:len(layers)]

    @staticmethod
    def _ptr_list(tensors):
        return (C.c_void_p * max(1, len(tensors)))(*[_dp(t).value for t in tensors])

    def layers_pixel_cov(self, covs, ns):
        """bcd_hip_layers_pixel_cov -> (per-pixel covariances L x H x W x 6, sums L x H x W x 3: cleared by the call, handed over filled with ones)"""
        covs = list(covs)
        H, W = ns.shape[:2]
        pc = self.torch.empty((len(covs), H, W, 6), dtype=ns.dtype, device=ns.device)
        s = self.torch.ones((len(covs), H, W, 3), dtype=ns.dtype, device=ns.device)
        self._chk(lib().bcd_hip_layers_pixel_cov(self.h, self._ptr_list(covs), len(covs), _dp(ns), W, H, _dp(pc), _dp(s)))
        return pc, s

    def layers_finalize(self, sums, c):
        sums = list(sums)
        outs = [self.torch.empty_like(s) for s in sums]
        self._chk(lib().bcd_hip_layers_finalize(self.h, self._ptr_list(sums), self._ptr_list(outs), len(sums), _dp(c), c.numel()))
        return outs

    def layers_downscale_avg(self, imgs):
        imgs = list(imgs)
        H, W, D = imgs[0].shape
        outs = [self.torch.empty((H // 2, W // 2, D), dtype=a.dtype, device=a.device) for a in imgs]
        self._chk(lib().bcd_hip_layers_downscale_avg(self.h, self._ptr_list(imgs), self._ptr_list(outs), len(imgs), W, H))
        return outs

    def layers_downscale_cov(self, covs, ns):
        covs = list(covs)
        H, W, D = covs[0].shape
        outs = [self.torch.empty((H // 2, W // 2, D), dtype=a.dtype, device=a.device) for a in covs]
        self._chk(lib().bcd_hip_layers_downscale_cov(self.h, self._ptr_list(covs), self._ptr_list(outs), len(covs), _dp(ns), W, H))
        return outs

    def layers_merge(self, his, los):
        """out of place: clones of `his` merged with `los`"""
        outs = [h.clone() for h in his]
        los = list(los)
        H, W, _ = outs[0].shape
        self._chk(lib().bcd_hip_layers_merge(self.h, self._ptr_list(outs), self._ptr_list(los), len(outs), W, H))
        return outs

    def bayes_last_redo_count(self):
        """items of the last bayes_accumulate call (patch radius 1) whose inverse took the spectral branch through the redo list"""
        n = C.c_int32(0)
        self._chk(lib().bcd_hip_bayes_last_redo_count(self.h, C.byref(n)))
        return n.value

    def finalize(self, s, c):
        out = self.torch.empty_like(s)
        self._chk(lib().bcd_hip_finalize(self.h, _dp(s), _dp(c), c.numel(), _dp(out)))
        return out

    def finalize_band(self, s, c, halo, up, down, out):
        """out (rows x W x 3 view) = finalisation of the accumulator rows s / c with the neighbours' halos (pairs or None) added"""
        rows, W, _ = s.shape
        z = C.c_void_p(0)
        self._chk(lib().bcd_hip_finalize_band(self.h, _dp(s), _dp(c), W, rows, halo, _dp(up[0]) if up else z, _dp(up[1]) if up else z,
                                              _dp(down[0]) if down else z, _dp(down[1]) if down else z, _dp(out)))
        return out

    def downscale_sum(self, a):
        H, W, D = a.shape
        o = self.torch.empty((H // 2, W // 2, D), dtype=a.dtype, device=a.device)
        self._chk(lib().bcd_hip_downscale_sum(self.h, _dp(a), W, H, D, _dp(o)))
        return o

    def downscale_avg(self, a):
        H, W, D = a.shape
        o = self.torch.empty((H // 2, W // 2, D), dtype=a.dtype, device=a.device)
        self._chk(lib().bcd_hip_downscale_avg(self.h, _dp(a), W, H, D, _dp(o)))
        return o

    def downscale_cov(self, cov, ns):
        H, W, D = cov.shape
        o = self.torch.empty((H // 2, W // 2, D), dtype=cov.dtype, device=cov.device)
        self._chk(lib().bcd_hip_downscale_cov(self.h, _dp(cov), _dp(ns), W, H, _dp(o)))
        return o

    def interpolate(self, lo, H, W):
        h, w, D = lo.shape
        o = self.torch.empty((H, W, D), dtype=lo.dtype, device=lo.device)
        self._chk(lib().bcd_hip_interpolate(self.h, _dp(lo), w, h, D, _dp(o), W, H))
        return o

    def merge(self, hi, lo):
        H, W, D = hi.shape
        o = hi.clone()
        self._chk(lib().bcd_hip_merge(self.h, _dp(o), W, H, _dp(lo), D))
        return o

    def merge_(self, hi, lo):
        """in place on hi (a contiguous H x W x D tensor or row-slice view)"""
        H, W, D = hi.shape
        self._chk(lib().bcd_hip_merge(self.h, _dp(hi), W, H, _dp(lo), D))
        return hi

    def spike_filter(self, col, ns, hist, cov, factor):
        H, W, D = hist.shape
        o = [self.torch.empty_like(t) for t in (col, ns, hist, cov)]
        self._chk(lib().bcd_hip_spike_filter(self.h, _dp(col), _dp(ns), _dp(hist), _dp(cov), W, H, D, factor,
                                             _dp(o[0]), _dp(o[1]), _dp(o[2]), _dp(o[3])))
        return o

    def spike_map(self, col, factor, count=True):
        """bcd_hip_spike_map -> (map: H x W int32 tensor of source pixel indices, moved: pixels with map[p] != p -- reading it synchronises; None
        without `count`)"""
        torch = self.torch
        H, W, _ = col.shape
        m = torch.empty((H, W), dtype=torch.int32, device=col.device)
        moved = torch.empty(1, dtype=torch.int32, device=col.device) if count else None
        self._chk(lib().bcd_hip_spike_map(self.h, _dp(col), W, H, factor, _dp(m), _dp(moved) if count else None))
        return m, (int(moved.item()) if count else None)

    def spike_apply(self, map, images, outs=None):
        """bcd_hip_spike_apply: every image of the list (H x W x depth tensors of one depth, at most 32) gathered through the map in one launch.
        Returns the outputs (`outs`: tensors to write into, optional)"""
        images = list(images)
        H, W = map.shape[:2]
        depth = images[0].numel() // (H * W) if images else 1
        if outs is None:
            outs = [self.torch.empty_like(a) for a in images]
        outs = list(outs)
        self._chk(lib().bcd_hip_spike_apply(self.h, _dp(map), W, H, depth, self._ptr_list(images), self._ptr_list(outs), len(images)))
        return outs

    def spike_filter_layers(self, ns, hist, layers, factor, count=False, own_map=True):
        """bcd_hip_spike_filter_layers: `layers` is a list of (colours, covariances); the map comes from layers[0]'s colours.  hist None: the form without
        histograms.  Returns (ns, hist or None, [(colours, covariances), ...], map), all filtered copies; with `count` a fifth value, the moved pixels.
        own_map False: the map stays in the context's scratch and None is returned in its place"""
        torch = self.torch
        layers = list(layers)
        H, W = ns.shape[:2]
        D = hist.shape[-1] if hist is not None else 0
        o_ns = torch.empty_like(ns)
        o_hist = torch.empty_like(hist) if hist is not None else None
        outs = [(torch.empty_like(c), torch.empty_like(v)) for c, v in layers]
        m = torch.empty((H, W), dtype=torch.int32, device=ns.device) if own_map else None
        moved = torch.empty(1, dtype=torch.int32, device=ns.device) if count else None
        arr = (SpikeLayer * max(1, len(layers)))()
        for k, ((c, v), (oc, ov)) in enumerate(zip(layers, outs)):
            arr[k].d_colors, arr[k].d_covariances, arr[k].d_colors_out, arr[k].d_covariances_out = _dp(c).value, _dp(v).value, _dp(oc).value, _dp(ov).value
        self._chk(lib().bcd_hip_spike_filter_layers(self.h, _dp(ns), _dp(hist) if hist is not None else None, W, H, D, factor, _dp(o_ns),
                                                    _dp(o_hist) if hist is not None else None, arr, len(layers), _dp(m) if own_map else None, _dp(moved) if count else None))
        res = (o_ns, o_hist, outs, m)
        return res + (int(moved.item()),) if count else res

    def spike_apply_inplace(self, map, images):
        """bcd_hip_spike_apply_inplace: every image of the list (H x W x depth tensors of any depths, at most 32) gathered through the map IN PLACE: pixel p
        ends with the values pixel map[p] held before the call.  Synchronises.  -> the number of moved pixels"""
        images = list(images)
        H, W = map.shape[:2]
        depths = (C.c_int32 * max(1, len(images)))(*[a.numel() // (H * W) for a in images])
        moved = C.c_int32(-1)
        self.torch.cuda.synchronize(self.device)                     # (the fills ran on torch's stream)
        self._chk(lib().bcd_hip_spike_apply_inplace(self.h, _dp(map), W, H, depths, self._ptr_list(images), len(images), C.byref(moved)))
        return moved.value

    def spike_filter_layers_inplace(self, ns, hist, layers, factor, own_map=True):
        """bcd_hip_spike_filter_layers_inplace: spike_filter_layers IN PLACE on `ns`, `hist` (None: the form without histograms) and the (colours, covariances)
        of `layers`.  Synchronises.  -> (map or None without own_map, moved pixels)"""
        torch = self.torch
        layers = list(layers)
        H, W = ns.shape[:2]
        D = hist.shape[-1] if hist is not None else 0
        m = torch.empty((H, W), dtype=torch.int32, device=ns.device) if own_map else None
        arr = (SpikeLayerInplace * max(1, len(layers)))()
        for k, (c, v) in enumerate(layers):
            arr[k].d_colors, arr[k].d_covariances = _dp(c).value, _dp(v).value
        moved = C.c_int32(-1)
        torch.cuda.synchronize(self.device)
        self._chk(lib().bcd_hip_spike_filter_layers_inplace(self.h, _dp(ns), _dp(hist) if hist is not None else None, W, H, D, factor, arr, len(layers),
                                                            _dp(m) if own_map else None, C.byref(moved)))
        return m, moved.value

    def accumulate_samples(self, samples, weights=None, nbins=20, gamma=2.2, maxval=2.5):
        """samples: (H, W, spp, 3) device tensor; weights: (H, W, spp) or None"""
        torch = self.torch
        H, W, spp, _ = samples.shape
        mk = lambda d: torch.empty((H, W, d), dtype=torch.float32, device=samples.device)
        ns, mean, cov, hist = mk(1), mk(3), mk(6), mk(3 * nbins)
        self._chk(lib().bcd_hip_accumulate_samples(self.h, _dp(samples), _dp(weights) if weights is not None else None, W, H, spp, nbins,
                                                   gamma, maxval, _dp(ns), _dp(mean), _dp(cov), _dp(hist)))
        return ns, mean, cov, hist

    def accumulator(self, W, H, nbins=20, gamma=2.2, maxval=2.5, capacity=0, layers=0, features=0):
        """persistent device SamplesAccumulator of a W x H frame (bcd_hip_accum_*); capacity > 0: scattered batches of up to that many
        samples never allocate; layers > 0: that many extra colour layers accumulated beside the beauty (bcd_hip_accum_create_layers);
        features > 0: that many auxiliary feature channels averaged beside the beauty (bcd_hip_accum_create_features)"""
        return Accumulator(self, W, H, nbins, gamma, maxval, capacity, layers, features)

    def zero_bad_values(self, img):
        self._chk(lib().bcd_hip_zero_bad_values(self.h, _dp(img), img.numel()))
        return img

    # ---- stats / timing
    def set_profiling(self, on):
        self._chk(lib().bcd_hip_set_profiling(self.h, 1 if on else 0))

    def set_concurrent_scales(self, on):
        self._chk(lib().bcd_hip_set_concurrent_scales(self.h, 1 if on else 0))

    def stats(self, scale):
        s = ScaleStats()
        self._chk(lib().bcd_hip_get_stats(self.h, scale, C.byref(s)))
        return s

    def kernel_time(self):
        ms, n = C.c_float(0), C.c_int32(0)
        self._chk(lib().bcd_hip_kernel_time(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def reset_kernel_time(self):
        self._chk(lib().bcd_hip_reset_kernel_time(self.h))

    def selftest_distance_kernels(self, hist, ns, b):
        """(variant, mismatching plane entries) of the production distance kernel against the exact general one on these inputs"""
        H, W, D = hist.shape
        v, n = C.c_int(0), C.c_int64(0)
        self._chk(lib().bcd_hip_selftest_distance_kernels(self.h, _dp(hist), _dp(ns), W, H, D, b, C.byref(v), C.byref(n)))
        return v.value, n.value

    def set_fast_similarity(self, on):
        self._chk(lib().bcd_hip_set_fast_similarity(self.h, 1 if on else 0))

    def set_margin_planes(self, on):
        """the approximate planes as one margin plane (default) or as the T and C planes (bcd_hip_set_margin_planes)"""
        self._chk(lib().bcd_hip_set_margin_planes(self.h, 1 if on else 0))

    def set_cu_share(self, percent):
        self._chk(lib().bcd_hip_set_cu_share(self.h, int(percent)))

    def selftest_approx_distance(self, hist, ns, b):
        """(max relative deviation of a patch distance, pairs with different bin counts, flags) of the approximate distance planes
        against the exact ones on these inputs"""
        H, W, D = hist.shape
        r, n, f = C.c_float(0), C.c_int64(0), C.c_int(0)
        self._chk(lib().bcd_hip_selftest_approx_distance(self.h, _dp(hist), _dp(ns), W, H, D, b, C.byref(r), C.byref(n), C.byref(f)))
        return r.value, n.value, f.value

    def selftest_bin_work(self, hist, ns, b, reps=3):
        """-> (lane_bins, wave_bins, wave_groups, production kernel ms): the arithmetic of the distance kernel on this frame (counting instantiation)"""
        H, W, D = hist.shape
        a, b_, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        ms = C.c_float(0)
        self._chk(lib().bcd_hip_selftest_bin_work(self.h, _dp(hist), _dp(ns), W, H, D, int(b), int(reps), C.byref(a), C.byref(b_), C.byref(c), C.byref(ms)))
        return a.value, b_.value, c.value, ms.value

    def eig27_batch(self, A, production_rule=False):
        """A: (n, 28, 28) symmetric device tensor (row / column 27 zero) -> (eigenvalues (n, 28), eigenvectors (n, 28, 28), kernel ms);
        production_rule: stop at 2e-9 like the estimate chain (no first-order correction) instead of the strict 1e-12"""
        torch = self.torch
        n = A.shape[0]
        eig = torch.zeros((n, 28), dtype=torch.float32, device=A.device)
        V = torch.zeros((n, 28, 28), dtype=torch.float32, device=A.device)
        ms = C.c_float(0)
        self._chk(lib().bcd_hip_eig27_batch_rule(self.h, _dp(A), n, _dp(eig), _dp(V), C.byref(ms), 1 if production_rule else 0))
        return eig, V, ms.value

    def selftest_prepare_solve(self, col, pixcov, mask, items, capacity=None, list_len=None, b=6, cu_share_pct=100):
        """bcd_hip_selftest_prepare_solve: the prepare and eigensolver phases on the list `items` (int32 device tensor of pixel indices line * W + column),
        as two kernels and as the fused kernel, into records for `capacity` items (default: the list's length); list_len: None = the kernels take
        `capacity` items, otherwise the list's length, which they read on the device.  -> number of 32-bit words in which the two sets of records differ"""
        H, W, _ = col.shape
        cap = int(items.numel() if capacity is None else capacity)
        assert mask.shape[0] == H and mask.shape[1] == W and pixcov.shape[:2] == col.shape[:2]
        assert min(cap, cap if list_len is None else int(list_len)) <= items.numel()
        n = C.c_int64(-1)
        self._chk(lib().bcd_hip_selftest_prepare_solve(self.h, _dp(col), _dp(pixcov), _dp(mask), _dp(items), cap, -1 if list_len is None else int(list_len),
                                                       W, H, int(b), int(cu_share_pct), C.byref(n)))
        return n.value

    def selftest_division(self, samples, seed=1):
        n = C.c_int64(-1)
        self._chk(lib().bcd_hip_selftest_division(self.h, seed, samples, C.byref(n)))
        return n.value

    def synchronize(self):
        self.torch.cuda.synchronize(self.device)


class Accumulator:
    """bcd_hip_accum: running sums in HBM, fed in batches (dense rows or scattered samples, each pixel in stream order), snapshots
    that go straight into Context.denoise"""

    def __init__(self, ctx, W, H, nbins=20, gamma=2.2, maxval=2.5, capacity=0, layers=0, features=0):
        self.ctx, self.W, self.H, self.nbins, self.layers, self.features = ctx, W, H, nbins, int(layers), int(features)
        h = _VP()
        if features:                                                 # (0: no feature channels; anything else is checked by the library)
            ctx._chk(lib().bcd_hip_accum_create_features(ctx.h, W, H, nbins, gamma, maxval, capacity, int(layers), int(features), C.byref(h)))
        elif layers:                                                 # (0: the plain accumulator; anything else is checked by the library)
            ctx._chk(lib().bcd_hip_accum_create_layers(ctx.h, W, H, nbins, gamma, maxval, capacity, int(layers), C.byref(h)))
        else:
            ctx._chk(lib().bcd_hip_accum_create(ctx.h, W, H, nbins, gamma, maxval, capacity, C.byref(h)))
        self.h = h
        ctx._accumulators.add(self)

    def _chk(self, rc):
        self.ctx._chk(rc)

    @staticmethod
    def _layer_list(layers, shape):
        """the host array of device pointers of a _layers add (None for a tensor that is None: the library refuses it)"""
        layers = list(layers)
        arr = (_VP * max(1, len(layers)))()
        for k, t in enumerate(layers):
            if t is not None:
                assert shape(t), "layer %d: not laid out like the beauty's buffer" % k
                arr[k] = _dp(t).value
        return arr

    def nb_layers(self):
        n = C.c_int(0)
        self._chk(lib().bcd_hip_accum_nb_layers(self.h, C.byref(n)))
        return n.value

    def nb_features(self):
        n = C.c_int(0)
        self._chk(lib().bcd_hip_accum_nb_features(self.h, C.byref(n)))
        return n.value

    def _feature_args(self, features, layers, lead, layer_shape):
        """(layer list or None, feature pointer) of a _features add; features: a float32 tensor of shape lead + (F,), required exactly when the
        accumulator has feature channels (a plain add on such an accumulator, or features on one without, is refused by the library)"""
        assert tuple(features.shape) == tuple(lead) + (self.features,) and features.dtype == self.ctx.torch.float32, \
            "features: one float32 value per sample and channel, laid out like the samples"
        arr = None
        if layers is not None:
            layers = list(layers)
            assert len(layers) == self.layers, "one tensor per layer expected"
            arr = self._layer_list(layers, layer_shape)
        return arr, (_dp(features) if features.numel() else None)

    def add_dense(self, samples, weights=None, row0=0, layers=None, features=None):
        """samples: (rows, W, k, 3 | 4) device tensor, the k samples of a pixel in accumulation order; weights: (rows, W, k) or None;
        layers: on an accumulator with layers, one (rows, W, k, 3 | 4) tensor per layer (all of one channel count); features: on an
        accumulator with feature channels, a (rows, W, k, F) tensor"""
        rows, W, k, ch = samples.shape
        assert W == self.W, "samples must cover whole rows of the frame"
        assert weights is None or tuple(weights.shape) == (rows, W, k)
        wp = _dp(weights) if weights is not None else None
        if features is not None:
            lch = next((t.shape[3] for t in (layers or ()) if t is not None), 3)
            arr, fp = self._feature_args(features, layers, (rows, W, k), lambda t: tuple(t.shape) == (rows, W, k, lch))
            self._chk(lib().bcd_hip_accum_add_dense_features(self.h, _dp(samples), wp, int(row0), rows, k, ch, arr, lch, fp))
            return
        if layers is None:
            self._chk(lib().bcd_hip_accum_add_dense(self.h, _dp(samples), wp, int(row0), rows, k, ch))
            return
        layers = list(layers)
        assert len(layers) == self.layers, "one tensor per layer expected"
        lch = next((t.shape[3] for t in layers if t is not None), 3)
        arr = self._layer_list(layers, lambda t: tuple(t.shape) == (rows, W, k, lch))
        self._chk(lib().bcd_hip_accum_add_dense_layers(self.h, _dp(samples), wp, int(row0), rows, k, ch, arr, lch))

    def add_samples(self, pixel, rgb, weights=None, layers=None, features=None):
        """pixel: (n,) int32 line * W + col (others are dropped and counted); rgb: (n, 3); weights: (n,) or None; layers: on an
        accumulator with layers, one (n, 3) tensor per layer; features: on an accumulator with feature channels, an (n, F) tensor"""
        n = pixel.shape[0]
        assert pixel.dtype == self.ctx.torch.int32 and tuple(rgb.shape) == (n, 3)
        assert weights is None or tuple(weights.shape) == (n,)
        wp = _dp(weights) if weights is not None else None
        if features is not None:
            arr, fp = self._feature_args(features, layers, (n,), lambda t: tuple(t.shape) == (n, 3))
            self._chk(lib().bcd_hip_accum_add_scattered_features(self.h, _dp(pixel), _dp(rgb), wp, n, arr, fp))
            return
        if layers is None:
            self._chk(lib().bcd_hip_accum_add_scattered(self.h, _dp(pixel), _dp(rgb), wp, n))
            return
        layers = list(layers)
        assert len(layers) == self.layers, "one tensor per layer expected"
        arr = self._layer_list(layers, lambda t: tuple(t.shape) == (n, 3))
        self._chk(lib().bcd_hip_accum_add_scattered_layers(self.h, _dp(pixel), _dp(rgb), wp, n, arr))

    def set_filter(self, kind_or_table, radius=None, param=2.0, table_size=16):
        """the pixel reconstruction filter of add_splatted (bcd_hip_accum_set_filter; definition in include/bcd_hip.h).  kind_or_table: a
        kind of filter_table() ("box", "tent", "gaussian", "blackman_harris"; param = the Gaussian's alpha), a square float32 array of
        finite values >= 0 (row = y index), or None to remove the filter; radius: a number or (radius_x, radius_y), each in (0, 3].
        The filter is not part of an exported state."""
        import numpy as np
        if kind_or_table is None:
            self._chk(lib().bcd_hip_accum_set_filter(self.h, 0.0, 0.0, 0, None))
            return
        rx, ry = _radii(radius)
        if isinstance(kind_or_table, str):
            table = filter_table(kind_or_table, (rx, ry), param, table_size)
        else:
            table = np.ascontiguousarray(kind_or_table, np.float32)
            if table.ndim != 2 or table.shape[0] != table.shape[1]:
                raise ValueError("a filter table must be a square 2-D array")
        self._chk(lib().bcd_hip_accum_set_filter(self.h, rx, ry, table.shape[0], table.ctypes.data_as(_VP)))

    def add_splatted(self, xy, rgb, weights=None, layers=None, features=None):
        """xy: (n, 2) float32 continuous positions (x, y), pixel (col, line) covering [col, col + 1) x [line, line + 1); rgb: (n, 3);
        weights: (n,) or None.  Every sample goes to the pixels of its filter footprint, each pixel in stream order.  layers: on an
        accumulator with layers, one (n, 3) tensor per layer; features: on an accumulator with feature channels, an (n, F) tensor"""
        n = xy.shape[0]
        assert tuple(xy.shape) == (n, 2) and tuple(rgb.shape) == (n, 3) and xy.dtype == self.ctx.torch.float32
        assert weights is None or tuple(weights.shape) == (n,)
        args = (self.h, _dp(xy) if n else None, _dp(rgb) if n else None, _dp(weights) if weights is not None and n else None, n)
        if features is not None:
            arr, fp = self._feature_args(features, layers if n else None, (n,), lambda t: tuple(t.shape) == (n, 3))
            if layers is not None and not n:
                arr = (_VP * max(1, self.layers))()
            self._chk(lib().bcd_hip_accum_add_splatted_features(*args, arr, fp))
            return
        if layers is None:
            self._chk(lib().bcd_hip_accum_add_splatted(*args))
            return
        layers = list(layers)
        assert len(layers) == self.layers, "one tensor per layer expected"
        arr = self._layer_list(layers, lambda t: tuple(t.shape) == (n, 3)) if n else (_VP * max(1, len(layers)))()
        self._chk(lib().bcd_hip_accum_add_splatted_layers(*args, arr))

    def layer_statistics(self, out=None):
        """-> [(mean (H, W, 3), cov (H, W, 6)) per layer], fresh tensors or the pairs of `out`, from the layers' sums and the shared weight
        sums (bcd_hip_accum_layer_statistics); state unchanged.  Appended to [(mean, cov)] of statistics() it is the layer list of
        Context.denoise_layers"""
        torch = self.ctx.torch
        if out is None:
            mk = lambda d: torch.empty((self.H, self.W, d), dtype=torch.float32, device="cuda:%d" % self.ctx.device)
            out = [(mk(3), mk(6)) for _ in range(self.layers)]
        out = [tuple(o) for o in out]
        assert len(out) == self.layers or self.layers == 0, "one (mean, cov) pair per layer expected"
        means, covs = (_VP * max(1, len(out)))(), (_VP * max(1, len(out)))()
        for k, (m, c) in enumerate(out):
            assert tuple(m.shape) == (self.H, self.W, 3) and tuple(c.shape) == (self.H, self.W, 6)
            means[k], covs[k] = _dp(m).value, _dp(c).value
        self._chk(lib().bcd_hip_accum_layer_statistics(self.h, means, covs))
        return out

    def feature_statistics(self, out=None, variances=True):
        """-> (features (H, W, F), variances (H, W, F) or None), fresh tensors or the pair of `out`: every channel's weighted mean over
        the pixel's samples and the variance of that mean (bcd_hip_accum_feature_statistics); state unchanged.  They go into
        Context.denoise_guided(..., features, variances=...) and similarity_masks_guide unchanged"""
        torch = self.ctx.torch
        if out is None:
            mk = lambda: torch.empty((self.H, self.W, max(self.features, 1)), dtype=torch.float32, device="cuda:%d" % self.ctx.device)
            out = (mk(), mk() if variances else None)
        f, v = out
        assert tuple(f.shape) == (self.H, self.W, f.shape[2]) and (v is None or tuple(v.shape) == tuple(f.shape))
        assert f.shape[2] == self.features or self.features == 0, "one value per pixel and channel expected"
        self._chk(lib().bcd_hip_accum_feature_statistics(self.h, _dp(f), _dp(v) if v is not None else None))
        return f, v

    def moments(self, out=None):
        """-> (ns (H, W, 1), mean (H, W, 3), cov (H, W, 6)), fresh tensors or the three of `out`: statistics() without the histograms, bit for bit
        (bcd_hip_accum_moments: no bin is read or written); state unchanged"""
        torch = self.ctx.torch
        if out is None:
            mk = lambda d: torch.empty((self.H, self.W, d), dtype=torch.float32, device="cuda:%d" % self.ctx.device)
            out = (mk(1), mk(3), mk(6))
        self._chk(lib().bcd_hip_accum_moments(self.h, *[_dp(t) for t in out]))
        return out

    def statistics(self, out=None):
        """-> (ns (H, W, 1), mean (H, W, 3), cov (H, W, 6), hist (H, W, 3 nbins)), fresh tensors or the four of `out`; state unchanged"""
        torch = self.ctx.torch
        if out is None:
            mk = lambda d: torch.empty((self.H, self.W, d), dtype=torch.float32, device="cuda:%d" % self.ctx.device)
            out = (mk(1), mk(3), mk(6), mk(3 * self.nbins))
        self._chk(lib().bcd_hip_accum_statistics(self.h, *[_dp(t) for t in out]))
        return out

    def reset(self):
        self._chk(lib().bcd_hip_accum_reset(self.h))

    def plan(self, budget, offset=0, threshold=0.0, eps=1e-3, min_samples=2.0, max_per_pixel=16, error=False):
        """where the next `budget` samples go (bcd_hip_accum_plan); the state is unchanged.
        -> (pixels (T,) int32 device tensor in ascending order, pixel p repeated counts[p] times -- the `pixel` of add_samples;
            counts (H, W) int32; the error image (H, W) float32 if `error` else None;
            summary dict: planned (T), active, unsampled, max_error).
        The kernels keep T on the device; this convenience synchronises the stream once to read the summary and trim the list."""
        if not 0 <= int(budget) < 2 ** 31:                           # (before the list buffer is allocated)
            raise ValueError("budget must be in [0, 2^31), got %d" % int(budget))
        torch = self.ctx.torch
        dev = "cuda:%d" % self.ctx.device
        prm = PlanParams(threshold, eps, min_samples, max_per_pixel)
        pixels = torch.empty((max(int(budget), 1),), dtype=torch.int32, device=dev)
        counts = torch.empty((self.H, self.W), dtype=torch.int32, device=dev)
        err = torch.empty((self.H, self.W), dtype=torch.float32, device=dev) if error else None
        summ = torch.empty((C.sizeof(PlanSummary) // 8,), dtype=torch.int64, device=dev)
        self._chk(lib().bcd_hip_accum_plan(self.h, C.byref(prm), int(budget), int(offset), _dp(err) if error else None, _dp(counts), _dp(pixels),
                                           pixels.numel(), C.cast(_dp(summ), C.POINTER(PlanSummary))))
        torch.cuda.synchronize(self.ctx.device)                     # the context's stream may not be torch's
        s = summ.cpu()
        T = int(s[0])
        summary = {"planned": T, "active": int(s[1]), "unsampled": int(s[2]), "max_error": float(s[3:4].view(torch.float32)[0])}
        return pixels[:T], counts, err, summary

    # ---- states (bcd_hip_accum_export / _import / _merge_state / _merge; format v1 and merge definition in include/bcd_hip.h)
    def state_bytes(self):
        n = C.c_int64(0)
        self._chk(lib().bcd_hip_accum_state_bytes(self.h, C.byref(n)))
        return n.value

    def export_state(self):
        """the serialised state (header + planes) as a numpy uint8 array; synchronises, the state is unchanged"""
        import numpy as np
        out = np.empty(self.state_bytes(), np.uint8)
        self._chk(lib().bcd_hip_accum_export(self.h, out.ctypes.data_as(_VP), out.size))
        return out

    def import_state(self, buf):
        """replaces the state and the counters with a serialised state of the same geometry and parameters"""
        a = _state_buffer(buf)
        self._chk(lib().bcd_hip_accum_import(self.h, a.ctypes.data_as(_VP) if a.size else None, a.size))

    def merge_state(self, buf):
        """adds a serialised state into this one (one fp32 add per element); returns once buf is no longer needed"""
        a = _state_buffer(buf)
        self._chk(lib().bcd_hip_accum_merge_state(self.h, a.ctypes.data_as(_VP) if a.size else None, a.size))

    def merge(self, other):
        """adds other's state into this one, in stream order on both contexts (other may live on another context or device); the layer
        and the feature planes too (both sides must have the same number of layers and of feature channels)"""
        self._chk(lib().bcd_hip_accum_merge(self.h, other.h if other is not None else None))

    # ---- the layer block (bcd_hip_accum_export_layers / _import_layers / _merge_layers_state): a checkpoint of an accumulator with layers
    # is export_state() plus export_layers_state()
    def layers_state_bytes(self):
        n = C.c_int64(0)
        self._chk(lib().bcd_hip_accum_layers_state_bytes(self.h, C.byref(n)))
        return n.value

    def export_layers_state(self):
        """the serialised layer block (header + the layers' planes) as a numpy uint8 array; synchronises, the state is unchanged"""
        import numpy as np
        out = np.empty(self.layers_state_bytes(), np.uint8)
        self._chk(lib().bcd_hip_accum_export_layers(self.h, out.ctypes.data_as(_VP), out.size))
        return out

    def import_layers_state(self, buf):
        """replaces the layers' planes with a serialised block of the same frame size and layer count"""
        a = _state_buffer(buf)
        self._chk(lib().bcd_hip_accum_import_layers(self.h, a.ctypes.data_as(_VP) if a.size else None, a.size))

    def merge_layers_state(self, buf):
        """adds a serialised layer block into the layers' planes (one fp32 add per element)"""
        a = _state_buffer(buf)
        self._chk(lib().bcd_hip_accum_merge_layers_state(self.h, a.ctypes.data_as(_VP) if a.size else None, a.size))

    # ---- the feature block (bcd_hip_accum_export_features / _import_features / _merge_features_state): a checkpoint of an accumulator with
    # feature channels is export_state() plus export_features_state() (plus export_layers_state() if it has layers)
    def features_state_bytes(self):
        n = C.c_int64(0)
        self._chk(lib().bcd_hip_accum_features_state_bytes(self.h, C.byref(n)))
        return n.value

    def export_features_state(self):
        """the serialised feature block (header + the feature planes) as a numpy uint8 array; synchronises, the state is unchanged"""
        import numpy as np
        out = np.empty(self.features_state_bytes(), np.uint8)
        self._chk(lib().bcd_hip_accum_export_features(self.h, out.ctypes.data_as(_VP), out.size))
        return out

    def import_features_state(self, buf):
        """replaces the feature planes with a serialised block of the same frame size and channel count"""
        a = _state_buffer(buf)
        self._chk(lib().bcd_hip_accum_import_features(self.h, a.ctypes.data_as(_VP) if a.size else None, a.size))

    def merge_features_state(self, buf):
        """adds a serialised feature block into the feature planes (one fp32 add per element)"""
        a = _state_buffer(buf)
        self._chk(lib().bcd_hip_accum_merge_features_state(self.h, a.ctypes.data_as(_VP) if a.size else None, a.size))

    def info(self):
        """(samples accumulated, samples dropped) since create / the last reset; synchronises"""
        a, d = C.c_int64(0), C.c_int64(0)
        self._chk(lib().bcd_hip_accum_info(self.h, C.byref(a), C.byref(d)))
        return a.value, d.value

    def close(self):
        if self.h:
            lib().bcd_hip_accum_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Selection:
    """bcd_hip_selection: the similar-patch selection of a frame, kept by Context.denoise_layers(..., keep=sel) so that further layers of that frame
    cost the estimate stage alone"""

    def __init__(self, ctx):
        h = _VP()
        rc = lib().bcd_hip_selection_create(ctx.h, C.byref(h))
        if rc != 0 or not h.value:
            raise BcdHipError("bcd_hip_selection_create failed: rc=%d" % rc)
        self.ctx, self.h = ctx, h
        ctx._selections.add(self)

    def _handle(self):
        if not self.h:
            raise BcdHipError("the selection is closed")
        return self.h

    def denoise(self, layers, ns=None, outs=None):
        """bcd_hip_selection_denoise: the estimate stage on the kept selection for a list of (colours, covariances) tensors of the kept frame size;
        ns: sample counts that replace the kept ones in the estimate stage (None: the kept ones).  Returns the list of outputs"""
        h = self._handle()
        info = self.info()
        layers = list(layers)
        if info["valid"]:
            H, W = info["H"], info["W"]
        else:                                                        # (the library refuses the call; shapes from the first layer so that it gets there)
            H, W = (layers[0][0].shape[0], layers[0][0].shape[1]) if layers else (1, 1)
        dev = layers[0][0].device if layers else "cuda:%d" % self.ctx.device
        arr, layers, outs = self.ctx._layer_array(layers, outs, H, W, dev)
        if ns is not None and ns.numel() != H * W:
            raise ValueError("sample counts must be %dx%d" % (H, W))
        self.ctx._chk(lib().bcd_hip_selection_denoise(h, _dp(ns) if ns is not None else None, arr, len(layers)))
        return outs

    def info(self):
        """bcd_hip_selection_info as a dict (host only): valid, W, H, D, nb_scales, params, device_bytes, scales = [dict(width, height, processed,
        fallback, similar_total, similarity_path)]"""
        i = SelectionInfo()
        rc = lib().bcd_hip_selection_info(self._handle(), C.byref(i))
        if rc != 0:
            raise BcdHipError("bcd_hip_selection_info: rc=%d" % rc)
        p = Params()
        C.memmove(C.byref(p), C.byref(i.params), C.sizeof(Params))
        return {"valid": bool(i.valid), "W": i.W, "H": i.H, "D": i.D, "nb_scales": i.nb_scales, "params": p, "device_bytes": i.device_bytes,
                "scales": [{k: getattr(i.scale[s], k) for k, _ in SelectionScale._fields_ if k != "reserved"} for s in range(i.nb_scales)]}

    def read(self, scale):
        """bcd_hip_selection_read -> (mask (h, w, words) int32, |S| (h, w) int32, states (h, w) uint8, count image (h, w) int32) of one scale, in the
        layouts of Context.similarity_masks / active_set"""
        h = self._handle()
        torch = self.ctx.torch
        info = self.info()
        if not info["valid"] or not 0 <= scale < info["nb_scales"]:
            hh, ww, words = 1, 1, 1                                  # (the library refuses the call)
        else:
            hh, ww = info["scales"][scale]["height"], info["scales"][scale]["width"]
            words = ((2 * info["params"].search_radius + 1) ** 2 + 31) // 32
        dev = "cuda:%d" % self.ctx.device
        mask = torch.zeros((hh, ww, words), dtype=torch.int32, device=dev)
        nsim = torch.zeros((hh, ww), dtype=torch.int32, device=dev)
        state = torch.zeros((hh, ww), dtype=torch.uint8, device=dev)
        count = torch.zeros((hh, ww), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(self.ctx.device)                      # (the fills ran on torch's stream)
        self.ctx._chk(lib().bcd_hip_selection_read(h, int(scale), _dp(mask), _dp(nsim), _dp(state), _dp(count)))
        return mask, nsim, state, count

    def close(self):
        if self.h:
            lib().bcd_hip_selection_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Sequence:
    """bcd_hip_sequence: the frames of an animation pushed one by one and popped denoised, each with its neighbours within `radius` frames (what
    Context.denoise_temporal returns for it).  Every frame is copied and its pyramid built once; every pair of frames is searched once -- the second
    cross pass of a pair is a transposition of the first one's masks"""

    def __init__(self, ctx, W, H, D, nscales, radius, prm, mode=None):
        h = _VP()
        self.mode = mode
        if mode is None:
            ctx._chk(lib().bcd_hip_sequence_create(ctx.h, int(W), int(H), int(D), int(nscales), int(radius), C.byref(prm), C.byref(h)))
        else:
            # ("Modes": push(ns, hist or None, [(colours, covariances), ...], features, variances), pop() -> (index, [layer, ...]))
            floors = (C.c_float * max(1, len(mode["feature_floors"])))(*mode["feature_floors"])
            if mode["features"] and len(mode["feature_floors"]) != mode["features"]:
                raise ValueError("feature_floors must hold one floor per feature channel")
            m = SequenceMode(mode["layers"], int(mode["moments"]), mode["var_floor"], mode["features"], int(mode["feature_variances"]),
                             C.addressof(floors) if mode["features"] else None, mode["feature_threshold"], None)
            ctx._chk(lib().bcd_hip_sequence_create_mode(ctx.h, int(W), int(H), int(D), int(nscales), int(radius), C.byref(prm), C.byref(m), C.byref(h)))
        self.ctx, self.h = ctx, h
        self.W, self.H, self.D, self.nscales, self.radius = int(W), int(H), int(D), int(nscales), int(radius)
        self.b = prm.search_radius
        ctx._selections.add(self)                                    # (closed with the context, like a selection)

    def _handle(self):
        if not self.h:
            raise BcdHipError("the sequence is closed")
        return self.h

    def _check(self, col, ns, hist, cov):
        H, W, D = self.H, self.W, self.D
        nns = ns.numel() if hasattr(ns, "numel") else ns.size
        shapes = (tuple(col.shape), int(nns), tuple(hist.shape), tuple(cov.shape))
        if shapes != ((H, W, 3), H * W, (H, W, D), (H, W, 6)):
            raise ValueError("a frame of this sequence is colours %dx%dx3, sample counts %dx%d, histograms %dx%dx%d, covariances %dx%dx6" % (H, W, H, W, H, W, D, H, W))

    def _frame(self, ns, hist, layers, features, variances, ptr):
        """the bcd_hip_sequence_frame of a frame in a mode (+ the objects it points into): ns, hist (None in a moments sequence), a list of (colours,
        covariances), features / variances (H, W, F) or None; ptr(a) is an address.  Shapes are checked here, the mode's rules by the library"""
        H, W, D, m = self.H, self.W, self.D, self.mode
        layers = list(layers)
        nns = ns.numel() if hasattr(ns, "numel") else ns.size
        if int(nns) != H * W or (hist is not None and tuple(hist.shape) != (H, W, D)):
            raise ValueError("a frame of this sequence has sample counts %dx%d and histograms %dx%dx%d" % (H, W, H, W, D))
        for k, (col, cov) in enumerate(layers):
            if tuple(col.shape) != (H, W, 3) or tuple(cov.shape) != (H, W, 6):
                raise ValueError("layer %d: colours must be %dx%dx3 and covariances %dx%dx6" % (k, H, W, H, W))
        for a in (features, variances):
            if a is not None and tuple(a.shape) != (H, W, m["features"]):
                raise ValueError("features and variances must be %dx%dx%d" % (H, W, m["features"]))
        arr = (FrameLayer * max(1, m["layers"]))()
        for k, (col, cov) in enumerate(layers[:m["layers"]]):
            arr[k] = FrameLayer(ptr(col), ptr(cov))
        opt = lambda a: None if a is None else ptr(a)
        # (a frame with too few layers reaches the library with a NULL layer and is refused there; one with too many is refused here)
        if len(layers) > m["layers"]:
            raise ValueError("a frame of this sequence has %d layers" % m["layers"])
        return SequenceFrame(ptr(ns), opt(hist), C.addressof(arr), opt(features), opt(variances), None), (arr, layers, ns, hist, features, variances)

    def _mode_args(self, frame, features, variances):
        """(ns, hist, layers, features, variances) of a push in a mode: features and variances may follow the layers positionally"""
        if not 3 <= len(frame) <= 5:
            raise TypeError("a frame of a sequence in a mode is (ns, hist or None, [(colours, covariances), ...][, features[, variances]])")
        rest = list(frame[3:]) + [None, None]
        return frame[0], frame[1], frame[2], rest[0] if features is None else features, rest[1] if variances is None else variances

    def _fields(self, motion, numel, conv=lambda a: a):
        """the step fields of a push from its keywords motion_prev / motion_next: None (zero motion) or (H, W, 2) floats each; only a sequence in a mode
        takes them.  -> None when neither keyword was given (a push without fields), else (prev, next)"""
        if set(motion) - {"motion_prev", "motion_next"}:
            raise TypeError("unexpected keyword %r" % sorted(set(motion) - {"motion_prev", "motion_next"})[0])
        if not motion:
            return None
        if self.mode is None:
            raise ValueError("motion fields are pushed to a sequence in a mode (Context.sequence(..., layers=1) is the plain sequence as one)")
        fields = tuple(None if motion.get(k) is None else conv(motion[k]) for k in ("motion_prev", "motion_next"))
        for m in fields:
            if m is not None and numel(m) != self.H * self.W * 2:
                raise ValueError("a motion field of this sequence holds (%d, %d, 2) floats" % (self.H, self.W))
        return fields

    def push(self, *frame, features=None, variances=None, **motion):
        """bcd_hip_sequence_push: the next frame, device tensors (copied: they are free again on return) -- (col, ns, hist, cov).
        In a mode (bcd_hip_sequence_push_frame): (ns, hist or None, [(colours, covariances), ...], features=None, variances=None); motion_prev / motion_next
        (bcd_hip_sequence_push_frame_motion, when either keyword is given): the (H, W, 2) fields of this frame towards the frame before and after it,
        None: zero motion"""
        h = self._handle()
        fields = self._fields(motion, lambda m: m.numel())
        if self.mode is not None:
            f, keep = self._frame(*self._mode_args(frame, features, variances), ptr=_dptr)
            self.ctx.torch.cuda.synchronize(self.ctx.device)
            if fields is None:
                self.ctx._chk(lib().bcd_hip_sequence_push_frame(h, C.byref(f)))
            else:
                self.ctx._chk(lib().bcd_hip_sequence_push_frame_motion(h, C.byref(f), *(None if m is None else _dp(m) for m in fields)))
            return
        col, ns, hist, cov = frame
        self._check(col, ns, hist, cov)
        self.ctx.torch.cuda.synchronize(self.ctx.device)
        self.ctx._chk(lib().bcd_hip_sequence_push(h, _dp(col), _dp(ns), _dp(hist), _dp(cov)))

    def push_host(self, *frame, features=None, variances=None, **motion):
        """bcd_hip_sequence_push_host: the next frame, NumPy arrays (uploaded once); the arguments of push"""
        import numpy as np
        h = self._handle()
        as32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        fields = self._fields(motion, np.size, as32)
        if self.mode is not None:
            ns, hist, layers, features, variances = self._mode_args(frame, features, variances)
            f, keep = self._frame(as32(ns), as32(hist), [(as32(c), as32(v)) for c, v in layers], as32(features), as32(variances), ptr=_hptr)
            if fields is None:
                self.ctx._chk(lib().bcd_hip_sequence_push_frame_host(h, C.byref(f)))
            else:
                self.ctx._chk(lib().bcd_hip_sequence_push_frame_motion_host(h, C.byref(f), *(None if m is None else C.c_void_p(_hptr(m)) for m in fields)))
            return
        col, ns, hist, cov = frame
        col, ns, hist, cov = (np.ascontiguousarray(a, np.float32) for a in (col, ns, hist, cov))
        self._check(col, ns, hist, cov)
        self.ctx._chk(lib().bcd_hip_sequence_push_host(h, _hptr(col), _hptr(ns), _hptr(hist), _hptr(cov)))

    def end(self):
        """no further frame follows: the frames still held become ready"""
        self.ctx._chk(lib().bcd_hip_sequence_end(self._handle()))

    def ready(self):
        """frames that can be popped now"""
        return lib().bcd_hip_sequence_ready(self._handle())

    def pop(self, out=None):
        """bcd_hip_sequence_pop -> (frame index, the denoised frame as a (H, W, 3) device tensor); in a mode (bcd_hip_sequence_pop_layers) the list of the
        denoised layers in its place (`out`: a list of tensors to write into)"""
        h = self._handle()
        torch = self.ctx.torch
        if self.mode is not None:
            outs = [torch.empty((self.H, self.W, 3), dtype=torch.float32, device="cuda:%d" % self.ctx.device) for _ in range(self.mode["layers"])] if out is None else list(out)
            ptrs = (C.c_void_p * max(1, len(outs)))(*[_dptr(o) for o in outs])
            idx = C.c_int64(-1)
            torch.cuda.synchronize(self.ctx.device)
            self.ctx._chk(lib().bcd_hip_sequence_pop_layers(h, ptrs, len(outs), C.byref(idx)))
            return idx.value, outs
        if out is None:
            out = torch.empty((self.H, self.W, 3), dtype=torch.float32, device="cuda:%d" % self.ctx.device)
        idx = C.c_int64(-1)
        torch.cuda.synchronize(self.ctx.device)
        self.ctx._chk(lib().bcd_hip_sequence_pop(h, _dp(out), C.byref(idx)))
        return idx.value, out

    def pop_host(self):
        """bcd_hip_sequence_pop_host -> (frame index, the denoised frame as a (H, W, 3) NumPy array)"""
        import numpy as np
        h = self._handle()
        idx = C.c_int64(-1)
        if self.mode is not None:                                     # (bcd_hip_sequence_pop_layers_host -> the list of the denoised layers)
            outs = [np.empty((self.H, self.W, 3), np.float32) for _ in range(self.mode["layers"])]
            ptrs = (C.c_void_p * len(outs))(*[_hptr(o) for o in outs])
            self.ctx._chk(lib().bcd_hip_sequence_pop_layers_host(h, ptrs, len(outs), C.byref(idx)))
            return idx.value, outs
        out = np.empty((self.H, self.W, 3), np.float32)
        self.ctx._chk(lib().bcd_hip_sequence_pop_host(h, _hptr(out), C.byref(idx)))
        return idx.value, out

    def set_reuse(self, on):
        """False: every pair is searched directly from both sides (comparisons, tests)"""
        self.ctx._chk(lib().bcd_hip_sequence_set_reuse(self._handle(), int(bool(on))))

    def set_prefilter(self, factor):
        """bcd_hip_sequence_set_prefilter: every frame pushed from now on passes through the spike prefilter with this factor, once, in place in its slot
        (<= 0: off).  Accepted while the sequence holds no frame"""
        self.ctx._chk(lib().bcd_hip_sequence_set_prefilter(self._handle(), float(factor)))

    def prefilter_info(self):
        """bcd_hip_sequence_prefilter_info -> (frames filtered, pixels moved) since the creation or the last reset"""
        n, m = C.c_int64(0), C.c_int64(0)
        self.ctx._chk(lib().bcd_hip_sequence_prefilter_info(self._handle(), C.byref(n), C.byref(m)))
        return n.value, m.value

    def motion_info(self):
        """bcd_hip_sequence_motion_info -> (neighbours warped, fields composed) by the pops since the creation or the last reset"""
        n, m = C.c_int64(0), C.c_int64(0)
        self.ctx._chk(lib().bcd_hip_sequence_motion_info(self._handle(), C.byref(n), C.byref(m)))
        return n.value, m.value

    def last_masks(self, neighbour, scale=0):
        """bcd_hip_sequence_last_masks -> (mask, count) of the last popped frame at `scale`: neighbour 0 its in-frame set, 1 .. its neighbours in ascending
        frame order"""
        h = self._handle()
        hh, ww = (self.H >> scale, self.W >> scale) if 0 <= scale < self.nscales else (1, 1)
        mask, cnt = _mask_and_count(hh, ww, self.b, "cuda:%d" % self.ctx.device)
        self.ctx.torch.cuda.synchronize(self.ctx.device)             # (the fills ran on torch's stream)
        self.ctx._chk(lib().bcd_hip_sequence_last_masks(h, int(neighbour), int(scale), _dp(mask), _dp(cnt)))
        return mask, cnt

    def info(self):
        """bcd_hip_sequence_info as a dict: frames_pushed, frames_popped, device_bytes, bytes_uploaded, pyramids_built, cross_computed, cross_transposed"""
        i = SequenceInfo()
        self.ctx._chk(lib().bcd_hip_sequence_info(self._handle(), C.byref(i)))
        return {k: getattr(i, k) for k, _ in SequenceInfo._fields_}

    def mode_info(self):
        """bcd_hip_sequence_mode_info as a dict: nb_layers, moments, nb_features, feature_variances, cross_feature_passes (the cross feature passes the pops
        launched: one per gated neighbour and scale, none for a transposed neighbour)"""
        i = SequenceModeInfo()
        self.ctx._chk(lib().bcd_hip_sequence_mode_info(self._handle(), C.byref(i)))
        return {k: getattr(i, k) for k, _ in SequenceModeInfo._fields_ if k != "reserved"}

    def reset(self):
        """forgets every frame and counter; the buffers stay"""
        self.ctx._chk(lib().bcd_hip_sequence_reset(self._handle()))

    def close(self):
        if self.h:
            lib().bcd_hip_sequence_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiDenoiser:
    """bcd_hip_multi: one frame over several GPUs (or several virtual ranks on one GPU); host buffers in and out"""

    def __init__(self, devices):
        h = _VP()
        arr = (C.c_int * len(devices))(*devices)
        rc = lib().bcd_hip_multi_create(C.byref(h), arr, len(devices))
        if rc != 0:
            raise BcdHipError("bcd_hip_multi_create failed: rc=%d" % rc)
        self.h = h

    def close(self):
        if self.h:
            lib().bcd_hip_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def denoise_host(self, col, ns, hist, cov, nscales, prm):
        import numpy as np
        H, W, D = hist.shape
        out = np.empty((H, W, 3), np.float32)
        rc = lib().bcd_hip_multi_denoise_host(self.h, _fptr(col), _fptr(ns), _fptr(hist), _fptr(cov), W, H, D, nscales, C.byref(prm), _fptr(out))
        if rc != 0:
            raise BcdHipError("rc=%d: %s" % (rc, lib().bcd_hip_multi_last_error(self.h).decode()))
        return out

    def stats(self):
        s = MultiStats()
        lib().bcd_hip_multi_get_stats(self.h, C.byref(s))
        return s

    def set_comm_trace(self, on):
        lib().bcd_hip_multi_set_comm_trace(self.h, 1 if on else 0)

    def set_frame_timeout(self, milliseconds):
        lib().bcd_hip_multi_set_frame_timeout(self.h, int(milliseconds))

    def comm_trace(self, rank):
        """[(channel, kind, bytes_up, bytes_down), ...] of the last frame, in the order `rank` enqueued its operations"""
        n = lib().bcd_hip_multi_get_comm_trace(self.h, rank, None, 0)
        buf = (C.c_int64 * max(1, n))()
        n = lib().bcd_hip_multi_get_comm_trace(self.h, rank, buf, n)
        v = list(buf[:n])
        return [tuple(v[i:i + 4]) for i in range(0, n, 4)]


def set_strict_eigensolver(on):
    """process-wide: the fully converged stopping rule of the estimate chain's eigensolver (bcd_hip_set_strict_eigensolver)"""
    lib().bcd_hip_set_strict_eigensolver(1 if on else 0)


def set_fused_prepare_solve(on):
    """process-wide: the prepare and eigensolver phases of a full estimate as one kernel (default) or as two (bcd_hip_set_fused_prepare_solve)"""
    lib().bcd_hip_set_fused_prepare_solve(1 if on else 0)


def rccl_info():
    """{"native": what libbcd_hip.so's band driver is linked against at run time, "mapped": every librccl copy mapped into this process}"""
    buf = C.create_string_buffer(512)
    lib().bcd_hip_multi_rccl_info(buf, 512)
    mapped = []
    try:
        for ln in open("/proc/self/maps"):
            f = ln.split()
            if len(f) >= 6 and "librccl" in f[5] and f[5] not in mapped:
                mapped.append(f[5])
    except OSError:
        pass
    native = buf.value.decode()
    path = native.split(" from ", 1)[1] if " from " in native else "?"
    return {"native": native, "mapped": mapped, "one_copy": len(mapped) <= 1, "native_is_mapped": os.path.realpath(path) in [os.path.realpath(m) for m in mapped]}


def multi_unique_ids(n):
    """n RCCL unique ids (bytes), to be created by rank 0 and handed to every process (bcd_hip_multi_create_rank)"""
    out = b""
    for _ in range(n):
        buf = C.create_string_buffer(MULTI_ID_BYTES)
        rc = lib().bcd_hip_multi_unique_id(buf)
        if rc != 0:
            raise BcdHipError("bcd_hip_multi_unique_id rc=%d" % rc)
        out += buf.raw
    return out


class RankDenoiser:
    """one rank of the row-band partition in a one-process-per-GPU job (bcd_hip_multi_rank_*): the band's inputs and result stay in HBM"""

    def __init__(self, rank, world, device, ids):
        h = _VP()
        rc = lib().bcd_hip_multi_create_rank(C.byref(h), rank, world, device, ids, len(ids) // MULTI_ID_BYTES if ids else 0)
        if rc != 0:
            raise BcdHipError("bcd_hip_multi_create_rank failed: rc=%d" % rc)
        self.h, self.rank, self.world = h, rank, world

    def _chk(self, rc):
        if rc != 0:
            raise BcdHipError("rc=%d: %s" % (rc, lib().bcd_hip_multi_last_error(self.h).decode()))

    def configure(self, W, H, D, nscales, prm):
        """-> (first input line, input lines, first owned line, owned lines) of this rank's band"""
        v = [C.c_int(0) for _ in range(4)]
        self._chk(lib().bcd_hip_multi_rank_configure(self.h, W, H, D, nscales, C.byref(prm), *[C.byref(x) for x in v]))
        self.W, self.owned = W, (v[2].value, v[3].value)
        return tuple(x.value for x in v)

    def upload(self, col, ns, hist, cov):
        self._chk(lib().bcd_hip_multi_rank_upload(self.h, _fptr(col), _fptr(ns), _fptr(hist), _fptr(cov)))

    def step(self):
        self._chk(lib().bcd_hip_multi_rank_step(self.h))

    def set_loopback(self, on=True):
        """one rank of one, exchanging with itself over real RCCL communicators (one-GPU test of the transport code)"""
        self._chk(lib().bcd_hip_multi_set_loopback(self.h, 1 if on else 0))

    def renew_ids(self, ids):
        self._chk(lib().bcd_hip_multi_rank_renew_ids(self.h, ids, len(ids) // MULTI_ID_BYTES))

    def stats(self):
        s = MultiStats()
        lib().bcd_hip_multi_get_stats(self.h, C.byref(s))
        return s

    def set_comm_trace(self, on):
        lib().bcd_hip_multi_set_comm_trace(self.h, 1 if on else 0)

    def comm_trace(self):
        n = lib().bcd_hip_multi_get_comm_trace(self.h, self.rank, None, 0)
        buf = (C.c_int64 * max(1, n))()
        n = lib().bcd_hip_multi_get_comm_trace(self.h, self.rank, buf, n)
        v = list(buf[:n])
        return [tuple(v[i:i + 4]) for i in range(0, n, 4)]

    def download(self):
        import numpy as np
        out = np.empty((self.owned[1], self.W, 3), np.float32)
        self._chk(lib().bcd_hip_multi_rank_download(self.h, _fptr(out)))
        return out

    def close(self):
        if self.h:
            lib().bcd_hip_multi_destroy(self.h)
            self.h = None


def selftest_transport(device=0, halo_bytes=7 * 3840 * 16):
    """bcd_hip_multi_selftest_transport: (rc, report line)"""
    buf = C.create_string_buffer(512)
    rc = lib().bcd_hip_multi_selftest_transport(int(device), int(halo_bytes), buf, 512)
    return rc, buf.value.decode()


def visit_order(W, H, w, random_order, seed):
    import numpy as np
    out = np.empty(((W - 2 * w) * (H - 2 * w),), np.int32)
    rc = lib().bcd_hip_visit_order(W, H, w, int(random_order), seed, out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise BcdHipError("bcd_hip_visit_order rc=%d" % rc)
    return out


def scale_seed(seed0, scale):
    return lib().bcd_hip_scale_seed(seed0, int(scale))


def strip_order_seed(W, H, w, b):
    """the `seed` argument of visit_order / the marking entry points for pixel order 2 (the reference's multi-thread -r 0 list: even
    strips of 2b lines, then the odd ones): it carries the frame geometry"""
    return lib().bcd_hip_strip_order_seed(int(W), int(H), int(w), int(b))
