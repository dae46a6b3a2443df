"""ctypes binding of the plain-C exports of libbcdcore.so (bcd_amd/host/capi.cpp): synthetic scenes, the
SamplesAccumulator, and the C++ bcd::Denoiser / bcd::MultiscaleDenoiser classes.  Plumbing for bench.py and tests."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libbcdcore.so")
_F = C.POINTER(C.c_float)
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libbcdcore.so is not built (%s): run `python -m bcd_amd.build`" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
    return _lib


def _fp(a):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_F)


def synthetic_scene(W, H, spp=32, seed=1234, sigma=0.35, spike_prob=0.01, first_line=0, nb_lines=None, pattern=0):
    """(colors, nsamples, histograms, covariances) of lines [first_line, first_line+nb_lines) of a W x H frame;
    pattern 0 = ramps + 16-pixel checker (SURVEY 8d probe scene), 1 = band-limited texture with oblique soft edges"""
    n = H - first_line if nb_lines is None else nb_lines
    ns = np.empty((n, W, 1), np.float32)
    mean = np.empty((n, W, 3), np.float32)
    cov = np.empty((n, W, 6), np.float32)
    hist = np.empty((n, W, 60), np.float32)
    rc = lib().bcdcore_synthetic_scene_ex(W, H, spp, C.c_uint(seed), C.c_float(sigma), C.c_float(spike_prob), int(pattern), first_line, n,
                                          _fp(ns), _fp(mean), _fp(cov), _fp(hist))
    if rc != 0:
        raise ValueError("bcdcore_synthetic_scene rc=%d" % rc)
    return mean, ns, hist, cov


def accumulate(samples, W, H, nbins=20, gamma=2.2, maxval=2.5):
    samples = np.ascontiguousarray(samples, np.float32)
    ns = np.empty((H, W, 1), np.float32)
    mean = np.empty((H, W, 3), np.float32)
    cov = np.empty((H, W, 6), np.float32)
    hist = np.empty((H, W, 3 * nbins), np.float32)
    lib().bcdcore_accumulate(_fp(samples), C.c_longlong(samples.shape[0]), W, H, nbins, C.c_float(gamma), C.c_float(maxval),
                             _fp(ns), _fp(mean), _fp(cov), _fp(hist))
    return ns, mean, cov, hist


def device_accumulate(samples, W, H, nbins=20, gamma=2.2, maxval=2.5, device=0, snapshot_at=0):
    """the same stream through bcd::DeviceSamplesAccumulator::addSample (HBM running sums); snapshot_at > 0: a host snapshot after that many
    samples, then the accumulation goes on"""
    samples = np.ascontiguousarray(samples, np.float32)
    ns = np.empty((H, W, 1), np.float32)
    mean = np.empty((H, W, 3), np.float32)
    cov = np.empty((H, W, 6), np.float32)
    hist = np.empty((H, W, 3 * nbins), np.float32)
    rc = lib().bcdcore_device_accumulate(_fp(samples), C.c_longlong(samples.shape[0]), W, H, nbins, C.c_float(gamma), C.c_float(maxval), int(device),
                                         C.c_longlong(snapshot_at), _fp(ns), _fp(mean), _fp(cov), _fp(hist))
    if rc != 0:
        lib().bcdcore_device_accumulate_error.restype = C.c_char_p
        raise RuntimeError("DeviceSamplesAccumulator: " + lib().bcdcore_device_accumulate_error().decode())
    return ns, mean, cov, hist


def device_splat(calls, W, H, radius, table, nbins=20, gamma=2.2, maxval=2.5, device=0):
    """a stream of mixed calls through bcd::DeviceSamplesAccumulator with a reconstruction filter set: calls (n, 7) float32, each
    (kind, a, b, r, g, b, w); kind 0: addSample(line = a, col = b, ...), kind 1: splatSample(x = a, y = b, ...).  radius: (radius_x, radius_y);
    table: square float32.  -> ((ns, mean, cov, hist), (samples accumulated, dropped))"""
    calls = np.ascontiguousarray(calls, np.float32)
    table = np.ascontiguousarray(table, np.float32)
    assert calls.ndim == 2 and calls.shape[1] == 7 and table.ndim == 2 and table.shape[0] == table.shape[1]
    ns = np.empty((H, W, 1), np.float32)
    mean = np.empty((H, W, 3), np.float32)
    cov = np.empty((H, W, 6), np.float32)
    hist = np.empty((H, W, 3 * nbins), np.float32)
    counts = (C.c_longlong * 2)()
    rc = lib().bcdcore_device_splat(_fp(calls), C.c_longlong(calls.shape[0]), W, H, nbins, C.c_float(gamma), C.c_float(maxval), int(device),
                                    C.c_float(radius[0]), C.c_float(radius[1]), int(table.shape[0]), _fp(table), _fp(ns), _fp(mean), _fp(cov),
                                    _fp(hist), counts)
    if rc != 0:
        lib().bcdcore_device_accumulate_error.restype = C.c_char_p
        raise RuntimeError("DeviceSamplesAccumulator: " + lib().bcdcore_device_accumulate_error().decode())
    return (ns, mean, cov, hist), (counts[0], counts[1])


def device_accumulate_layers(calls, layer_rgb, W, H, radius=None, table=None, batch=0, snapshot_at=0, state_path=None, layers_path=None, nbins=20,
                             gamma=2.2, maxval=2.5, device=0):
    """mixed calls through the batch forms of a bcd::DeviceSamplesAccumulator with colour layers: calls (n, 7) float32 as for device_splat,
    layer_rgb (L, n, 3) the layers' colours of the same calls; runs of one kind go through addSamples / splatSamples in pieces of at most
    `batch` calls; snapshot_at > 0: host snapshots before that call; state_path and layers_path: saveState + saveLayers at the end, loaded
    into a second accumulator whose statistics are returned.
    -> ((ns, mean, cov, hist), [(mean, cov) per layer], (samples accumulated, dropped))"""
    calls = np.ascontiguousarray(calls, np.float32)
    layer_rgb = np.ascontiguousarray(layer_rgb, np.float32)
    n, L = calls.shape[0], layer_rgb.shape[0]
    assert calls.ndim == 2 and calls.shape[1] == 7 and layer_rgb.shape == (L, n, 3)
    if table is not None:
        table = np.ascontiguousarray(table, np.float32)
        assert table.ndim == 2 and table.shape[0] == table.shape[1]
    ns = np.empty((H, W, 1), np.float32)
    mean = np.empty((H, W, 3), np.float32)
    cov = np.empty((H, W, 6), np.float32)
    hist = np.empty((H, W, 3 * nbins), np.float32)
    lmean = np.empty((L, H, W, 3), np.float32)
    lcov = np.empty((L, H, W, 6), np.float32)
    counts = (C.c_longlong * 2)()
    rx, ry = radius if radius is not None else (0.0, 0.0)
    path = lambda p: None if p is None else os.fsencode(str(p))
    rc = lib().bcdcore_device_accumulate_layers(_fp(calls), C.c_longlong(n), _fp(layer_rgb), int(L), W, H, nbins, C.c_float(gamma), C.c_float(maxval),
                                                int(device), C.c_float(rx), C.c_float(ry), int(table.shape[0]) if table is not None else 0,
                                                _fp(table) if table is not None else None, C.c_longlong(batch), C.c_longlong(snapshot_at),
                                                C.c_char_p(path(state_path)), C.c_char_p(path(layers_path)), _fp(ns), _fp(mean), _fp(cov), _fp(hist),
                                                _fp(lmean), _fp(lcov), counts)
    if rc != 0:
        lib().bcdcore_device_accumulate_error.restype = C.c_char_p
        raise RuntimeError("DeviceSamplesAccumulator: " + lib().bcdcore_device_accumulate_error().decode())
    return (ns, mean, cov, hist), [(lmean[k], lcov[k]) for k in range(L)], (counts[0], counts[1])


def device_accumulate_features(calls, features, W, H, layer_rgb=None, radius=None, table=None, batch=0, state_path=None, layers_path=None,
                               features_path=None, merge_again=False, nbins=20, gamma=2.2, maxval=2.5, device=0):
    """mixed calls through the batch forms of a bcd::DeviceSamplesAccumulator with feature channels: calls (n, 7) float32 as for device_splat,
    features (n, F) the feature channels of the same calls, layer_rgb (L, n, 3) or None (no layers); runs of one kind go through addSamples /
    splatSamples in pieces of at most `batch` calls; state_path, features_path (and layers_path with layers): saveState + saveFeatures
    (+ saveLayers) at the end, loaded into a second accumulator whose statistics are returned; merge_again: the files are then merged into
    it once more.  -> ((ns, mean, cov, hist), [(mean, cov) per layer], (feature means, variances of the means), (samples accumulated, dropped))"""
    calls = np.ascontiguousarray(calls, np.float32)
    features = np.ascontiguousarray(features, np.float32)
    n, F = calls.shape[0], features.shape[1]
    L = 0 if layer_rgb is None else layer_rgb.shape[0]
    layer_rgb = np.ascontiguousarray(layer_rgb if L else np.zeros((1, 1, 3)), np.float32)
    assert calls.ndim == 2 and calls.shape[1] == 7 and features.shape == (n, F) and (L == 0 or layer_rgb.shape == (L, n, 3))
    if table is not None:
        table = np.ascontiguousarray(table, np.float32)
        assert table.ndim == 2 and table.shape[0] == table.shape[1]
    mk = lambda *shape: np.empty(shape, np.float32)
    ns, mean, cov, hist = mk(H, W, 1), mk(H, W, 3), mk(H, W, 6), mk(H, W, 3 * nbins)
    lmean, lcov = mk(max(L, 1), H, W, 3), mk(max(L, 1), H, W, 6)
    fmean, fvar = mk(H, W, max(F, 1)), mk(H, W, max(F, 1))
    counts = (C.c_longlong * 2)()
    rx, ry = radius if radius is not None else (0.0, 0.0)
    path = lambda p: None if p is None else os.fsencode(str(p))
    rc = lib().bcdcore_device_accumulate_features(_fp(calls), C.c_longlong(n), _fp(layer_rgb), int(L), _fp(features), int(F), W, H, nbins, C.c_float(gamma),
                                                  C.c_float(maxval), int(device), C.c_float(rx), C.c_float(ry),
                                                  int(table.shape[0]) if table is not None else 0, _fp(table) if table is not None else None,
                                                  C.c_longlong(batch), C.c_char_p(path(state_path)), C.c_char_p(path(layers_path)),
                                                  C.c_char_p(path(features_path)), int(bool(merge_again)), _fp(ns), _fp(mean), _fp(cov), _fp(hist),
                                                  _fp(lmean), _fp(lcov), _fp(fmean), _fp(fvar), counts)
    if rc != 0:
        lib().bcdcore_device_accumulate_error.restype = C.c_char_p
        raise RuntimeError("DeviceSamplesAccumulator: " + lib().bcdcore_device_accumulate_error().decode())
    return (ns, mean, cov, hist), [(lmean[k], lcov[k]) for k in range(L)], (fmean, fvar), (counts[0], counts[1])


def device_features_refusals(nb_layers, nb_features, device=0):
    """what a bcd::DeviceSamplesAccumulator with these counts answers, with or without a device: -> (isValid() after the constructor, the
    messages of lastError() after the constructor, addSample, splatSample, addSamples without features, addSamples and splatSamples with
    null features; a seventh line if a refused add was applied)"""
    buf = C.create_string_buffer(4096)
    valid = lib().bcdcore_device_features_refusals(int(nb_layers), int(nb_features), int(device), buf, len(buf))
    return bool(valid), buf.value.decode().split("\n")[:-1]


def device_plan(samples, W, H, budget, offset=0, threshold=0.0, eps=1e-3, min_samples=2.0, max_per_pixel=16, nbins=20, gamma=2.2, maxval=2.5,
                device=0, invalid_first=False):
    """the stream through bcd::DeviceSamplesAccumulator::addSample (left in its host buffer), then planSamples -> (pixel list, summary dict);
    invalid_first: two planSamples calls with invalid arguments come first and must fail"""
    samples = np.ascontiguousarray(samples, np.float32)
    pixels = np.empty(max(int(budget), 1), np.int32)
    summary = np.zeros(4, np.float64)
    L = lib()
    L.bcdcore_device_plan.restype = C.c_longlong
    T = L.bcdcore_device_plan(_fp(samples), C.c_longlong(samples.shape[0]), W, H, nbins, C.c_float(gamma), C.c_float(maxval), int(device),
                              C.c_longlong(budget), C.c_ulonglong(offset), C.c_float(threshold), C.c_float(eps), C.c_float(min_samples),
                              int(max_per_pixel), int(bool(invalid_first)), pixels.ctypes.data_as(C.POINTER(C.c_int)),
                              summary.ctypes.data_as(C.POINTER(C.c_double)))
    if T == -2:
        raise RuntimeError("DeviceSamplesAccumulator::planSamples accepted invalid arguments")
    if T < 0:
        L.bcdcore_device_accumulate_error.restype = C.c_char_p
        raise RuntimeError("DeviceSamplesAccumulator: " + L.bcdcore_device_accumulate_error().decode())
    return pixels[:T].copy(), {"planned": int(summary[0]), "active": int(summary[1]), "unsampled": int(summary[2]),
                               "max_error": float(np.float32(summary[3]))}


class DeviceAccumulator:
    """a bcd::DeviceSamplesAccumulator kept alive between calls (capi.cpp bcdcore_device_acc_*), for its state methods: exportState,
    saveState, loadState, mergeState and merge.  Failing methods raise RuntimeError with the class's lastError()"""

    def __init__(self, W, H, nbins=20, gamma=2.2, maxval=2.5, device=0):
        L = lib()
        L.bcdcore_device_acc_create.restype = C.c_void_p
        L.bcdcore_device_acc_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int]
        L.bcdcore_device_acc_destroy.argtypes = [C.c_void_p]
        L.bcdcore_device_acc_destroy.restype = None
        L.bcdcore_device_acc_error.argtypes = [C.c_void_p]
        L.bcdcore_device_acc_error.restype = C.c_char_p
        L.bcdcore_device_acc_valid.argtypes = [C.c_void_p]
        L.bcdcore_device_acc_add.argtypes = [C.c_void_p, _F, C.c_longlong]
        L.bcdcore_device_acc_add.restype = None
        L.bcdcore_device_acc_export.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong]
        L.bcdcore_device_acc_export.restype = C.c_longlong
        for name in ("save", "load", "merge_state"):
            getattr(L, "bcdcore_device_acc_" + name).argtypes = [C.c_void_p, C.c_char_p]
        L.bcdcore_device_acc_merge.argtypes = [C.c_void_p, C.c_void_p]
        L.bcdcore_device_acc_statistics.argtypes = [C.c_void_p, _F, _F, _F, _F, C.POINTER(C.c_longlong)]
        self.W, self.H, self.nbins = W, H, nbins
        self.h = L.bcdcore_device_acc_create(W, H, nbins, gamma, maxval, int(device))
        if not L.bcdcore_device_acc_valid(self.h):
            msg = L.bcdcore_device_acc_error(self.h).decode()
            self.close()
            raise RuntimeError("DeviceSamplesAccumulator: " + msg)

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError("DeviceSamplesAccumulator: " + lib().bcdcore_device_acc_error(self.h).decode())

    def add(self, samples):
        """(n, 6) stream (line, col, r, g, b, w) through addSample"""
        samples = np.ascontiguousarray(samples, np.float32)
        lib().bcdcore_device_acc_add(self.h, _fp(samples), samples.shape[0])

    def export_state(self):
        n = lib().bcdcore_device_acc_export(self.h, None, 0)
        self._chk(0 if n >= 0 else -1)
        out = np.empty(n, np.uint8)
        self._chk(0 if lib().bcdcore_device_acc_export(self.h, out.ctypes.data_as(C.c_void_p), n) == n else -1)
        return out

    def save_state(self, path):
        self._chk(lib().bcdcore_device_acc_save(self.h, os.fsencode(path)))

    def load_state(self, path):
        self._chk(lib().bcdcore_device_acc_load(self.h, os.fsencode(path)))

    def merge_state(self, path):
        self._chk(lib().bcdcore_device_acc_merge_state(self.h, os.fsencode(path)))

    def merge(self, other):
        self._chk(lib().bcdcore_device_acc_merge(self.h, other.h))

    def statistics(self):
        """host snapshot (ns, mean, cov, hist) and (samples accumulated, dropped)"""
        H, W = self.H, self.W
        ns, mean, cov = np.empty((H, W, 1), np.float32), np.empty((H, W, 3), np.float32), np.empty((H, W, 6), np.float32)
        hist = np.empty((H, W, 3 * self.nbins), np.float32)
        counts = (C.c_longlong * 2)()
        self._chk(lib().bcdcore_device_acc_statistics(self.h, _fp(ns), _fp(mean), _fp(cov), _fp(hist), counts))
        return (ns, mean, cov, hist), (counts[0], counts[1])

    def close(self):
        if self.h:
            lib().bcdcore_device_acc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def denoise(col, ns, hist, cov, nscales=1, tau=1.0, w=1, b=6, min_eig=1e-8, random_order=True, m=1.0, seed=1234, hist_width_override=0,
            use_cuda=True, devices=None, prefilter_factor=0.0):
    """bcd::Denoiser / bcd::MultiscaleDenoiser via IDenoiser; returns (ok, out, progress_monotone).
    use_cuda -> DenoiserParameters::m_useCuda, devices -> setDevices, prefilter_factor -> setSpikePrefilter"""
    H, W, D = hist.shape
    out = np.zeros((H, W, 3), np.float32)
    p = lambda a: None if a is None else _fp(a)
    devs = (C.c_int * len(devices))(*devices) if devices else None
    rc = lib().bcdcore_denoise_ex(p(col), p(ns), p(hist), p(cov), W, H, D, nscales, C.c_float(tau), w, b, C.c_float(min_eig),
                                  1 if random_order else 0, C.c_float(m), C.c_uint(seed), _fp(out), int(hist_width_override),
                                  1 if use_cuda else 0, devs, len(devices) if devices else 0, C.c_float(prefilter_factor))
    return rc != 0, out, rc == 1


def denoise_layers(layers, ns, hist, nscales=1, tau=1.0, b=6, min_eig=1e-8, random_order=True, m=1.0, seed=1234, zero_bad=False,
                   prefilter_factor=0.0, size_mismatch_layer=0, after_clear=False, prefilter_layers=False):
    """bcd::Denoiser / bcd::MultiscaleDenoiser with colour layers: layers[0] = (colours, covariances) goes through DenoiserInputs, the others through
    addLayer.  Returns (ok, [output per layer]).  size_mismatch_layer > 0: that added layer gets a covariance image of the wrong size;
    after_clear: clearLayers() and a second denoise() follow, whose result replaces the first output; prefilter_layers -> setSpikePrefilterLayers: the
    prefilter (prefilter_factor > 0) is accepted beside added layers and covers every layer"""
    H, W, D = hist.shape
    L = len(layers)
    cols = np.ascontiguousarray(np.stack([c for c, _ in layers]), np.float32)
    covs = np.ascontiguousarray(np.stack([v for _, v in layers]), np.float32)
    outs = np.zeros((L, H, W, 3), np.float32)
    rc = lib().bcdcore_denoise_layers_ex(_fp(cols), _fp(covs), _fp(ns), _fp(hist), W, H, D, nscales, L, C.c_float(tau), b, C.c_float(min_eig),
                                         1 if random_order else 0, C.c_float(m), C.c_uint(seed), 1 if zero_bad else 0, C.c_float(prefilter_factor),
                                         int(size_mismatch_layer), 1 if after_clear else 0, 1 if prefilter_layers else 0, _fp(outs))
    return rc != 0, [outs[k] for k in range(L)]


def _motion_stack(motions, F, H, W):
    """(fields (max(F, 1), H, W, 2) float32, flags int32[max(F, 1)]) of a list of F motion fields or None entries"""
    motions = list(motions)
    if len(motions) != F:
        raise ValueError("one motion field (or None) per neighbour expected (%d, not %d)" % (F, len(motions)))
    fields = np.zeros((max(F, 1), H, W, 2), np.float32)
    flags = (C.c_int * max(F, 1))()
    for k, mv in enumerate(motions):
        if mv is not None:
            fields[k] = np.asarray(mv, np.float32).reshape(H, W, 2)
            flags[k] = 1
    return fields, flags


def _takes_prefilter_frames(fn):
    """adds two keywords to a wrapper of a call with neighbour frames or of a sequence.  prefilter_frames=<factor>: > 0 sets setSpikePrefilter(factor) and
    setSpikePrefilterFrames(true) on the denoiser the call builds -- every frame passes through the spike prefilter on its own
    (bcd_hip_denoise_temporal_host_ex, bcd_hip_sequence_set_prefilter); 0 (the default): the call as it always was.  prefilter_without_switch=<factor> (for
    tests of the refusals): setSpikePrefilter(factor) alone, which denoise() must refuse beside neighbour frames and in a sequence"""
    import functools

    @functools.wraps(fn)
    def call(*args, prefilter_frames=0.0, prefilter_without_switch=0.0, **kw):
        if prefilter_frames < 0 or prefilter_without_switch < 0 or (prefilter_frames and prefilter_without_switch):
            raise ValueError("prefilter_frames and prefilter_without_switch are factors >= 0, and one of them at most is given")
        if not prefilter_frames and not prefilter_without_switch:
            return fn(*args, **kw)
        lib().bcdcore_set_frame_prefilter(C.c_float(prefilter_frames or prefilter_without_switch), 1 if prefilter_frames else 0)
        try:
            return fn(*args, **kw)
        finally:
            lib().bcdcore_set_frame_prefilter(C.c_float(0.0), 0)
    return call


@_takes_prefilter_frames
def denoise_temporal(col, ns, hist, cov, neighbours, nscales=1, tau=1.0, b=6, min_eig=1e-8, random_order=True, m=1.0, seed=1234, after_clear=False, motions=None,
                     features=None, neighbour_features=None, **guide):
    """bcd::Denoiser / bcd::MultiscaleDenoiser with neighbouring frames of the sequence (addNeighbourFrame): neighbours is a list of (col, ns, hist, cov)
    arrays of the frame's size, at most four.  after_clear: clearNeighbourFrames() and a second denoise() follow, whose result replaces the first.
    motions: None, or per neighbour an (H, W, 2) motion field or None (setNeighbourMotion).  features / neighbour_features (and variances, neighbour_variances,
    floors, threshold): the feature buffers of denoise_temporal_layers, which then serves the call with one layer.  Returns (ok, denoised frame)"""
    if features is not None or neighbour_features is not None:
        ok, outs = denoise_temporal_layers(ns, hist, [(col, cov)], [(f[1], f[2], [(f[0], f[3])]) for f in neighbours], nscales, tau, b, min_eig, random_order, m, seed,
                                           after_clear=after_clear, motions=motions, features=features, neighbour_features=neighbour_features, **guide)
        return ok, outs[0]
    H, W, D = hist.shape
    F = len(neighbours)
    stack = lambda k, d: np.ascontiguousarray(np.stack([np.asarray(f[k], np.float32).reshape(H, W, d) for f in neighbours]) if F else np.zeros((1, H, W, d)), np.float32)
    out = np.zeros((H, W, 3), np.float32)
    if motions is not None:
        fields, flags = _motion_stack(motions, F, H, W)
        rc = lib().bcdcore_denoise_temporal_motion(_fp(col), _fp(ns), _fp(hist), _fp(cov), _fp(stack(0, 3)), _fp(stack(1, 1)), _fp(stack(2, D)), _fp(stack(3, 6)), F,
                                                   _fp(fields), flags, W, H, D, int(nscales), C.c_float(tau), b, C.c_float(min_eig), 1 if random_order else 0,
                                                   C.c_float(m), C.c_uint(seed), 1 if after_clear else 0, _fp(out))
        return rc != 0, out
    rc = lib().bcdcore_denoise_temporal(_fp(col), _fp(ns), _fp(hist), _fp(cov), _fp(stack(0, 3)), _fp(stack(1, 1)), _fp(stack(2, D)), _fp(stack(3, 6)), F, W, H, D,
                                        int(nscales), C.c_float(tau), b, C.c_float(min_eig), 1 if random_order else 0, C.c_float(m), C.c_uint(seed),
                                        1 if after_clear else 0, _fp(out))
    return rc != 0, out


@_takes_prefilter_frames
def denoise_sequence(frames, radius=1, nscales=1, tau=1.0, w=1, b=6, min_eig=1e-8, random_order=True, m=1.0, seed=1234, unsupported=0, layers=None, features=None,
                     feature_variances=None, feature_floors=(), feature_threshold=1.0, var_floor=1e-8, break_settings=0, motions=None, break_motion=0):
    """bcd::SequenceDenoiser: frames is a list of (col, ns, hist, cov) arrays of one size, pushed one by one and popped as they become ready; frame t comes out
    denoised with the frames t - radius .. t + radius that exist (what denoise_temporal returns for it with those neighbours in ascending order), every
    frame uploaded once and every pair of frames searched once.  unsupported: bits of settings the sequence must refuse (bcdcore_denoise_sequence).
    Returns (ok, [denoised frame per frame]).
    With `layers` (per frame a list of further (colours, covariances) beside the frame's own, which are layer 0), a frame whose hist is None (every frame:
    the selection from means and covariances with `var_floor`) or `features` (per frame an (H, W, F) image; feature_variances the same or None, with
    feature_floors and feature_threshold) the class runs with setFrameSettings(true) and the result is (ok, [[layer 0, layer 1, ...] per frame]);
    break_settings: bits of settings that must be refused then (bcdcore_denoise_sequence_modes).
    motions: None, or per frame None or a (prev, next) pair -- the (H, W, 2) motion fields of that frame towards the frame before and after it, each an array or
    None (SequenceDenoiser::setFrameMotion; bcdcore_denoise_sequence_motion); break_motion: bits of what a field must be refused for (1: three channels, 2:
    another width).  The result has the shape it has without motions"""
    T = len(frames)
    modes = layers is not None or features is not None or frames[0][2] is None or break_settings
    if modes or motions is not None:
        H, W = np.asarray(frames[0][0]).shape[:2]
        hist = frames[0][2] is not None
        D = np.asarray(frames[0][2]).shape[2] if hist else 0
        lay = [[(f[0], f[3])] + list(layers[k] if layers is not None else []) for k, f in enumerate(frames)]
        L = len(lay[0])
        if any(len(x) != L for x in lay) or any((f[2] is not None) != hist for f in frames):
            raise ValueError("every frame brings the same layers, and histograms or none")
        as32 = lambda a, d: np.asarray(a, np.float32).reshape(H, W, d)
        cols = np.ascontiguousarray(np.stack([np.stack([as32(c, 3) for c, _ in x]) for x in lay]), np.float32)
        covs = np.ascontiguousarray(np.stack([np.stack([as32(v, 6) for _, v in x]) for x in lay]), np.float32)
        nss = np.ascontiguousarray(np.stack([as32(f[1], 1) for f in frames]), np.float32)
        hists = np.ascontiguousarray(np.stack([as32(f[2], D) for f in frames]), np.float32) if hist else None
        F = np.asarray(features[0]).shape[2] if features is not None else 0
        feats = np.ascontiguousarray(np.stack([as32(a, F) for a in features]), np.float32) if features is not None else None
        fvars = np.ascontiguousarray(np.stack([as32(a, F) for a in feature_variances]), np.float32) if feature_variances is not None else None
        floors = np.ascontiguousarray(feature_floors, np.float32)
        outs = np.zeros((T, L, H, W, 3), np.float32)
        opt = lambda a: None if a is None else _fp(a)
        args = (_fp(cols), _fp(nss), opt(hists), _fp(covs), opt(feats), opt(fvars), T, L, F, _fp(floors) if floors.size else None, int(floors.size),
                C.c_float(feature_threshold), C.c_float(var_floor), W, H, D, int(nscales), int(radius), C.c_float(tau), int(w), int(b), C.c_float(min_eig),
                1 if random_order else 0, C.c_float(m), C.c_uint(seed), int(break_settings), _fp(outs))
        if motions is None:
            rc = lib().bcdcore_denoise_sequence_modes(*args)
        else:
            motions = list(motions)
            if len(motions) != T:
                raise ValueError("one (prev, next) pair of motion fields (or None) per frame expected (%d, not %d)" % (T, len(motions)))
            fields = np.zeros((T, 2, H, W, 2), np.float32)
            flags = (C.c_int * (2 * T))()
            for k, pair in enumerate(motions):
                for d, mv in enumerate(pair if pair is not None else (None, None)):
                    if mv is not None:
                        fields[k, d] = as32(mv, 2)
                        flags[2 * k + d] = 1
            rc = lib().bcdcore_denoise_sequence_motion(*args, _fp(fields), flags, int(break_motion))
        return rc != 0, [[outs[k, j] for j in range(L)] for k in range(T)] if modes else [outs[k, 0] for k in range(T)]
    H, W, D = frames[0][2].shape
    stack = lambda k, d: np.ascontiguousarray(np.stack([np.asarray(f[k], np.float32).reshape(H, W, d) for f in frames]), np.float32)
    outs = np.zeros((T, H, W, 3), np.float32)
    rc = lib().bcdcore_denoise_sequence(_fp(stack(0, 3)), _fp(stack(1, 1)), _fp(stack(2, D)), _fp(stack(3, 6)), T, W, H, D, int(nscales), int(radius), C.c_float(tau),
                                        int(w), int(b), C.c_float(min_eig), 1 if random_order else 0, C.c_float(m), C.c_uint(seed), int(unsupported), _fp(outs))
    return rc != 0, [outs[k] for k in range(T)]


@_takes_prefilter_frames
def denoise_temporal_layers(ns, hist, layers, neighbours, nscales=1, tau=1.0, b=6, min_eig=1e-8, random_order=True, m=1.0, seed=1234, drop_layers=0, after_clear=False,
                            motions=None, features=None, neighbour_features=None, variances=None, neighbour_variances=None, floors=(), threshold=1.0,
                            neighbours_with_features=None, moment_selection=False, devices=None):
    """bcd::Denoiser / bcd::MultiscaleDenoiser with colour layers beside neighbouring frames (addLayer, addNeighbourFrame, addNeighbourFrameLayer): layers is a
    list of (colours, covariances), [0] going through DenoiserInputs; neighbours a list of (ns, hist, [(colours, covariances)]) with the same layers.
    drop_layers: the last neighbour is given that many layers fewer (denoise() must refuse).  after_clear: clearNeighbourFrames() and a second denoise()
    follow, whose results replace the first.  motions: None, or per neighbour an (H, W, 2) motion field or None (setNeighbourMotion).
    features (H, W, F) with floors and threshold (and variances): setGuideFeatures; neighbour_features, one (H, W, F') per neighbour (and neighbour_variances):
    setNeighbourGuideFeatures -- the call is then bcd_hip_denoise_temporal_guided_host.  neighbours_with_features: only that many neighbours get theirs;
    moment_selection, devices: setMomentSelection(true), setDevices (denoise() must refuse these).  Returns (ok, [output per layer])"""
    H, W, D = hist.shape
    L, F = len(layers), len(neighbours)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    cols, covs = f32(np.stack([c for c, _ in layers])), f32(np.stack([v for _, v in layers]))
    nb_cols = f32(np.stack([c for _, _, lay in neighbours for c, _ in lay])) if F else np.zeros((1, H, W, 3), np.float32)
    nb_covs = f32(np.stack([v for _, _, lay in neighbours for _, v in lay])) if F else np.zeros((1, H, W, 6), np.float32)
    nb_ns = f32(np.stack([np.asarray(n, np.float32).reshape(H, W, 1) for n, _, _ in neighbours])) if F else np.zeros((1, H, W, 1), np.float32)
    nb_hists = f32(np.stack([h for _, h, _ in neighbours])) if F else np.zeros((1, H, W, D), np.float32)
    outs = np.zeros((L, H, W, 3), np.float32)
    if features is not None or neighbour_features is not None:
        if features is None:
            raise ValueError("neighbour_features go with features: the gate covers the frame and every neighbour, or nothing")
        p = lambda a: None if a is None else _fp(a)
        feat, var = f32(features), None if variances is None else f32(variances)
        nfeat = f32(np.stack([f32(x) for x in neighbour_features])) if neighbour_features else None
        nvar = f32(np.stack([f32(x) for x in neighbour_variances])) if neighbour_variances else None
        fl = f32(np.asarray(floors, np.float32).reshape(-1))
        fields, flags = _motion_stack(motions, F, H, W) if motions is not None else (None, None)
        devs = (C.c_int * len(devices))(*devices) if devices else None
        given = (len(neighbour_features) if neighbour_features else 0) if neighbours_with_features is None else int(neighbours_with_features)
        rc = lib().bcdcore_denoise_temporal_guided(_fp(cols), _fp(covs), _fp(f32(ns)), _fp(f32(hist)), _fp(nb_cols), _fp(nb_covs), _fp(nb_ns), _fp(nb_hists), F, L, p(fields),
                                                   flags, W, H, D, int(nscales), C.c_float(tau), b, C.c_float(min_eig), 1 if random_order else 0, C.c_float(m), C.c_uint(seed),
                                                   1 if after_clear else 0, _fp(feat), p(var), feat.shape[2], _fp(fl) if fl.size else None, int(fl.size), C.c_float(threshold),
                                                   p(nfeat), p(nvar), nfeat.shape[3] if nfeat is not None else feat.shape[2], given, 1 if moment_selection else 0, devs,
                                                   len(devices) if devices else 0, _fp(outs))
        return rc != 0, [outs[k] for k in range(L)]
    if motions is not None:
        fields, flags = _motion_stack(motions, F, H, W)
        rc = lib().bcdcore_denoise_temporal_layers_motion(_fp(cols), _fp(covs), _fp(f32(ns)), _fp(f32(hist)), _fp(nb_cols), _fp(nb_covs), _fp(nb_ns), _fp(nb_hists), F, L,
                                                          _fp(fields), flags, W, H, D, int(nscales), C.c_float(tau), b, C.c_float(min_eig), 1 if random_order else 0,
                                                          C.c_float(m), C.c_uint(seed), int(drop_layers), 1 if after_clear else 0, _fp(outs))
        return rc != 0, [outs[k] for k in range(L)]
    rc = lib().bcdcore_denoise_temporal_layers(_fp(cols), _fp(covs), _fp(f32(ns)), _fp(f32(hist)), _fp(nb_cols), _fp(nb_covs), _fp(nb_ns), _fp(nb_hists), F, L, W, H, D,
                                               int(nscales), C.c_float(tau), b, C.c_float(min_eig), 1 if random_order else 0, C.c_float(m), C.c_uint(seed),
                                               int(drop_layers), 1 if after_clear else 0, _fp(outs))
    return rc != 0, [outs[k] for k in range(L)]


@_takes_prefilter_frames
def denoise_temporal_moments(ns, layers, neighbours, nscales=1, tau=1.0, b=6, min_eig=1e-8, random_order=True, m=1.0, seed=1234, var_floor=1e-8, motions=None,
                             features=None, neighbour_features=None, variances=None, neighbour_variances=None, floors=(), threshold=1.0, moment_selection=True,
                             plain_neighbours=0, drop_layers=0, devices=None):
    """bcd::Denoiser / bcd::MultiscaleDenoiser under setMomentSelection(true, var_floor) with neighbour frames added by addNeighbourFrameMoments: no histogram
    anywhere (bcd_hip_denoise_temporal_moments_host).  layers: a list of (colours, covariances), [0] the guide going through DenoiserInputs; neighbours: a list of
    (ns, [(colours, covariances)]) with the same layers; motions: None, or per neighbour an (H, W, 2) field or None; features (with neighbour_features, one per
    neighbour, floors, threshold and optional variances for every frame): the feature gate.  For the refusals denoise() owes: moment_selection=False leaves
    setMomentSelection off, the first plain_neighbours neighbours are added by addNeighbourFrame, the last neighbour gets drop_layers layers fewer, devices:
    setDevices.  Returns (ok, [output per layer])"""
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    p = lambda a: None if a is None else _fp(a)
    ns = f32(ns)
    H, W = ns.shape[0], ns.shape[1]
    L, F = len(layers), len(neighbours)
    cols, covs = f32(np.stack([c for c, _ in layers])), f32(np.stack([v for _, v in layers]))
    nb_cols = f32(np.stack([c for _, lay in neighbours for c, _ in lay])) if F else np.zeros((1, H, W, 3), np.float32)
    nb_covs = f32(np.stack([v for _, lay in neighbours for _, v in lay])) if F else np.zeros((1, H, W, 6), np.float32)
    nb_ns = f32(np.stack([np.asarray(n, np.float32).reshape(H, W, 1) for n, _ in neighbours])) if F else np.zeros((1, H, W, 1), np.float32)
    outs = np.zeros((L, H, W, 3), np.float32)
    fields, flags = _motion_stack(motions, F, H, W) if motions is not None else (None, None)
    feat = var = nfeat = nvar = None
    fl = f32(np.asarray(floors, np.float32).reshape(-1))
    if features is not None:
        feat, var = f32(features), None if variances is None else f32(variances)
        nfeat = f32(np.stack([f32(x) for x in neighbour_features])) if neighbour_features else None
        nvar = f32(np.stack([f32(x) for x in neighbour_variances])) if neighbour_variances else None
        if F and (nfeat is None or nfeat.shape != (F,) + feat.shape or (nvar is not None and nvar.shape != nfeat.shape)):
            raise ValueError("one feature image (and one variance image, or none at all) per neighbour expected, shaped like the frame's")
    devs = (C.c_int * len(devices))(*devices) if devices else None
    rc = lib().bcdcore_denoise_temporal_moments(_fp(cols), _fp(covs), _fp(ns), _fp(nb_cols), _fp(nb_covs), _fp(nb_ns), F, L, p(fields), flags, W, H, int(nscales),
                                                C.c_float(tau), b, C.c_float(min_eig), 1 if random_order else 0, C.c_float(m), C.c_uint(seed), C.c_float(var_floor), p(feat),
                                                p(var), feat.shape[2] if feat is not None else 0, _fp(fl) if fl.size else None, int(fl.size), C.c_float(threshold), p(nfeat),
                                                p(nvar), 1 if moment_selection else 0, int(plain_neighbours), int(drop_layers), devs, len(devices) if devices else 0, _fp(outs))
    return rc != 0, [outs[k] for k in range(L)]


def denoise_moments(layers, ns, nscales=1, tau=1.0, b=6, min_eig=1e-8, random_order=True, m=1.0, seed=1234, zero_bad=False, prefilter_factor=0.0,
                    prefilter_layers=False, var_floor=1e-8, devices=None):
    """bcd::Denoiser / bcd::MultiscaleDenoiser with setMomentSelection(true, var_floor): no histogram image; layers[0] = (colours, covariances) is the
    guide and goes through DenoiserInputs, the others through addLayer.  Returns (ok, [output per layer])"""
    H, W = ns.shape[0], ns.shape[1]
    L = len(layers)
    cols = np.ascontiguousarray(np.stack([c for c, _ in layers]), np.float32)
    covs = np.ascontiguousarray(np.stack([v for _, v in layers]), np.float32)
    outs = np.zeros((L, H, W, 3), np.float32)
    devs = (C.c_int * len(devices))(*devices) if devices else None
    rc = lib().bcdcore_denoise_moments(_fp(cols), _fp(covs), _fp(np.ascontiguousarray(ns, np.float32)), W, H, nscales, L, C.c_float(tau), b, C.c_float(min_eig),
                                       1 if random_order else 0, C.c_float(m), C.c_uint(seed), 1 if zero_bad else 0, C.c_float(prefilter_factor),
                                       1 if prefilter_layers else 0, C.c_float(var_floor), devs, len(devices) if devices else 0, _fp(outs))
    return rc != 0, [outs[k] for k in range(L)]


def denoise_guided(layers, ns, hist, features, variances=None, floors=(), threshold=1.0, nscales=1, tau=1.0, b=6, min_eig=1e-8, random_order=True, m=1.0, seed=1234,
                   zero_bad=False, prefilter_factor=0.0, prefilter_layers=False, var_floor=1e-8, devices=None, feature_width_override=0):
    """bcd::Denoiser / bcd::MultiscaleDenoiser with setGuideFeatures(features, variances, floors, threshold): layers[0] = (colours, covariances) goes through
    DenoiserInputs, the others through addLayer; hist None: setMomentSelection(true, var_floor) and no histogram image; features None: a null features pointer
    (the gate is off); feature_width_override > 0: the feature image is given that width.  Returns (ok, [output per layer])"""
    H, W = ns.shape[0], ns.shape[1]
    D = hist.shape[2] if hist is not None else 0
    L = len(layers)
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    p = lambda a: None if a is None else _fp(a)
    cols = np.ascontiguousarray(np.stack([c for c, _ in layers]), np.float32)
    covs = np.ascontiguousarray(np.stack([v for _, v in layers]), np.float32)
    ns, hist, features, variances = f32(ns), f32(hist), f32(features), f32(variances)
    fl = np.ascontiguousarray(np.asarray(floors, np.float32).reshape(-1))
    outs = np.zeros((L, H, W, 3), np.float32)
    devs = (C.c_int * len(devices))(*devices) if devices else None
    rc = lib().bcdcore_denoise_guided(_fp(cols), _fp(covs), _fp(ns), p(hist), W, H, D, nscales, L, C.c_float(tau), b, C.c_float(min_eig), 1 if random_order else 0,
                                      C.c_float(m), C.c_uint(seed), 1 if zero_bad else 0, C.c_float(prefilter_factor), 1 if prefilter_layers else 0,
                                      C.c_float(var_floor), p(features), p(variances), features.shape[2] if features is not None else 0, variances.shape[2] if variances is not None else 0,
                                      _fp(fl) if fl.size else None, int(fl.size), C.c_float(threshold), int(feature_width_override), devs, len(devices) if devices else 0, _fp(outs))
    return rc != 0, [outs[k] for k in range(L)]


def denoise_reuse(col, ns, hist, cov, nscales=3, b=6, nb_of_cores=0):
    """one IDenoiser object, denoise() twice with -r 0: (ok, first output, second output, (m_nbOfCores after call 1, after call 2))"""
    H, W, D = hist.shape
    o1, o2 = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
    after = (C.c_int * 2)()
    rc = lib().bcdcore_denoise_reuse(_fp(col), _fp(ns), _fp(hist), _fp(cov), W, H, D, nscales, b, nb_of_cores, _fp(o1), _fp(o2), after)
    return rc != 0, o1, o2, (after[0], after[1])


def last_nb_of_cores():
    """DenoiserParameters::m_nbOfCores after the last denoise() (the reference writes the actual thread count back)"""
    return lib().bcdcore_last_nb_of_cores()


def release_engines():
    """bcd::releaseEngines(): destroy the cached engine contexts (device workspaces) of libbcdcore"""
    lib().bcdcore_release_engines()


def accumulate_threadsafe(samples, W, H, threads=4, nbins=20, gamma=2.2, maxval=2.5):
    """SamplesAccumulatorThreadSafe::addSampleThreadSafely from `threads` OpenMP threads"""
    samples = np.ascontiguousarray(samples, np.float32)
    ns = np.empty((H, W, 1), np.float32)
    mean = np.empty((H, W, 3), np.float32)
    cov = np.empty((H, W, 6), np.float32)
    hist = np.empty((H, W, 3 * nbins), np.float32)
    lib().bcdcore_accumulate_threadsafe(_fp(samples), C.c_longlong(samples.shape[0]), W, H, nbins, C.c_float(gamma), C.c_float(maxval), threads,
                                        _fp(ns), _fp(mean), _fp(cov), _fp(hist))
    return ns, mean, cov, hist


def spike_filter(col, ns, hist, cov, factor=2.0):
    H, W, D = hist.shape
    c, n, h, v = col.copy(), ns.copy(), hist.copy(), cov.copy()
    lib().bcdcore_spike_filter(_fp(c), _fp(n), _fp(h), _fp(v), W, H, D, C.c_float(factor))
    return c, n, h, v


def spike_filter_host(col, ns, hist, cov, factor=2.0):
    """SpikeRemovalFilter::filterOnHost (the loops filter() runs when no HIP device is usable)"""
    H, W, D = hist.shape
    c, n, h, v = col.copy(), ns.copy(), hist.copy(), cov.copy()
    lib().bcdcore_spike_filter_host(_fp(c), _fp(n), _fp(h), _fp(v), W, H, D, C.c_float(factor))
    return c, n, h, v


def merge_hist_ns(hist, ns):
    H, W, D = hist.shape
    out = np.empty((H, W, D + 1), np.float32)
    lib().bcdcore_merge_hist_ns(_fp(hist), _fp(ns), W, H, D, _fp(out))
    return out


def split_hist_ns(merged):
    H, W, D1 = merged.shape
    hist = np.empty((H, W, D1 - 1), np.float32)
    ns = np.empty((H, W, 1), np.float32)
    rc = lib().bcdcore_split_hist_ns(_fp(merged), W, H, D1, _fp(hist), _fp(ns))
    return (hist, ns) if rc == 0 else None


def write_exr(path, img, multi_channels):
    H, W, D = img.shape
    rc = lib().bcdcore_write_exr(path.encode(), _fp(np.ascontiguousarray(img, np.float32)), W, H, D, 1 if multi_channels else 0)
    if rc != 0:
        lib().bcdcore_exr_last_error.restype = C.c_char_p
        raise IOError(lib().bcdcore_exr_last_error().decode())


def read_exr(path, multi_channels):
    W, H, D = C.c_int(), C.c_int(), C.c_int()
    lib().bcdcore_exr_last_error.restype = C.c_char_p
    if lib().bcdcore_read_exr(path.encode(), 1 if multi_channels else 0, C.byref(W), C.byref(H), C.byref(D), None, C.c_longlong(0)) != 0:
        raise IOError(lib().bcdcore_exr_last_error().decode())
    out = np.empty((H.value, W.value, D.value), np.float32)
    rc = lib().bcdcore_read_exr(path.encode(), 1 if multi_channels else 0, C.byref(W), C.byref(H), C.byref(D), _fp(out), C.c_longlong(out.size))
    if rc != 0:
        raise IOError("read_exr rc=%d" % rc)
    return out
