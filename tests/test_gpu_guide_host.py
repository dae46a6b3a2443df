"""GPU tests of the feature gate through the host library: bcd_cli --features and Denoiser / MultiscaleDenoiser::setGuideFeatures give what the
Python resident call (Context.denoise_guided) gives on the same numbers.  "The same" between two runs of the same build: 1e-5 relative L-inf (TOL_SAME).
bcd_cli writes its colours in half precision, so its file is compared with that bar plus the rounding of the file format: a value x within
TOL_SAME * max of the resident result w lands, after rounding to binary16, within 2^-11 |x| (normal range; 2^-25 absolute below 2^-14) of itself."""
import os
import subprocess

import numpy as np
import pytest

import guide_cases as gc
import moments_cases as mc
from test_gpu_layers import TOL_SAME, dev, frame, rel_linf, split_layers

pytestmark = pytest.mark.gpu


def test_cli_features_is_the_resident_call(hipctx, tmp_path):
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    W, H = 72, 56
    col, ns, hist, cov = core.synthetic_scene(W, H, 16, 21, 0.15, 0.02)
    f, v, _ = gc.features(W, H, 3, seed=4)
    stem = str(tmp_path / "frame")
    core.write_exr(stem + ".exr", col, False)
    core.write_exr(stem + "_hist.exr", core.merge_hist_ns(hist, ns), True)
    core.write_exr(stem + "_cov.exr", cov, True)
    core.write_exr(stem + "_f.exr", f, True)
    core.write_exr(stem + "_fv.exr", v, True)
    col_disk = core.read_exr(stem + ".exr", False)                                      # (colours go through half precision on disk, features do not)
    assert np.array_equal(core.read_exr(stem + "_f.exr", True), f) and np.array_equal(core.read_exr(stem + "_fv.exr", True), v)
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    d_ns, d_hist, d_f, d_v = dev(ns, hist, f, v)
    d_layer = tuple(dev(col_disk, cov))
    prm = bh.default_params(b=4, m=0.0, seed=5)
    plain = hipctx.zero_bad_values(hipctx.denoise_layers(d_ns, d_hist, [d_layer], 2, prm)[0]).cpu().numpy()
    for name, tail, kw in (("with variances", ["--feature-variances", stem + "_fv.exr", "--feature-floors", "1e-4,1e-4,1e-4"], dict(variances=d_v, floors=[1e-4] * 3, threshold=1.0)),
                           ("floors only", ["--feature-floors", "0.01,0,0.01", "--feature-threshold", "0.75"], dict(variances=None, floors=[0.01, 0.0, 0.01], threshold=0.75))):
        out_path = str(tmp_path / ("out_%d.exr" % len(tail)))
        r = subprocess.run([exe, "-i", stem + ".exr", "-o", out_path, "-p", "0", "-s", "2", "-b", "4", "-m", "0", "--seed", "5", "--features", stem + "_f.exr"] + tail,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        want = hipctx.denoise_guided(d_ns, d_hist, [d_layer], 2, prm, d_f, **kw)[0]
        w = hipctx.zero_bad_values(want).cpu().numpy()
        got = core.read_exr(out_path, False)
        same = TOL_SAME * np.max(np.abs(w))
        bound = same + np.maximum(2.0 ** -11 * (np.abs(w) + same), 2.0 ** -25)
        worst = float(np.max(np.abs(got - w) / bound))
        print("bcd_cli --features, %s: worst deviation from the resident call %.3f of the bound (TOL_SAME + binary16 rounding)" % (name, worst))
        assert np.all(np.abs(got - w) <= bound)
        assert rel_linf(w, plain) > 1e-3                                                # the gate did something


@pytest.mark.parametrize("nscales,with_hist", [(1, True), (3, True), (3, False)])
def test_set_guide_features_is_the_resident_call(hipctx, nscales, with_hist):
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    W, H = 90, 52
    col, ns, hist, cov = frame(W, H, 8)
    layers = split_layers(col, cov, 2)
    f, v, _ = gc.features(W, H, 3, seed=7)
    fl = gc.floors(3, True)
    ok, got = core.denoise_guided(layers, ns, hist if with_hist else None, f, v, fl, 1.0, nscales=nscales, seed=21, m=1.0, var_floor=1e-6)
    assert ok
    d_ns, d_hist, d_f, d_v = dev(ns, hist, f, v)
    prm = bh.default_params(m=1.0, random_order=1, seed=21)
    d_layers = [tuple(dev(c, x)) for c, x in layers]
    want = [o.cpu().numpy() for o in hipctx.denoise_guided(d_ns, d_hist if with_hist else None, d_layers, nscales, prm, d_f, d_v, fl, 1.0, var_floor=1e-6)]
    for k in range(2):
        e = rel_linf(got[k], want[k])
        print("setGuideFeatures, %d scale(s), %s, layer %d: vs the resident call %.3e" % (nscales, "histograms" if with_hist else "moment selection", k, e))
        assert e <= TOL_SAME
    # a null features pointer switches the gate off: the unguided call
    ok, off = core.denoise_guided(layers[:1], ns, hist if with_hist else None, None, nscales=nscales, seed=21, m=1.0, var_floor=1e-6)
    assert ok
    unguided = (hipctx.denoise_layers(d_ns, d_hist, d_layers[:1], nscales, prm) if with_hist else hipctx.denoise_moments(d_ns, d_layers[:1], nscales, prm, 1e-6))[0].cpu().numpy()
    assert rel_linf(off[0], unguided) <= TOL_SAME and rel_linf(got[0], unguided) > 1e-3
