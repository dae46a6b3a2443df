"""Reference of the colour layers of a frame denoised with its neighbour frames (bcd_hip_denoise_temporal_layers, bcd_hip_bayes_accumulate_temporal_layers;
DESIGN.md section 16, "Layers").  TEST INFRASTRUCTURE.

By definition layer k of the layered call is what the single-layer call returns on layer k's colours and covariances of every frame with the shared sample
counts and histograms.  So the reference of layer k IS tests/temporal_ref.py run on that layer: nothing is shared between the layers here, and the selection
is computed again for each of them -- that the per-scale figures then agree across the layers is asserted by tests/test_temporal_layers_cases_cpu.py, not
assumed."""
import numpy as np

import temporal_ref as tr


def accumulate(layered, k, dtype=np.float64):
    """the estimate stage on layer k of a temporal_layers_cases.LayeredCase -> (sum, count, per_item) of temporal_ref.accumulate"""
    return tr.accumulate(*layered.layer(k).args(), dtype=dtype)


def denoise_multiscale(ns, hist, layers, neighbours, k, nscales, w, b, tau, min_eig, orders, draws, dtype=np.float64):
    """layers: [(colours, covariances)] of the frame; neighbours: [(ns, hist, [(colours, covariances)])] -> (layer k of the result, per-scale stats)"""
    frame = (layers[k][0], ns, hist, layers[k][1])
    nb = [(lay[k][0], ns_f, hist_f, lay[k][1]) for (ns_f, hist_f, lay) in neighbours]
    return tr.denoise_multiscale(frame, nb, nscales, w, b, tau, min_eig, orders, draws, dtype)
