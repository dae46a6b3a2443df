// bcd_spike.h -- the decision of the spike prefilter, shared by the kernel that filters (k_spike, k_pointwise.hip) and the kernel that only
// records the decision as a source map (k_spike_map, k_spike.hip): one function, so the two cannot drift apart.  Device code only.
#pragma once
#include "bcd_common.h"

// SpikeRemovalFilter::filter (src/core/SpikeRemovalFilter.cpp:18-116), float-abs semantics: the pixel whose values the filter copies into pixel
// (l, c) of a W x H colour image (W, H >= 3), as a linear pixel index -- (l, c) itself where the pixel is no spike.  The window is the nine
// neighbours centred on the pixel, centred one pixel inward at the frame border; mean and standard deviation per channel in the reference's
// operation order, a spike when one channel is further than factor * sd from its mean, replaced by the window's L1 median.
__device__ __forceinline__ size_t bcd_spike_source(const float *__restrict__ col, int W, int H, int l, int c, float factor)
{
    size_t src = (size_t)l * W + c;
    int cl = l < 1 ? 1 : (l > H - 2 ? H - 2 : l);
    int cc = c < 1 ? 1 : (c > W - 2 ? W - 2 : c);
    float v[3][9];
    int k = 0;
    for (int nl = cl - 1; nl <= cl + 1; ++nl)
        for (int nc = cc - 1; nc <= cc + 1; ++nc, ++k) {
            const float *px = col + ((size_t)nl * W + nc) * 3;
            v[0][k] = px[0]; v[1][k] = px[1]; v[2][k] = px[2];
        }
    const float *me = col + ((size_t)l * W + c) * 3;
    bool spike = false;
    for (int ch = 0; ch < 3; ++ch) {
        float total = 0.f;
        for (int i = 0; i < 9; ++i) total += v[ch][i];
        float avg = total / 9;
        total = 0;
        for (int i = 0; i < 9; ++i) total += (v[ch][i] - avg) * (v[ch][i] - avg);
        float sd = sqrtf(total / 8);
        spike = spike || (fabsf(me[ch] - avg) > factor * sd);
    }
    if (spike) {
        int best = 0;
        float bestd = -1.f;
        for (int m = 0; m < 9; ++m) {
            float tot = 0.f;
            for (int i = 0; i < 9; ++i)
                tot += fabsf(v[0][i] - v[0][m]) + fabsf(v[1][i] - v[1][m]) + fabsf(v[2][i] - v[2][m]);
            if (bestd < 0 || tot < bestd) { bestd = tot; best = m; }
        }
        src = (size_t)(cl - 1 + best / 3) * W + (cc - 1 + best % 3);
    }
    return src;
}
