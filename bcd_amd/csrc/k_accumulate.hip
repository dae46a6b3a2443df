// k_accumulate.hip -- the persistent device SamplesAccumulator (bcd_hip_accum_*, include/bcd_hip.h): the reference's running sums
// (src/core/SamplesAccumulator.cpp:44-105) kept in HBM between calls, fed in batches, and snapshotted into the statistics images
// (computeSampleStatistics, :108-141) without being changed.
//
// State: (11 + D) fp32 PLANES of W*H values each, plane-major -- weight sum, squared-weight sum, 3 weighted colour sums, 6 weighted
// second moments (xx,yy,zz,yz,xz,xy), then the D = 3 * nb_bins histogram bins (channel-major, bin index ch * nb_bins + bin).  One thread
// owns one pixel, so every plane read or written by a wavefront is 64 consecutive floats; a 1-sample pass touches 6 of the D bin planes,
// the ones its colours fall in (neighbouring pixels mostly share them).
//
// Determinism: every pixel's samples are applied by one thread, in stream order, with the same float operations in the same order as
// SamplesAccumulator::addSample and k_accumulate_samples (-ffp-contract=off).  No float atomics anywhere; the scattered path sorts
// (pixel, sample index) with a stable radix sort and walks each pixel's run in order.  A merge of two states is one fp32 add per element
// (the sums are plain running sums), so it is as deterministic as the rest.
#include <algorithm>
#include <type_traits>
#include <cstring> // (before rocprim: texture_cache_iterator.hpp uses memset)
#include <rocprim/rocprim.hpp>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "accum_kernels.h"
#include "bcd_common.h"

namespace {

// the binning of one colour channel, SamplesAccumulator.cpp:66-90 (same expressions as k_accumulate_samples)
__device__ inline void acc_bin(float x, int nbins, float gamma, float maxval, int &lo, float &lw, float &hw)
{
    const float sat = 2.f;
    float v = x > 0 ? x : 0;
    if (gamma > 1) v = powf(v, 1.f / gamma);
    if (maxval > 0) v = v / maxval;
    v = v > sat ? sat : v;
    const float fi = v * (nbins - 2);
    lo = (int)fi;
    if (lo < nbins - 2) hw = fi - lo;
    else { lo = nbins - 2; hw = (v - 1.0f) / (sat - 1.f); }
    lw = 1.0f - hw;
}

struct AccSums {
    float wsum, w2sum, m[3], c[6];
    __device__ void load(const float *__restrict__ st, int64_t N, int64_t p)
    {
        wsum = st[ACC_W * N + p]; w2sum = st[ACC_W2 * N + p];
        for (int i = 0; i < 3; ++i) m[i] = st[(ACC_M + i) * N + p];
        for (int i = 0; i < 6; ++i) c[i] = st[(ACC_C + i) * N + p];
    }
    __device__ void store(float *__restrict__ st, int64_t N, int64_t p) const
    {
        st[ACC_W * N + p] = wsum; st[ACC_W2 * N + p] = w2sum;
        for (int i = 0; i < 3; ++i) st[(ACC_M + i) * N + p] = m[i];
        for (int i = 0; i < 6; ++i) st[(ACC_C + i) * N + p] = c[i];
    }
    // SamplesAccumulator.cpp:53-65, in its order
    __device__ void add(float R, float G, float B, float w)
    {
        wsum += w;
        w2sum += w * w;
        m[0] += w * R; m[1] += w * G; m[2] += w * B;
        c[0] += w * R * R; c[1] += w * G * G; c[2] += w * B * B;
        c[3] += w * G * B; c[4] += w * R * B; c[5] += w * R * G;
    }
};

// computeSampleStatistics of one pixel (SamplesAccumulator.cpp:108-141): the mean and the bias-corrected covariance (xx,yy,zz,yz,xz,xy);
// the number of samples is s.wsum.  Shared by the snapshot and the plan's error pass, so that both see the same bits.
__device__ inline void acc_statistics(const AccSums &s, float mean[3], float cov[6])
{
    const float inv = 1.f / s.wsum;
    for (int i = 0; i < 3; ++i) mean[i] = inv * s.m[i];
    float cv[6];
    for (int i = 0; i < 6; ++i) cv[i] = s.c[i] * inv;
    cv[0] -= mean[0] * mean[0]; cv[1] -= mean[1] * mean[1]; cv[2] -= mean[2] * mean[2];
    cv[3] -= mean[1] * mean[2]; cv[4] -= mean[0] * mean[2]; cv[5] -= mean[0] * mean[1];
    const float bias = 1.f / (1 - s.w2sum / (s.wsum * s.wsum));
    for (int i = 0; i < 6; ++i) cov[i] = cv[i] * bias;
}

// Colour layers (bcd_hip_accum_*_layers): a layer keeps the nine colour sums only, ACC_LAYER_PLANES planes of N floats
// in the order of ACC_M / ACC_C, layer after layer in a buffer of its own; the weight sum and the squared-weight sum are the beauty's.
// One thread owns one (pixel, layer) and applies its contributions in stream order: the nine m / c lines of AccSums::add with the same
// weight, so a layer has the bits of a separate accumulator fed its colours.
#define ACC_LAYER_PLANES 9
struct LayerSums {
    float m[3], c[6];
    __device__ void load(const float *__restrict__ ly, int64_t N, int64_t p)
    {
        for (int i = 0; i < 3; ++i) m[i] = ly[i * N + p];
        for (int i = 0; i < 6; ++i) c[i] = ly[(3 + i) * N + p];
    }
    __device__ void store(float *__restrict__ ly, int64_t N, int64_t p) const
    {
        for (int i = 0; i < 3; ++i) ly[i * N + p] = m[i];
        for (int i = 0; i < 6; ++i) ly[(3 + i) * N + p] = c[i];
    }
    __device__ void add(float R, float G, float B, float w)
    {
        m[0] += w * R; m[1] += w * G; m[2] += w * B;
        c[0] += w * R * R; c[1] += w * G * G; c[2] += w * B * B;
        c[3] += w * G * B; c[4] += w * R * B; c[5] += w * R * G;
    }
};

// (a) dense add: pixels [p0, p0 + npix) of the frame, k samples each (contiguous, `channels` floats per sample, the 4th ignored).
// STAGED = false: the 6k touched bins are read-modified-written in HBM directly (a progressive pass of k = 1 moves 6 of the D bins);
// STAGED = true: the pixel's D bins are loaded into LDS ([bin][thread], bank-conflict free), accumulated there and written back once.
template <bool STAGED>
__global__ __launch_bounds__(64) void k_accum_dense(const float *__restrict__ samples, const float *__restrict__ weights, int64_t p0, int64_t npix,
                                                    int64_t N, int k, int channels, int nbins, float gamma, float maxval, float *__restrict__ st)
{
    extern __shared__ float lds_h[];
    const int t = threadIdx.x, D = 3 * nbins;
    const int64_t q = (int64_t)blockIdx.x * 64 + t; // pixel within the batch
    if (q >= npix) return;                          // (no barrier below: each thread only touches its own LDS column)
    const int64_t p = p0 + q;
    float *hp = st + (int64_t)ACC_H * N + p;        // bin b of this pixel: hp[b * N]
    if (STAGED)
        for (int b = 0; b < D; ++b) lds_h[b * 64 + t] = hp[b * N];
    AccSums s;
    s.load(st, N, p);
    const float *sp = samples + q * k * channels;
    const float *wp = weights ? weights + q * k : nullptr;
    for (int i = 0; i < k; ++i) {
        const float R = sp[i * channels], G = sp[i * channels + 1], B = sp[i * channels + 2];
        const float w = wp ? wp[i] : 1.f;
        s.add(R, G, B, w);
        const float rgb[3] = { R, G, B };
        for (int ch = 0; ch < 3; ++ch) {
            int lo;
            float lw, hw;
            acc_bin(rgb[ch], nbins, gamma, maxval, lo, lw, hw);
            const int b = ch * nbins + lo;
            if (STAGED) {
                lds_h[b * 64 + t] += w * lw;
                lds_h[(b + 1) * 64 + t] += w * hw;
            } else {
                hp[b * N] += w * lw;
                hp[(b + 1) * N] += w * hw;
            }
        }
    }
    s.store(st, N, p);
    if (STAGED)
        for (int b = 0; b < D; ++b) hp[b * N] = lds_h[b * 64 + t];
}

// (a') dense add of the layers: blockIdx.y = layer, one thread per (pixel, layer); a 1-sample pass moves the sample, its weight and the
// nine planes twice
__global__ __launch_bounds__(256) void k_accum_dense_layers(BcdAccumLayerIn in, const float *__restrict__ weights, int64_t p0, int64_t npix,
                                                            int64_t N, int k, int channels, float *__restrict__ layers)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= npix) return;
    const int64_t p = p0 + q;
    float *ly = layers + (int64_t)blockIdx.y * ACC_LAYER_PLANES * N;
    LayerSums s;
    s.load(ly, N, p);
    const float *sp = in.src[blockIdx.y] + q * k * channels;
    const float *wp = weights ? weights + q * k : nullptr;
    for (int i = 0; i < k; ++i) s.add(sp[i * channels], sp[i * channels + 1], sp[i * channels + 2], wp ? wp[i] : 1.f);
    s.store(ly, N, p);
}

// (b) scattered add, step 1: key = pixel index (out-of-range indices -> N, sorted past every pixel and skipped), value = position in the
// batch; the dropped ones are counted (integer atomics, one per wavefront)
__global__ __launch_bounds__(256) void k_accum_keys(const int32_t *__restrict__ pix, int64_t n, int64_t N, uint32_t *__restrict__ keys,
                                                    uint32_t *__restrict__ vals, unsigned long long *__restrict__ dropped)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool drop = false;
    if (i < n) {
        const int32_t p = pix[i];
        const bool ok = p >= 0 && (int64_t)p < N;
        keys[i] = ok ? (uint32_t)p : (uint32_t)N;
        vals[i] = (uint32_t)i;
        drop = !ok;
    }
    const unsigned long long bal = __ballot(drop);
    if (bal && (threadIdx.x & 63) == __ffsll((long long)bal) - 1) atomicAdd(dropped, (unsigned long long)__popcll(bal));
}

// one sample into a pixel's running sums (registers) and its bins in HBM (hp[b * N] = bin b of the pixel): addSample of the scattered and
// the splatted paths
__device__ inline void acc_add_sample(AccSums &s, float *__restrict__ hp, int64_t N, float R, float G, float B, float w, int nbins, float gamma,
                                      float maxval)
{
    s.add(R, G, B, w);
    const float c3[3] = { R, G, B };
    for (int ch = 0; ch < 3; ++ch) {
        int lo;
        float lw, hw;
        acc_bin(c3[ch], nbins, gamma, maxval, lo, lw, hw);
        const int b = ch * nbins + lo;
        hp[b * N] += w * lw;
        hp[(b + 1) * N] += w * hw;
    }
}

// (b) step 3: one thread per run of equal keys in the stably sorted batch walks the run -- the pixel's samples in stream order
__global__ __launch_bounds__(256) void k_accum_segments(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, int64_t n, int64_t N,
                                                        const float *__restrict__ rgb, const float *__restrict__ weights, int nbins, float gamma,
                                                        float maxval, float *__restrict__ st)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t key = keys[i];
    if ((int64_t)key >= N || (i > 0 && keys[i - 1] == key)) return;
    const int64_t p = key;
    float *hp = st + (int64_t)ACC_H * N + p;
    AccSums s;
    s.load(st, N, p);
    for (int64_t j = i; j < n && keys[j] == key; ++j) {
        const int64_t e = vals[j];
        acc_add_sample(s, hp, N, rgb[e * 3], rgb[e * 3 + 1], rgb[e * 3 + 2], weights ? weights[e] : 1.f, nbins, gamma, maxval);
    }
    s.store(st, N, p);
}

// (b) step 3 for the layers, on the same sorted keys and values: blockIdx.y = layer
__global__ __launch_bounds__(256) void k_accum_segments_layers(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, int64_t n,
                                                               int64_t N, BcdAccumLayerIn in, const float *__restrict__ weights,
                                                               float *__restrict__ layers)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t key = keys[i];
    if ((int64_t)key >= N || (i > 0 && keys[i - 1] == key)) return;
    const int64_t p = key;
    float *ly = layers + (int64_t)blockIdx.y * ACC_LAYER_PLANES * N;
    const float *rgb = in.src[blockIdx.y];
    LayerSums s;
    s.load(ly, N, p);
    for (int64_t j = i; j < n && keys[j] == key; ++j) {
        const int64_t e = vals[j];
        s.add(rgb[e * 3], rgb[e * 3 + 1], rgb[e * 3 + 2], weights ? weights[e] : 1.f);
    }
    s.store(ly, N, p);
}

// (b') splatted add (bcd_hip_accum_add_splatted; the definition is in include/bcd_hip.h, the design in DESIGN.md section 10): samples at
// continuous positions go through the accumulator's reconstruction filter to every pixel of their footprint.  Gather form: the n samples
// are sorted by their CELL (the pixel floor(x), floor(y) on the frame extended by (kx, ky)), and one thread per destination pixel merges
// the runs of the cells around it by batch position -- the pixel's contributions in stream order, no float atomics.
// step 1: key = the sample's cell on the extended frame, value = position in the batch.  Samples that contribute nothing (position not
// finite or outside the extended frame, empty footprint: a pure function of the sample and the filter) get the past-the-end key and are
// counted as dropped (integer atomics, one per wavefront)
__global__ __launch_bounds__(256) void k_accum_splat_keys(const float *__restrict__ xy, int64_t n, int W, int H, SplatFilter F,
                                                          const float *__restrict__ T, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                          unsigned long long *__restrict__ dropped)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool drop = false;
    if (i < n) {
        const int We = W + 2 * F.kx, He = H + 2 * F.ky;
        const float x = xy[2 * i], y = xy[2 * i + 1];
        uint32_t key = (uint32_t)((int64_t)We * He);
        bool ok = __builtin_isfinite(x) && __builtin_isfinite(y) && x >= -(float)F.kx && x < (float)(W + F.kx) && y >= -(float)F.ky &&
                  y < (float)(H + F.ky);
        if (ok) {
            const int c0 = (int)floorf(x), l0 = (int)floorf(y);
            const int ca = c0 - F.nx > 0 ? c0 - F.nx : 0, cb = c0 + F.nx < W - 1 ? c0 + F.nx : W - 1;
            const int la = l0 - F.ny > 0 ? l0 - F.ny : 0, lb = l0 + F.ny < H - 1 ? l0 + F.ny : H - 1;
            bool any = false;
            for (int line = la; line <= lb && !any; ++line)
                for (int col = ca; col <= cb && !any; ++col) any = splat_weight(F, T, x, y, col, line) != 0.f;
            ok = any;
            if (any) key = (uint32_t)((int64_t)(l0 + F.ky) * We + (c0 + F.kx));
        }
        keys[i] = key;
        vals[i] = (uint32_t)i;
        drop = !ok;
    }
    const unsigned long long bal = __ballot(drop);
    if (bal && (threadIdx.x & 63) == __ffsll((long long)bal) - 1) atomicAdd(dropped, (unsigned long long)__popcll(bal));
}

// step 3: the run of every cell in the sorted batch, [cells[c].x, cells[c].y) (the array is zeroed before: empty cells stay (0, 0))
__global__ __launch_bounds__(256) void k_accum_splat_cells(const uint32_t *__restrict__ keys, int64_t n, uint32_t NE, uint2 *__restrict__ cells)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t key = keys[i];
    if (key >= NE) return;
    if (i == 0 || keys[i - 1] != key) cells[key].x = (uint32_t)i;
    if (i == n - 1 || keys[i + 1] != key) cells[key].y = (uint32_t)(i + 1);
}

// step 4 (the tile, its ring and the merge of a pixel's runs: accum_kernels.h)
#define SPLAT_SAMPLE_BYTES 28                                                                // staged: position, x, y, r, g, b, weight

// the samples of the ring's cells with their colours and weights
template <bool STAGED>
struct SplatRuns : SplatKeys<STAGED> {
    const float *s_r, *s_g, *s_b, *s_w;               // LDS staging arrays
    const float *rgb, *weights;                       // the batch itself
    __device__ void colour(uint32_t i, float &R, float &G, float &B, float &w) const
    {
        if (STAGED) { R = s_r[i]; G = s_g[i]; B = s_b[i]; w = s_w[i]; }
        else { const int64_t e = this->vals[i]; R = rgb[3 * e]; G = rgb[3 * e + 1]; B = rgb[3 * e + 2]; w = weights ? weights[e] : 1.f; }
    }
};

// one destination pixel: adds each contribution of splat_merge as k_accum_segments does.  LAYER: st is a layer's nine planes and the
// colours are the layer's -- the sums alone, no bins
template <bool STAGED, bool LAYER>
__device__ inline void splat_pixel(const SplatRuns<STAGED> &S, const SplatFilter &F, const float *T, int rc0, int RW, int col, int line, int64_t p,
                                   int64_t N, int nbins, float gamma, float maxval, float *__restrict__ st)
{
    float *hp = LAYER ? st : st + (int64_t)ACC_H * N + p;
    typename std::conditional<LAYER, LayerSums, AccSums>::type s;
    bool loaded = false;
    splat_merge(S, F, T, rc0, RW, col, line, [&](uint32_t idx, float f) {
        if (!loaded) { s.load(st, N, p); loaded = true; }
        float R, G, B, w;
        S.colour(idx, R, G, B, w);
        if constexpr (LAYER) s.add(R, G, B, w * f);
        else acc_add_sample(s, hp, N, R, G, B, w * f, nbins, gamma, maxval);
    });
    if (loaded) s.store(st, N, p); // (a pixel without contributions does not touch its planes)
}

// dynamic LDS: the table (ts * ts), g0[SPLAT_RING_MAX], b0[SPLAT_RING_MAX + 4], then 7 staging arrays of `cap` entries.
// LAYER: one colour layer of the chunk the beauty's launch has just served (rgb: the layer's colours, st: its nine planes)
template <bool LAYER>
__global__ __launch_bounds__(256) void k_accum_splat(const uint2 *__restrict__ cells, const uint32_t *__restrict__ vals, const float *__restrict__ xy,
                                                     const float *__restrict__ rgb, const float *__restrict__ weights, int W, int H, int tiles_x,
                                                     SplatFilter F, const float *__restrict__ T, int cap, int nbins, float gamma, float maxval,
                                                     float *__restrict__ st)
{
    extern __shared__ float lds_s[];
    const int t = threadIdx.x, tt = F.ts * F.ts;
    float *s_T = lds_s;
    uint32_t *s_g0 = (uint32_t *)(lds_s + tt), *s_b0 = s_g0 + SPLAT_RING_MAX, *s_pos = s_b0 + SPLAT_RING_MAX + 4;
    float *s_x = (float *)(s_pos + cap), *s_y = s_x + cap, *s_r = s_y + cap, *s_g = s_r + cap, *s_b = s_g + cap, *s_w = s_b + cap;
    const int px0 = (int)(blockIdx.x % (unsigned)tiles_x) * SPLAT_TX, py0 = (int)(blockIdx.x / (unsigned)tiles_x) * SPLAT_TY;
    const int RW = SPLAT_TX + 2 * F.nx, RC = RW * (SPLAT_TY + 2 * F.ny);
    const uint32_t total = splat_ring_load(cells, T, F, W, H, px0, py0, s_T, s_g0, s_b0);
    if (total == 0) return;
    const bool staged = total <= (uint32_t)cap; // (uniform over the workgroup)
    if (staged) {
        for (uint32_t j = t; j < total; j += 256) {
            const int64_t e = splat_slot_sample(s_g0, s_b0, RC, vals, j);
            s_pos[j] = (uint32_t)e;
            s_x[j] = xy[2 * e]; s_y[j] = xy[2 * e + 1];
            s_r[j] = rgb[3 * e]; s_g[j] = rgb[3 * e + 1]; s_b[j] = rgb[3 * e + 2];
            s_w[j] = weights ? weights[e] : 1.f;
        }
        __syncthreads();
    }
    const int lx = t % SPLAT_TX, ly = t / SPLAT_TX, col = px0 + lx, line = py0 + ly;
    if (col >= W || line >= H) return;
    const int64_t N = (int64_t)W * H, p = (int64_t)line * W + col;
    const int rc0 = ly * RW + lx;
    if (staged) {
        const SplatRuns<true> S = { { s_g0, s_b0, s_pos, s_x, s_y, vals, xy }, s_r, s_g, s_b, s_w, rgb, weights };
        splat_pixel<true, LAYER>(S, F, s_T, rc0, RW, col, line, p, N, nbins, gamma, maxval, st);
    } else {
        const SplatRuns<false> S = { { s_g0, s_b0, s_pos, s_x, s_y, vals, xy }, s_r, s_g, s_b, s_w, rgb, weights };
        splat_pixel<false, LAYER>(S, F, s_T, rc0, RW, col, line, p, N, nbins, gamma, maxval, st);
    }
}

// (c) snapshot: computeSampleStatistics (SamplesAccumulator.cpp:108-141) of 64 pixels per workgroup into DeepImage layout; the bin planes
// are transposed through LDS ([pixel][D + 1]) so that both the plane reads and the interleaved writes are coalesced.  State is read only.
__global__ __launch_bounds__(64) void k_accum_snapshot(const float *__restrict__ st, int64_t N, int D, float *__restrict__ ons,
                                                       float *__restrict__ omean, float *__restrict__ ocov, float *__restrict__ ohist)
{
    extern __shared__ float lds_t[];
    const int t = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * 64, p = p0 + t;
    const int cnt = (int)(N - p0 < 64 ? N - p0 : 64);
    if (t < cnt) {
        AccSums s;
        s.load(st, N, p);
        float mean[3], cov[6];
        acc_statistics(s, mean, cov);
        for (int i = 0; i < 3; ++i) omean[p * 3 + i] = mean[i];
        for (int i = 0; i < 6; ++i) ocov[p * 6 + i] = cov[i];
        ons[p] = s.wsum;
        const float *hp = st + (int64_t)ACC_H * N + p;
        for (int b = 0; b < D; ++b) lds_t[t * (D + 1) + b] = hp[b * N];
    }
    __syncthreads();
    float *oh = ohist + p0 * D;
    for (int e = t; e < cnt * D; e += 64) {
        const int q = e / D;
        oh[e] = lds_t[q * (D + 1) + (e - q * D)];
    }
}

// (c0) the snapshot without the bins: the AccSums planes in (11 plane-major reads of 64 consecutive floats per wavefront), nSamples / mean /
// covariance out through acc_statistics -- the bits of k_accum_snapshot's three images -- 44 B read and 40 B written per pixel.  No LDS: the
// transpose of k_accum_snapshot serves the bin planes only.  State is read only.
__global__ __launch_bounds__(256) void k_accum_moments(const float *__restrict__ st, int64_t N, float *__restrict__ ons, float *__restrict__ omean,
                                                       float *__restrict__ ocov)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    AccSums s;
    s.load(st, N, p);
    float mean[3], cov[6];
    acc_statistics(s, mean, cov);
    for (int i = 0; i < 3; ++i) omean[p * 3 + i] = mean[i];
    for (int i = 0; i < 6; ++i) ocov[p * 6 + i] = cov[i];
    ons[p] = s.wsum;
}

// (c') snapshot of the layers: acc_statistics on a layer's nine sums with the beauty's weight sum and squared-weight sum; blockIdx.y =
// layer.  Reads 8 + 36 B and writes 36 B per pixel and layer; state and layers are read only.
__global__ __launch_bounds__(256) void k_accum_snapshot_layers(const float *__restrict__ st, const float *__restrict__ layers, int64_t N,
                                                               BcdAccumLayerOut out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    LayerSums l;
    l.load(layers + (int64_t)blockIdx.y * ACC_LAYER_PLANES * N, N, p);
    AccSums s;
    s.wsum = st[ACC_W * N + p]; s.w2sum = st[ACC_W2 * N + p];
    for (int i = 0; i < 3; ++i) s.m[i] = l.m[i];
    for (int i = 0; i < 6; ++i) s.c[i] = l.c[i];
    float mean[3], cov[6];
    acc_statistics(s, mean, cov);
    float *omean = out.mean[blockIdx.y], *ocov = out.cov[blockIdx.y];
    for (int i = 0; i < 3; ++i) omean[p * 3 + i] = mean[i];
    for (int i = 0; i < 6; ++i) ocov[p * 6 + i] = cov[i];
}

// (d) adaptive plan (bcd_hip_accum_plan).  Reductions of the error pass: the largest finite error of the active
// pixels as float bits (errors are >= 0, so the bits order like the values: an integer max is exact and order-independent), and the
// active / unsampled counts packed in one word (active << 32 | unsampled; both < 2^31, so the low half never carries).
struct PlanRed {
    unsigned int emax, pad;
    unsigned long long counts;
};

// e_p: the relative standard error of the pixel's mean, sqrt(trace(cov / n) / 3) / (eps + luminance), from the snapshot's statistics;
// +inf for pixels below min_samples and for non-finite statistics
__device__ inline float plan_error(const AccSums &s, float eps, float min_samples)
{
    float mean[3], cov[6];
    acc_statistics(s, mean, cov);
    const float ns = s.wsum, inv = 1.f / ns;
    const float t = (cov[0] * inv + cov[1] * inv) + cov[2] * inv;
    const float l = (mean[0] + mean[1]) + mean[2];
    if (!(ns >= min_samples) || !__builtin_isfinite(t) || !__builtin_isfinite(l)) return __builtin_inff();
    return sqrtf(fmaxf(t / 3.f, 0.f)) / (eps + fmaxf(l / 3.f, 0.f));
}

// plane-major error pass: 11 state planes in, e out, over a grid of at most PLAN_ERROR_BLOCKS workgroups striding the frame; one
// wavefront reduction per wave, then one integer atomic per workgroup and word (the atomics all hit one address and serialise in L2,
// so their number is kept near the CU count rather than N / 256)
#define PLAN_ERROR_BLOCKS 1024
__global__ __launch_bounds__(256) void k_plan_error(const float *__restrict__ st, int64_t N, float eps, float min_samples, float tau,
                                                    float *__restrict__ err, PlanRed *__restrict__ red)
{
    __shared__ unsigned int s_e[4];
    __shared__ unsigned long long s_c[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned int eb = 0;
    unsigned long long cnt = 0;
    for (int64_t p0 = (int64_t)blockIdx.x * 256; p0 < N; p0 += (int64_t)gridDim.x * 256) {
        const int64_t p = p0 + t;
        bool act = false, uns = false;
        if (p < N) {
            AccSums s;
            s.load(st, N, p);
            const float e = plan_error(s, eps, min_samples);
            err[p] = e;
            act = e > tau;
            uns = act && __builtin_isinf(e);
            if (act && !uns && __float_as_uint(e) > eb) eb = __float_as_uint(e);
        }
        cnt += ((unsigned long long)__popcll(__ballot(act)) << 32) + (unsigned long long)__popcll(__ballot(uns));
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned int x = __shfl_xor(eb, o);
        eb = x > eb ? x : eb;
    }
    if (lane == 0) { s_e[wave] = eb; s_c[wave] = cnt; }
    __syncthreads();
    if (t == 0) {
        unsigned int e = s_e[0];
        unsigned long long c = s_c[0];
        for (int w = 1; w < 4; ++w) { e = s_e[w] > e ? s_e[w] : e; c += s_c[w]; }
        if (e) atomicMax(&red->emax, e);
        if (c) atomicAdd(&red->counts, c);
    }
}

// q_p, the integer weight of a pixel: 0 (converged), 2^24 (e = inf), else max(1, floor(2^24 e / E)); E is read from the device
struct PlanWeight {
    const PlanRed *red;
    float tau;
    __device__ uint64_t operator()(float e) const
    {
        if (!(e > tau)) return 0;
        if (__builtin_isinf(e)) return (uint64_t)1 << 24;
        const uint32_t q = (uint32_t)((e / __uint_as_float(red->emax)) * 16777216.f);
        return q > 1 ? q : 1;
    }
};

// floor((c B + u) / Q) for c <= Q <= 2^55, B < 2^31, u < Q: the quotient is at most B, so a double estimate is off by at most one and is
// corrected exactly in 128 bits
__device__ inline uint64_t plan_floor(uint64_t c, uint64_t B, uint64_t u, uint64_t Q)
{
    const unsigned __int128 x = (unsigned __int128)c * B + u;
    uint64_t f = (uint64_t)(((double)c * (double)B + (double)u) / (double)Q);
    unsigned __int128 m = (unsigned __int128)f * Q;
    while (m > x) { --f; m -= Q; }
    while (x - m >= Q) { ++f; m += Q; }
    return f;
}

// n_p = min(K, F(C_p) - F(C_{p-1})), F(c) = floor((c B + u mod Q) / Q): the budget split in proportion to q, exactly B before the cap
__global__ __launch_bounds__(256) void k_plan_counts(const uint64_t *__restrict__ C, int64_t N, int64_t B, uint64_t offset, int K,
                                                     int32_t *__restrict__ counts)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const uint64_t Q = C[N - 1];
    int32_t n = 0;
    if (Q != 0 && B != 0) {
        const uint64_t u = offset % Q, c1 = C[p], c0 = p > 0 ? C[p - 1] : 0;
        const uint64_t d = plan_floor(c1, (uint64_t)B, u, Q) - plan_floor(c0, (uint64_t)B, u, Q);
        n = d < (uint64_t)K ? (int32_t)d : K;
    }
    counts[p] = n;
}

// the summary, once the positions are known
__global__ void k_plan_summary(const PlanRed *__restrict__ red, const int32_t *__restrict__ ends, int64_t N, int64_t *__restrict__ summary)
{
    summary[0] = ends[N - 1];
    summary[1] = (int64_t)(red->counts >> 32);
    summary[2] = (int64_t)(red->counts & 0xffffffffu);
    *(float *)(summary + 3) = __uint_as_float(red->emax);
}

// the pixel list: pixel p at [ends[p-1], ends[p]).  Short runs are written by their pixel's thread; runs longer than PLAN_SHORT_RUN are
// taken one at a time by the whole wavefront, 64 entries per store
#define PLAN_SHORT_RUN 16
__global__ __launch_bounds__(256) void k_plan_expand(const int32_t *__restrict__ ends, int64_t N, int32_t *__restrict__ pixels, int64_t capacity)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int64_t e0 = 0, n = 0;
    if (p < N) {
        e0 = p > 0 ? ends[p - 1] : 0;
        n = ends[p] - e0;
        if (e0 + n > capacity) n = capacity > e0 ? capacity - e0 : 0; // (T <= budget <= capacity: never taken)
    }
    if (n <= PLAN_SHORT_RUN)
        for (int64_t j = 0; j < n; ++j) pixels[e0 + j] = (int32_t)p;
    unsigned long long longs = __ballot(n > PLAN_SHORT_RUN);
    while (longs) {
        const int src = __ffsll((long long)longs) - 1;
        longs &= longs - 1;
        const int64_t b = __shfl(e0, src), m = __shfl(n, src);
        const int32_t q = (int32_t)__shfl(p, src);
        for (int64_t j = lane; j < m; j += 64) pixels[b + j] = q;
    }
}

// (e) merge of two states (bcd_hip_accum_merge*): dst[i] = dst[i] + src[i] over a flat range of the state, one fp32
// add per element and nothing else.  Elements [head, head + 4 nvec) go as float4 (the launcher found dst + head and src + head both
// 16-byte aligned), [0, head) and the tail one at a time; bases that are not co-aligned take the scalar loop for everything (head = n).
// Grid-stride over a grid capped from the CU count.
__global__ __launch_bounds__(256) void k_accum_merge(float *__restrict__ dst, const float *__restrict__ src, int64_t n, int64_t head, int64_t nvec)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    float4 *dv = reinterpret_cast<float4 *>(dst + head);
    const float4 *sv = reinterpret_cast<const float4 *>(src + head);
    for (int64_t j = t; j < nvec; j += stride) {
        float4 a = dv[j];
        const float4 b = sv[j];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        dv[j] = a;
    }
    for (int64_t j = t; j < head; j += stride) dst[j] += src[j];
    for (int64_t j = head + 4 * nvec + t; j < n; j += stride) dst[j] += src[j];
}

// the drop counter of an import or a merge: *dst = (keep ? *dst : 0) + (src ? *src : 0) + add
__global__ void k_accum_counter(unsigned long long *dst, const unsigned long long *src, unsigned long long add, int keep)
{
    *dst = (keep ? *dst : 0ull) + (src ? *src : 0ull) + add;
}

} // namespace

// dense passes of k >= BCD_ACCUM_STAGE_SPP samples stage the pixel's histogram in LDS
#define BCD_ACCUM_STAGE_SPP 8

size_t bcd_accum_snapshot_lds(int D) { return (size_t)64 * (D + 1) * sizeof(float); }

hipError_t bcd_launch_accum_dense(const float *samples, const float *weights, int64_t p0, int64_t npix, int64_t N, int k, int channels, int nbins,
                                  float gamma, float maxval, float *st, hipStream_t s)
{
    if (npix <= 0) return hipSuccess;
    const size_t lds = (size_t)3 * nbins * 64 * sizeof(float);
    if (k >= BCD_ACCUM_STAGE_SPP && lds <= 64 * 1024)
        hipLaunchKernelGGL(k_accum_dense<true>, dim3(nblk(npix, 64)), dim3(64), lds, s, samples, weights, p0, npix, N, k, channels, nbins, gamma,
                           maxval, st);
    else
        hipLaunchKernelGGL(k_accum_dense<false>, dim3(nblk(npix, 64)), dim3(64), 0, s, samples, weights, p0, npix, N, k, channels, nbins, gamma,
                           maxval, st);
    return hipGetLastError();
}

// layers: nb_layers x 9 planes of N floats; in.src[l]: the layer's samples of the pass, `channels` floats each
hipError_t bcd_launch_accum_dense_layers(const BcdAccumLayerIn &in, int nb_layers, const float *weights, int64_t p0, int64_t npix, int64_t N, int k,
                                         int channels, float *layers, hipStream_t s)
{
    if (npix <= 0 || nb_layers <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_accum_dense_layers, dim3(nblk(npix, 256), (unsigned)nb_layers), dim3(256), 0, s, in, weights, p0, npix, N, k, channels, layers);
    return hipGetLastError();
}

hipError_t bcd_launch_accum_keys(const int32_t *pix, int64_t n, int64_t N, uint32_t *keys, uint32_t *vals, unsigned long long *dropped, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_accum_keys, dim3(nblk(n, 256)), dim3(256), 0, s, pix, n, N, keys, vals, dropped);
    return hipGetLastError();
}

// stable LSD radix sort of (key, value) pairs on the low end_bit bits; tmp == nullptr: *tmp_bytes <- the scratch it needs
hipError_t bcd_accum_sort(void *tmp, size_t *tmp_bytes, const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout, int64_t n,
                          int end_bit, hipStream_t s)
{
    size_t bytes = *tmp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, (size_t)n, 0u, (unsigned)end_bit, s, false);
    *tmp_bytes = bytes;
    return e;
}

hipError_t bcd_launch_accum_segments(const uint32_t *keys, const uint32_t *vals, int64_t n, int64_t N, const float *rgb, const float *weights,
                                     int nbins, float gamma, float maxval, float *st, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_accum_segments, dim3(nblk(n, 256)), dim3(256), 0, s, keys, vals, n, N, rgb, weights, nbins, gamma, maxval, st);
    return hipGetLastError();
}

hipError_t bcd_launch_accum_segments_layers(const uint32_t *keys, const uint32_t *vals, int64_t n, int64_t N, const BcdAccumLayerIn &in, int nb_layers,
                                            const float *weights, float *layers, hipStream_t s)
{
    if (n <= 0 || nb_layers <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_accum_segments_layers, dim3(nblk(n, 256), (unsigned)nb_layers), dim3(256), 0, s, keys, vals, n, N, in, weights, layers);
    return hipGetLastError();
}

// ---- splatted add ---------------------------------------------------------------------------------------------------------------------
// cells of a tile's ring, and the largest number of samples the staging arrays of a workgroup can hold beside a ts x ts table
int bcd_splat_ring_cells(int nx, int ny) { return (SPLAT_TX + 2 * nx) * (SPLAT_TY + 2 * ny); }
int bcd_splat_max_staged(int ts) { return (int)((SPLAT_LDS_BYTES - splat_fixed_lds(ts)) / SPLAT_SAMPLE_BYTES); }

// filter: rx, ry, inv_rx, inv_ry; geom: ts, kx, ky, nx, ny (the definition in include/bcd_hip.h); T: the table on the device
hipError_t bcd_launch_splat_keys(const float *xy, int64_t n, int W, int H, const float *filter, const int *geom, const float *T, uint32_t *keys,
                                 uint32_t *vals, unsigned long long *dropped, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_accum_splat_keys, dim3(nblk(n, 256)), dim3(256), 0, s, xy, n, W, H, splat_filter(filter, geom), T, keys, vals, dropped);
    return hipGetLastError();
}

// cells: (W + 2 kx) * (H + 2 ky) pairs
hipError_t bcd_launch_splat_cells(const uint32_t *keys, int64_t n, int64_t NE, void *cells, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(cells, 0, (size_t)NE * sizeof(uint2), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_accum_splat_cells, dim3(nblk(n, 256)), dim3(256), 0, s, keys, n, (uint32_t)NE, (uint2 *)cells);
    return hipGetLastError();
}

// cap: samples the staging arrays hold (<= bcd_splat_max_staged); a tile whose ring holds more reads the sorted batch from global memory.
// layer: st is one layer's nine planes and rgb its colours (nbins, gamma and maxval are not used)
hipError_t bcd_launch_splat(const void *cells, const uint32_t *vals, const float *xy, const float *rgb, const float *weights, int W, int H,
                            const float *filter, const int *geom, const float *T, int cap, int nbins, float gamma, float maxval, float *st,
                            hipStream_t s, bool layer)
{
    const SplatFilter F = splat_filter(filter, geom);
    const int tiles_x = (W + SPLAT_TX - 1) / SPLAT_TX;
    const int64_t tiles = (int64_t)tiles_x * ((H + SPLAT_TY - 1) / SPLAT_TY);
    cap = std::max(0, std::min(cap, bcd_splat_max_staged(F.ts)));
    const size_t lds = splat_fixed_lds(F.ts) + (size_t)cap * SPLAT_SAMPLE_BYTES;
    if (layer)
        hipLaunchKernelGGL(k_accum_splat<true>, dim3((unsigned)tiles), dim3(256), lds, s, (const uint2 *)cells, vals, xy, rgb, weights, W, H, tiles_x,
                           F, T, cap, nbins, gamma, maxval, st);
    else
        hipLaunchKernelGGL(k_accum_splat<false>, dim3((unsigned)tiles), dim3(256), lds, s, (const uint2 *)cells, vals, xy, rgb, weights, W, H, tiles_x,
                           F, T, cap, nbins, gamma, maxval, st);
    return hipGetLastError();
}

hipError_t bcd_launch_accum_snapshot(const float *st, int64_t N, int D, float *ons, float *omean, float *ocov, float *ohist, hipStream_t s)
{
    hipLaunchKernelGGL(k_accum_snapshot, dim3(nblk(N, 64)), dim3(64), bcd_accum_snapshot_lds(D), s, st, N, D, ons, omean, ocov, ohist);
    return hipGetLastError();
}

hipError_t bcd_launch_accum_moments(const float *st, int64_t N, float *ons, float *omean, float *ocov, hipStream_t s)
{
    hipLaunchKernelGGL(k_accum_moments, dim3(nblk(N, 256)), dim3(256), 0, s, st, N, ons, omean, ocov);
    return hipGetLastError();
}

hipError_t bcd_launch_accum_snapshot_layers(const float *st, const float *layers, int64_t N, const BcdAccumLayerOut &out, int nb_layers, hipStream_t s)
{
    if (nb_layers <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_accum_snapshot_layers, dim3(nblk(N, 256), (unsigned)nb_layers), dim3(256), 0, s, st, layers, N, out);
    return hipGetLastError();
}

// ---- adaptive plan ------------------------------------------------------------------------------------------------------------------
size_t bcd_plan_red_bytes() { return sizeof(PlanRed); }

// the two scans' temporary storage for N pixels
hipError_t bcd_plan_scan_bytes(int64_t N, size_t *bytes)
{
    size_t a = 0, b = 0;
    rocprim::transform_iterator<const float *, PlanWeight, uint64_t> it((const float *)nullptr, PlanWeight{ nullptr, 0.f });
    hipError_t e = rocprim::inclusive_scan(nullptr, a, it, (uint64_t *)nullptr, (size_t)N, rocprim::plus<uint64_t>());
    if (e != hipSuccess) return e;
    e = rocprim::inclusive_scan(nullptr, b, (const int32_t *)nullptr, (int32_t *)nullptr, (size_t)N, rocprim::plus<int32_t>());
    *bytes = a > b ? a : b;
    return e;
}

// error pass -> C = inclusive scan of q -> capped counts -> their inclusive scan (ends) -> summary -> pixel list.  `red` must be zeroed
// before; Q, E and T stay on the device
hipError_t bcd_launch_accum_plan(const float *st, int64_t N, float eps, float min_samples, float tau, int K, int64_t B, uint64_t offset, float *err,
                                 int32_t *counts, int32_t *pixels, int64_t capacity, int64_t *summary, void *red, uint64_t *C, int32_t *ends,
                                 void *tmp, size_t tmp_bytes, hipStream_t s)
{
    PlanRed *r = (PlanRed *)red;
    const unsigned eblk = nblk(N, 256) < PLAN_ERROR_BLOCKS ? nblk(N, 256) : PLAN_ERROR_BLOCKS;
    hipLaunchKernelGGL(k_plan_error, dim3(eblk), dim3(256), 0, s, st, N, eps, min_samples, tau, err, r);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    rocprim::transform_iterator<const float *, PlanWeight, uint64_t> q(err, PlanWeight{ r, tau });
    size_t bytes = tmp_bytes;
    e = rocprim::inclusive_scan(tmp, bytes, q, C, (size_t)N, rocprim::plus<uint64_t>(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_plan_counts, dim3(nblk(N, 256)), dim3(256), 0, s, C, N, B, offset, K, counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    bytes = tmp_bytes;
    e = rocprim::inclusive_scan(tmp, bytes, (const int32_t *)counts, ends, (size_t)N, rocprim::plus<int32_t>(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_plan_summary, dim3(1), dim3(1), 0, s, r, ends, N, summary);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (B > 0) hipLaunchKernelGGL(k_plan_expand, dim3(nblk(N, 256)), dim3(256), 0, s, ends, N, pixels, capacity);
    return hipGetLastError();
}

// ---- merge ------------------------------------------------------------------------------------------------------------------------
// workgroups of 256 per CU in a merge grid: 8 fill the 8 wave slots of every SIMD
#define MERGE_BLOCKS_PER_CU 8

hipError_t bcd_launch_accum_merge(float *dst, const float *src, int64_t n, int num_cus, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    const uintptr_t a = (uintptr_t)dst & 15, b = (uintptr_t)src & 15;
    int64_t head = n, nvec = 0;
    if (a == b && (a & 3) == 0) {
        head = std::min<int64_t>(n, (int64_t)((16 - a) & 15) / 4);
        nvec = (n - head) / 4;
    }
    const int64_t work = std::max<int64_t>(nvec, n - 4 * nvec);
    const unsigned cap = (unsigned)std::max(1, num_cus) * MERGE_BLOCKS_PER_CU;
    hipLaunchKernelGGL(k_accum_merge, dim3(std::min(nblk(work, 256), cap)), dim3(256), 0, s, dst, src, n, head, nvec);
    return hipGetLastError();
}

hipError_t bcd_launch_accum_counter(unsigned long long *dst, const unsigned long long *src, unsigned long long add, int keep, hipStream_t s)
{
    hipLaunchKernelGGL(k_accum_counter, dim3(1), dim3(1), 0, s, dst, src, add, keep);
    return hipGetLastError();
}
