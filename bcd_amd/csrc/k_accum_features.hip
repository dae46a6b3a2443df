// k_accum_features.hip -- auxiliary feature channels of the persistent device SamplesAccumulator (bcd_hip_accum_*_features, include/bcd_hip.h;
// DESIGN.md section 10, "Features"): per channel k two running sums, s1_k = sum w x_k and s2_k = sum w x_k x_k, beside the beauty's state,
// and their snapshot into the two images of a bcd_hip_guide -- the weighted mean and the variance of that mean.
//
// Planes: 2 F planes of N = W*H floats in a buffer of their own, plane-major, channel after channel (s1_0, s2_0, s1_1, ...).  The weight sum
// and the squared-weight sum are the beauty's (planes ACC_W and ACC_W2 of the state); only the snapshot reads them.
//
// One thread owns one pixel and all of its F channels, the kernels are templated on F so that the 2 F sums live in registers; a plane read
// or written by a wavefront is 64 consecutive floats.  A sample's F channels are F consecutive floats, read as float4 / float2 / float (V)
// where F and the buffer's address allow: the launcher decides from the pointer, the values loaded are the same.  Every pixel's samples are
// applied by one thread in stream order with (w * x) and (w * x) * x, the operations of AccSums::add on m[0] and c[0] (-ffp-contract=off):
// channel k has the bits of the first colour channel of an accumulator fed x_k.  No float atomics.
#include <algorithm>
#include <type_traits>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "accum_kernels.h"
#include "bcd_common.h"

namespace {

// F consecutive floats at p (V floats per load; the launcher has checked the alignment)
template <int F, int V>
__device__ inline void feat_read(const float *__restrict__ p, float x[F])
{
    static_assert(F % V == 0, "vector width must divide the channel count");
    if constexpr (V == 4) {
#pragma unroll
        for (int k = 0; k < F; k += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(p + k);
            x[k] = v.x; x[k + 1] = v.y; x[k + 2] = v.z; x[k + 3] = v.w;
        }
    } else if constexpr (V == 2) {
#pragma unroll
        for (int k = 0; k < F; k += 2) {
            const float2 v = *reinterpret_cast<const float2 *>(p + k);
            x[k] = v.x; x[k + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < F; ++k) x[k] = p[k];
    }
}

template <int F, int V>
__device__ inline void feat_write(float *__restrict__ p, const float x[F])
{
    static_assert(F % V == 0, "vector width must divide the channel count");
    if constexpr (V == 4) {
#pragma unroll
        for (int k = 0; k < F; k += 4) *reinterpret_cast<float4 *>(p + k) = make_float4(x[k], x[k + 1], x[k + 2], x[k + 3]);
    } else if constexpr (V == 2) {
#pragma unroll
        for (int k = 0; k < F; k += 2) *reinterpret_cast<float2 *>(p + k) = make_float2(x[k], x[k + 1]);
    } else {
#pragma unroll
        for (int k = 0; k < F; ++k) p[k] = x[k];
    }
}

template <int F>
struct FeatSums {
    float s1[F], s2[F];
    __device__ void load(const float *__restrict__ ft, int64_t N, int64_t p)
    {
#pragma unroll
        for (int k = 0; k < F; ++k) { s1[k] = ft[(2 * k) * N + p]; s2[k] = ft[(2 * k + 1) * N + p]; }
    }
    __device__ void store(float *__restrict__ ft, int64_t N, int64_t p) const
    {
#pragma unroll
        for (int k = 0; k < F; ++k) { ft[(2 * k) * N + p] = s1[k]; ft[(2 * k + 1) * N + p] = s2[k]; }
    }
    // the m[0] and c[0] lines of AccSums::add for every channel
    __device__ void add(const float x[F], float w)
    {
#pragma unroll
        for (int k = 0; k < F; ++k) {
            s1[k] += w * x[k];
            s2[k] += w * x[k] * x[k];
        }
    }
};

// (a) dense add: pixels [p0, p0 + npix), k samples each.  A 1-sample pass moves 4 F B of sample, 4 B of weight and the 2 F planes twice:
// 20 F + 4 B per pixel; the weight sums are not read
template <int F, int V>
__global__ __launch_bounds__(256) void k_feat_dense(const float *__restrict__ feat, const float *__restrict__ weights, int64_t p0, int64_t npix,
                                                    int64_t N, int k, float *__restrict__ ft)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= npix) return;
    const int64_t p = p0 + q;
    FeatSums<F> s;
    s.load(ft, N, p);
    const float *fp = feat + q * k * F;
    const float *wp = weights ? weights + q * k : nullptr;
    for (int i = 0; i < k; ++i) {
        float x[F];
        feat_read<F, V>(fp + (int64_t)i * F, x);
        s.add(x, wp ? wp[i] : 1.f);
    }
    s.store(ft, N, p);
}

// (b) scattered add on the chunk's sorted keys and values (k_accum_keys and the sort of the beauty's add): one thread per run of equal keys
// walks the run -- the pixel's samples in stream order
template <int F, int V>
__global__ __launch_bounds__(256) void k_feat_segments(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, int64_t n, int64_t N,
                                                       const float *__restrict__ feat, const float *__restrict__ weights, float *__restrict__ ft)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t key = keys[i];
    if ((int64_t)key >= N || (i > 0 && keys[i - 1] == key)) return;
    const int64_t p = key;
    FeatSums<F> s;
    s.load(ft, N, p);
    for (int64_t j = i; j < n && keys[j] == key; ++j) {
        const int64_t e = vals[j];
        float x[F];
        feat_read<F, V>(feat + e * F, x);
        s.add(x, weights ? weights[e] : 1.f);
    }
    s.store(ft, N, p);
}

// (b') splatted add on the chunk's cells and sorted values: the tile, ring and merge of k_accum_splat (accum_kernels.h) with the features
// and the weight as payload.  Staged: position, x, y, weight and F channel arrays of `cap` entries, 4 (4 + F) B per sample
#define FEAT_SAMPLE_BYTES(F) (4 * (4 + (F)))

template <bool STAGED, int F, int V>
struct SplatFeatureRuns : SplatKeys<STAGED> {
    const float *s_w, *s_f;                           // LDS staging arrays (channel k of slot i: s_f[k * cap + i])
    int cap;
    const float *feat, *weights;                      // the batch itself
    __device__ void feature(uint32_t i, float x[F], float &w) const
    {
        if (STAGED) {
#pragma unroll
            for (int k = 0; k < F; ++k) x[k] = s_f[k * cap + i];
            w = s_w[i];
        } else {
            const int64_t e = this->vals[i];
            feat_read<F, V>(feat + e * F, x);
            w = weights ? weights[e] : 1.f;
        }
    }
};

template <bool STAGED, int F, int V>
__device__ inline void splat_feature_pixel(const SplatFeatureRuns<STAGED, F, V> &S, const SplatFilter &Fl, const float *T, int rc0, int RW, int col,
                                           int line, int64_t p, int64_t N, float *__restrict__ ft)
{
    FeatSums<F> s;
    bool loaded = false;
    splat_merge(S, Fl, T, rc0, RW, col, line, [&](uint32_t idx, float f) {
        if (!loaded) { s.load(ft, N, p); loaded = true; }
        float x[F], w;
        S.feature(idx, x, w);
        s.add(x, w * f);
    });
    if (loaded) s.store(ft, N, p); // (a pixel without contributions does not touch its planes)
}

// dynamic LDS: the table (ts * ts), g0[SPLAT_RING_MAX], b0[SPLAT_RING_MAX + 4], then 4 + F staging arrays of `cap` entries
template <int F, int V>
__global__ __launch_bounds__(256) void k_feat_splat(const uint2 *__restrict__ cells, const uint32_t *__restrict__ vals, const float *__restrict__ xy,
                                                    const float *__restrict__ feat, const float *__restrict__ weights, int W, int H, int tiles_x,
                                                    SplatFilter Fl, const float *__restrict__ T, int cap, float *__restrict__ ft)
{
    extern __shared__ float lds_f[];
    const int t = threadIdx.x, tt = Fl.ts * Fl.ts;
    float *s_T = lds_f;
    uint32_t *s_g0 = (uint32_t *)(lds_f + tt), *s_b0 = s_g0 + SPLAT_RING_MAX, *s_pos = s_b0 + SPLAT_RING_MAX + 4;
    float *s_x = (float *)(s_pos + cap), *s_y = s_x + cap, *s_w = s_y + cap, *s_f = s_w + cap;
    const int px0 = (int)(blockIdx.x % (unsigned)tiles_x) * SPLAT_TX, py0 = (int)(blockIdx.x / (unsigned)tiles_x) * SPLAT_TY;
    const int RW = SPLAT_TX + 2 * Fl.nx, RC = RW * (SPLAT_TY + 2 * Fl.ny);
    const uint32_t total = splat_ring_load(cells, T, Fl, W, H, px0, py0, s_T, s_g0, s_b0);
    if (total == 0) return;
    const bool staged = total <= (uint32_t)cap; // (uniform over the workgroup)
    if (staged) {
        for (uint32_t j = t; j < total; j += 256) {
            const int64_t e = splat_slot_sample(s_g0, s_b0, RC, vals, j);
            float x[F];
            feat_read<F, V>(feat + e * F, x);
            s_pos[j] = (uint32_t)e;
            s_x[j] = xy[2 * e]; s_y[j] = xy[2 * e + 1];
            s_w[j] = weights ? weights[e] : 1.f;
#pragma unroll
            for (int k = 0; k < F; ++k) s_f[k * cap + j] = x[k];
        }
        __syncthreads();
    }
    const int lx = t % SPLAT_TX, ly = t / SPLAT_TX, col = px0 + lx, line = py0 + ly;
    if (col >= W || line >= H) return;
    const int64_t N = (int64_t)W * H, p = (int64_t)line * W + col;
    const int rc0 = ly * RW + lx;
    if (staged) {
        const SplatFeatureRuns<true, F, V> S = { { s_g0, s_b0, s_pos, s_x, s_y, vals, xy }, s_w, s_f, cap, feat, weights };
        splat_feature_pixel(S, Fl, s_T, rc0, RW, col, line, p, N, ft);
    } else {
        const SplatFeatureRuns<false, F, V> S = { { s_g0, s_b0, s_pos, s_x, s_y, vals, xy }, s_w, s_f, cap, feat, weights };
        splat_feature_pixel(S, Fl, s_T, rc0, RW, col, line, p, N, ft);
    }
}

// (c) snapshot: the weighted mean of every channel and the variance of that mean, pixel-interleaved (the two images of a bcd_hip_guide).
// mean and v are the mean[0] and cov[0] lines of acc_statistics (k_accumulate.hip) on (wsum, w2sum, s1, s2); vm = v * (w2sum / wsum^2) is
// v / n for unit weights; what is not a positive number -- negative round-off, NaN (one sample: 0 * inf; no sample), a zero of either sign
// -- is stored as +0.  Reads 8 + 8 F B and writes 4 F (VAR = false) or 8 F B per pixel; state and planes are read only.
template <int F, int V, bool VAR>
__global__ __launch_bounds__(256) void k_feat_snapshot(const float *__restrict__ st, const float *__restrict__ ft, int64_t N,
                                                       float *__restrict__ omean, float *__restrict__ ovar)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const float wsum = st[ACC_W * N + p], w2sum = st[ACC_W2 * N + p];
    FeatSums<F> s;
    s.load(ft, N, p);
    const float inv = 1.f / wsum;
    const float r = w2sum / (wsum * wsum);
    const float bias = 1.f / (1 - r);
    float mean[F], var[F];
#pragma unroll
    for (int k = 0; k < F; ++k) {
        mean[k] = inv * s.s1[k];
        float cv = s.s2[k] * inv;
        cv -= mean[k] * mean[k];
        const float v = cv * bias;
        const float vm = v * r;
        var[k] = vm > 0.f ? vm : 0.f;
    }
    feat_write<F, V>(omean + p * F, mean);
    if constexpr (VAR) feat_write<F, V>(ovar + p * F, var);
}

// the widest load of F consecutive floats that every sample of a buffer at p allows: samples are F floats apart
int feat_vector(const void *p, int F)
{
    const uintptr_t a = (uintptr_t)p;
    if (F % 4 == 0 && a % 16 == 0) return 4;
    if (F % 2 == 0 && a % 8 == 0) return 2;
    return 1;
}

template <int N>
using IC = std::integral_constant<int, N>;

// fn(IC<F>, IC<V>) with V the widest of 4, 2, 1 that is <= vec and divides F
template <int F, class FN>
void feat_with_vector(int vec, FN &fn)
{
    if constexpr (F % 4 == 0)
        if (vec >= 4) { fn(IC<F>(), IC<4>()); return; }
    if constexpr (F % 2 == 0)
        if (vec >= 2) { fn(IC<F>(), IC<2>()); return; }
    fn(IC<F>(), IC<1>());
}

template <class FN>
hipError_t feat_dispatch(int F, int vec, FN fn)
{
    switch (F) {
    case 1: feat_with_vector<1>(vec, fn); break;
    case 2: feat_with_vector<2>(vec, fn); break;
    case 3: feat_with_vector<3>(vec, fn); break;
    case 4: feat_with_vector<4>(vec, fn); break;
    case 5: feat_with_vector<5>(vec, fn); break;
    case 6: feat_with_vector<6>(vec, fn); break;
    case 7: feat_with_vector<7>(vec, fn); break;
    case 8: feat_with_vector<8>(vec, fn); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace

// feat: [pixel of the pass][k][F]; ft: the 2 F planes
hipError_t bcd_launch_feat_dense(const float *feat, int F, const float *weights, int64_t p0, int64_t npix, int64_t N, int k, float *ft, hipStream_t s)
{
    if (npix <= 0) return hipSuccess;
    return feat_dispatch(F, feat_vector(feat, F), [&](auto f, auto v) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_feat_dense<decltype(f)::value, decltype(v)::value>), dim3(nblk(npix, 256)), dim3(256), 0, s, feat, weights,
                           p0, npix, N, k, ft);
    });
}

// keys, vals: the chunk's sorted keys and values; feat: [sample of the chunk][F]
hipError_t bcd_launch_feat_segments(const uint32_t *keys, const uint32_t *vals, int64_t n, int64_t N, const float *feat, int F, const float *weights,
                                    float *ft, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    return feat_dispatch(F, feat_vector(feat, F), [&](auto f, auto v) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_feat_segments<decltype(f)::value, decltype(v)::value>), dim3(nblk(n, 256)), dim3(256), 0, s, keys, vals, n, N,
                           feat, weights, ft);
    });
}

// the largest number of samples the staging arrays of a feature splat workgroup hold beside a ts x ts table, within the LDS of k_accum_splat
int bcd_feat_splat_max_staged(int ts, int F) { return (int)((SPLAT_LDS_BYTES - splat_fixed_lds(ts)) / FEAT_SAMPLE_BYTES(F)); }

// the arguments of bcd_launch_splat with the features for the colours; cap is cut to bcd_feat_splat_max_staged: a tile whose ring holds
// more reads the sorted batch from global memory, to the same bits
hipError_t bcd_launch_feat_splat(const void *cells, const uint32_t *vals, const float *xy, const float *feat, int F, const float *weights, int W, int H,
                                 const float *filter, const int *geom, const float *T, int cap, float *ft, hipStream_t s)
{
    const SplatFilter Fl = splat_filter(filter, geom);
    const int tiles_x = (W + SPLAT_TX - 1) / SPLAT_TX;
    const int64_t tiles = (int64_t)tiles_x * ((H + SPLAT_TY - 1) / SPLAT_TY);
    cap = std::max(0, std::min(cap, bcd_feat_splat_max_staged(Fl.ts, F)));
    const size_t lds = splat_fixed_lds(Fl.ts) + (size_t)cap * FEAT_SAMPLE_BYTES(F);
    return feat_dispatch(F, feat_vector(feat, F), [&](auto f, auto v) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_feat_splat<decltype(f)::value, decltype(v)::value>), dim3((unsigned)tiles), dim3(256), lds, s,
                           (const uint2 *)cells, vals, xy, feat, weights, W, H, tiles_x, Fl, T, cap, ft);
    });
}

// st: the accumulator's state (its weight sums are read); omean, ovar: W*H*F floats each, ovar may be null
hipError_t bcd_launch_feat_snapshot(const float *st, const float *ft, int64_t N, int F, float *omean, float *ovar, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    const int vec = std::min(feat_vector(omean, F), ovar ? feat_vector(ovar, F) : 4);
    return feat_dispatch(F, vec, [&](auto f, auto v) {
        constexpr int FF = decltype(f)::value, VV = decltype(v)::value;
        if (ovar) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_feat_snapshot<FF, VV, true>), dim3(nblk(N, 256)), dim3(256), 0, s, st, ft, N, omean, ovar);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_feat_snapshot<FF, VV, false>), dim3(nblk(N, 256)), dim3(256), 0, s, st, ft, N, omean, ovar);
    });
}
