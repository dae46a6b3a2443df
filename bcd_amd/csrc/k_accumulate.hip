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
// (pixel, sample index) with a stable radix sort and walks each pixel's run in order.
#include <cstring> // (before rocprim: texture_cache_iterator.hpp uses memset)
#include <rocprim/rocprim.hpp>

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

enum { ACC_W = 0, ACC_W2 = 1, ACC_M = 2, ACC_C = 5, ACC_H = 11 };

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
        const float R = rgb[e * 3], G = rgb[e * 3 + 1], B = rgb[e * 3 + 2];
        const float w = weights ? weights[e] : 1.f;
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
    s.store(st, N, p);
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
        const float inv = 1.f / s.wsum;
        float mean[3];
        for (int i = 0; i < 3; ++i) { mean[i] = inv * s.m[i]; omean[p * 3 + i] = mean[i]; }
        float cv[6];
        for (int i = 0; i < 6; ++i) cv[i] = s.c[i] * inv;
        cv[0] -= mean[0] * mean[0]; cv[1] -= mean[1] * mean[1]; cv[2] -= mean[2] * mean[2];
        cv[3] -= mean[1] * mean[2]; cv[4] -= mean[0] * mean[2]; cv[5] -= mean[0] * mean[1];
        const float bias = 1.f / (1 - s.w2sum / (s.wsum * s.wsum));
        for (int i = 0; i < 6; ++i) ocov[p * 6 + i] = cv[i] * bias;
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

inline unsigned nblk(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

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

hipError_t bcd_launch_accum_snapshot(const float *st, int64_t N, int D, float *ons, float *omean, float *ocov, float *ohist, hipStream_t s)
{
    hipLaunchKernelGGL(k_accum_snapshot, dim3(nblk(N, 64)), dim3(64), bcd_accum_snapshot_lds(D), s, st, N, D, ons, omean, ocov, ohist);
    return hipGetLastError();
}
