// k_spike.hip -- the spike prefilter as a source map and a gather: k_spike_map records which pixel the filter would copy
// into every pixel, k_spike_apply gathers any number of images of one depth through that map.  The decision is bcd_spike_source (bcd_spike.h),
// the function k_spike (k_pointwise.hip) filters with, compiled with the same flags: the map is k_spike's `src`, nothing else.
#include "bcd_common.h"
#include "bcd_spike.h"

namespace {

// One thread per pixel: 3 x 9 colours in, one int32 out.  moved (may be null): pixels with map[p] != p, one integer atomic per wavefront.
__global__ __launch_bounds__(256) void k_spike_map(const float *__restrict__ col, int W, int H, uint32_t npix, float factor, int32_t *__restrict__ map,
                                                   int32_t *__restrict__ moved)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    bool mv = false;
    if (p < npix) {
        const int l = (int)(p / (uint32_t)W), c = (int)(p - (uint32_t)l * (uint32_t)W);
        const uint32_t src = (uint32_t)bcd_spike_source(col, W, H, l, c, factor); // (pixel indices fit 31 bits: checked by the host entry points)
        map[p] = (int32_t)src;
        mv = src != p;
    }
    if (moved) { // (no lane has left: the ballot sees the whole wavefront)
        const unsigned long long b = __ballot(mv);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(moved, (int32_t)__popcll(b));
    }
}

// dst[p * depth + z] = src[map[p] * depth + z], out of place, for the images of blockIdx.y.  A workgroup serves a 64-pixel strip of a line
// (blockIdx.x = line * strips + strip): its 64 map entries go through LDS and the 64 lanes then move the 64 pixels' values as contiguous runs,
// the form k_spike uses for its copies.  A map entry outside [0, npix) reads as the pixel itself -- a caller's bad map cannot fault the device.
// DEPTH > 0: the depth at compile time (1, 3, 6: the divisions fold); 0: `depth` at run time.  vec16: bit k set = images k (source and
// destination) are 16-byte aligned; with a depth that is a multiple of 4 they move as 16-byte accesses.
template <int DEPTH>
__global__ __launch_bounds__(64) void k_spike_apply(BcdSpikeTable t, const int32_t *__restrict__ map, int W, int strips, uint32_t npix, int depth_rt, uint32_t vec16)
{
    __shared__ unsigned int s_src[64];
    const int depth = DEPTH > 0 ? DEPTH : depth_rt;
    const int l = (int)(blockIdx.x / (uint32_t)strips), c0 = (int)(blockIdx.x - (uint32_t)l * (uint32_t)strips) * 64;
    const int ncols = min(64, W - c0);
    const size_t row_base = (size_t)l * W + c0; // first destination pixel of the workgroup
    if ((int)threadIdx.x < ncols) {
        const uint32_t p = (uint32_t)row_base + threadIdx.x, m = (uint32_t)map[p];
        s_src[threadIdx.x] = m < npix ? m : p;
    }
    __syncthreads();
    const float *__restrict__ src = t.src[blockIdx.y];
    float *__restrict__ dst = t.dst[blockIdx.y];
    if ((depth & 3) == 0 && ((vec16 >> blockIdx.y) & 1u)) {
        const int Q = depth >> 2;
        const float4 *s4 = reinterpret_cast<const float4 *>(src);
        float4 *d4 = reinterpret_cast<float4 *>(dst);
        for (int e = threadIdx.x; e < ncols * Q; e += 64) { const int px = e / Q; d4[row_base * Q + e] = s4[(size_t)s_src[px] * Q + (e - px * Q)]; }
    } else
        for (int e = threadIdx.x; e < ncols * depth; e += 64) { const int px = e / depth; dst[row_base * depth + e] = src[(size_t)s_src[px] * depth + (e - px * depth)]; }
}

} // namespace

// the source map of a W x H colour image (W, H >= 3, W * H < 2^31); d_moved (may be null) is zeroed and receives the number of moved pixels
hipError_t bcd_launch_spike_map(const float *col, int W, int H, float factor, int32_t *map, int32_t *d_moved, hipStream_t st)
{
    const uint32_t npix = (uint32_t)W * (uint32_t)H;
    if (d_moved) {
        hipError_t e = hipMemsetAsync(d_moved, 0, sizeof(int32_t), st);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_spike_map, dim3((npix + 255u) / 256u), dim3(256), 0, st, col, W, H, npix, factor, map, d_moved);
    return hipGetLastError();
}

// n images (1 .. BCD_SPIKE_MAX_IMAGES) of one depth gathered through the map in one launch
hipError_t bcd_launch_spike_apply(const BcdSpikeTable &t, int n, const int32_t *map, int W, int H, int depth, hipStream_t st)
{
    if (n < 1 || n > BCD_SPIKE_MAX_IMAGES || depth < 1) return hipErrorInvalidValue;
    const int strips = (W + 63) / 64;
    const uint32_t npix = (uint32_t)W * (uint32_t)H;
    uint32_t vec16 = 0; // (the public entry point takes any device pointers -- a view into a larger buffer may be 4-byte aligned only: those take the scalar copies)
    for (int k = 0; k < n; ++k)
        if ((((uintptr_t)t.src[k] | (uintptr_t)t.dst[k]) & 15) == 0) vec16 |= 1u << k;
    const dim3 grid((uint32_t)strips * (uint32_t)H, n), block(64);
    switch (depth) {
    case 1: hipLaunchKernelGGL(k_spike_apply<1>, grid, block, 0, st, t, map, W, strips, npix, depth, vec16); break;
    case 3: hipLaunchKernelGGL(k_spike_apply<3>, grid, block, 0, st, t, map, W, strips, npix, depth, vec16); break;
    case 6: hipLaunchKernelGGL(k_spike_apply<6>, grid, block, 0, st, t, map, W, strips, npix, depth, vec16); break;
    default: hipLaunchKernelGGL(k_spike_apply<0>, grid, block, 0, st, t, map, W, strips, npix, depth, vec16); break;
    }
    return hipGetLastError();
}
