// k_spike_inplace.hip -- the gather through a source map IN PLACE ("In place"): after the call every image holds at pixel p the
// values it held before the call at pixel m(p), m(p) = map[p] inside [0, npix) and p otherwise (the rule of k_spike_apply).  A map has chains, cycles
// and fan-out, so no pixel may be written before every pixel that reads it has been read: the moved pixels (m(p) != p) are compacted into a list of
// (destination, source) pairs, k_spike_stage<false> copies every listed pixel's SOURCE values of every image into a staging buffer, and -- behind a
// kernel boundary on the stream -- k_spike_stage<true> copies the staging rows to the destinations.  Only moved pixels are touched.  The list's
// order varies from run to run (one atomic per workgroup); row i of the staging buffer belongs to entry i in both kernels, so the result does not.
#include "bcd_common.h"

namespace {

__device__ __forceinline__ uint32_t effective_source(const int32_t *__restrict__ map, uint32_t p, uint32_t npix)
{
    const uint32_t m = (uint32_t)map[p];
    return m < npix ? m : p;
}

// A workgroup of the two list kernels serves SPIKE_CHUNK consecutive pixels in SPIKE_ITERS rounds of 256: its wavefronts count their moved pixels with one
// ballot per round, the four counts meet in LDS, and ONE integer atomic per workgroup goes to the global word -- 507 of them on a 1080p frame.  (One atomic
// per wavefront on one word, the form k_spike_map counts with, costs 0.3 ms at 1080p when most wavefronts hold a moved pixel: docs/EXPERIMENTS.md section 33.)
constexpr int SPIKE_ITERS = 16;
constexpr uint32_t SPIKE_CHUNK = 256u * SPIKE_ITERS;

// the moved pixels of this wavefront's share of the chunk (uniform over the wavefront: no lane leaves before a ballot)
__device__ __forceinline__ int chunk_wave_count(const int32_t *__restrict__ map, uint32_t npix)
{
    int cnt = 0;
    for (int it = 0; it < SPIKE_ITERS; ++it) {
        const uint32_t p = (blockIdx.x * SPIKE_ITERS + it) * 256u + threadIdx.x;
        const bool mv = p < npix && effective_source(map, p, npix) != p;
        cnt += (int)__popcll(__ballot(mv));
    }
    return cnt;
}

// count[0] += pixels with m(p) != p
__global__ __launch_bounds__(256) void k_spike_moved_count(const int32_t *__restrict__ map, uint32_t npix, int32_t *__restrict__ count)
{
    __shared__ int s_wave[4];
    const int cnt = chunk_wave_count(map, npix);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        if (total) atomicAdd(count, total);
    }
}

// list[cursor ...] = (p, m(p)) of every moved pixel: the workgroup takes its run of entries with one atomic, a wavefront its part of the run from the counts
// in LDS, a lane its place from the ballot of its round (the map is read a second time, from cache).  An entry beyond `capacity` is dropped (the list was
// sized from k_spike_moved_count on the same map: there is none)
__global__ __launch_bounds__(256) void k_spike_compact(const int32_t *__restrict__ map, uint32_t npix, int32_t *__restrict__ cursor, int2 *__restrict__ list,
                                                       uint32_t capacity)
{
    __shared__ int s_wave[4];
    __shared__ int s_base;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int cnt = chunk_wave_count(map, npix);
    if (lane == 0) s_wave[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        s_base = total ? atomicAdd(cursor, total) : 0;
    }
    __syncthreads();
    uint32_t at = (uint32_t)s_base;
    for (uint32_t w = 0; w < wave; ++w) at += (uint32_t)s_wave[w];
    for (int it = 0; it < SPIKE_ITERS; ++it) {
        const uint32_t p = (blockIdx.x * SPIKE_ITERS + it) * 256u + threadIdx.x;
        const uint32_t m = p < npix ? effective_source(map, p, npix) : p;
        const bool mv = m != p;
        const unsigned long long b = __ballot(mv);
        if (mv) {
            const uint32_t i = at + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
            if (i < capacity) list[i] = make_int2((int)p, (int)m);
        }
        at += (uint32_t)__popcll(b);
    }
}

// BACK false: stage row i = the values of pixel list[i].y (the source); BACK true: pixel list[i].x (the destination) = stage row i.  A workgroup serves
// 64 list entries of the image blockIdx.y: their pixel indices go through LDS and the 64 lanes move the 64 pixels' values as contiguous runs of the
// staging buffer, the form of k_spike_apply.  The staging rows of image k start t.stage_off[k] floats in (a multiple of 4).  vec16: bit k set = image
// k is 16-byte aligned; with a depth that is a multiple of 4 it moves as 16-byte accesses.
template <bool BACK>
__global__ __launch_bounds__(64) void k_spike_stage(BcdSpikeInplaceTable t, const int2 *__restrict__ list, uint32_t moved, float *__restrict__ stage,
                                                    unsigned long long vec16)
{
    __shared__ unsigned int s_px[64];
    const uint32_t i0 = blockIdx.x * 64u;
    const int n = (int)min(64u, moved - i0);
    if ((int)threadIdx.x < n) { const int2 e = list[i0 + threadIdx.x]; s_px[threadIdx.x] = (unsigned int)(BACK ? e.x : e.y); }
    __syncthreads();
    const int k = blockIdx.y, depth = t.depth[k];
    float *img = t.img[k];
    float *st = stage + t.stage_off[k] + (size_t)i0 * depth;
    if ((depth & 3) == 0 && ((vec16 >> k) & 1ull)) {
        const int Q = depth >> 2;
        float4 *i4 = reinterpret_cast<float4 *>(img), *s4 = reinterpret_cast<float4 *>(st);
        for (int e = threadIdx.x; e < n * Q; e += 64) {
            const int px = e / Q;
            const size_t at = (size_t)s_px[px] * Q + (e - px * Q);
            if (BACK) i4[at] = s4[e]; else s4[e] = i4[at];
        }
    } else
        for (int e = threadIdx.x; e < n * depth; e += 64) {
            const int px = e / depth;
            const size_t at = (size_t)s_px[px] * depth + (e - px * depth);
            if (BACK) img[at] = st[e]; else st[e] = img[at];
        }
}

} // namespace

// d_count is zeroed and receives the number of pixels with m(p) != p
hipError_t bcd_launch_spike_moved_count(const int32_t *map, uint32_t npix, int32_t *d_count, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(d_count, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_spike_moved_count, dim3((npix + SPIKE_CHUNK - 1u) / SPIKE_CHUNK), dim3(256), 0, st, map, npix, d_count);
    return hipGetLastError();
}

// the (destination, source) pairs of the moved pixels into list[0 .. capacity); d_cursor is zeroed and ends as their number
hipError_t bcd_launch_spike_compact(const int32_t *map, uint32_t npix, int32_t *d_cursor, int2 *list, uint32_t capacity, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(d_cursor, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_spike_compact, dim3((npix + SPIKE_CHUNK - 1u) / SPIKE_CHUNK), dim3(256), 0, st, map, npix, d_cursor, list, capacity);
    return hipGetLastError();
}

// the two copies of the in-place gather over list[0 .. moved), moved >= 1: n images (1 .. BCD_SPIKE_INPLACE_MAX_IMAGES), each of its own depth; `stage`
// is 16-byte aligned and holds bcd_spike_stage_floats() floats, which also fills t.stage_off
size_t bcd_spike_stage_floats(BcdSpikeInplaceTable &t, int n, uint32_t moved)
{
    size_t off = 0;
    for (int k = 0; k < n; ++k) {
        t.stage_off[k] = off;
        off += ((size_t)moved * (size_t)t.depth[k] + 3) & ~(size_t)3;
    }
    return off;
}

hipError_t bcd_launch_spike_stage(const BcdSpikeInplaceTable &t, int n, const int2 *list, uint32_t moved, float *stage, hipStream_t st)
{
    if (n < 1 || n > BCD_SPIKE_INPLACE_MAX_IMAGES || moved < 1) return hipErrorInvalidValue;
    unsigned long long vec16 = 0; // (the public entry point takes any device pointers: a view that is 4-byte aligned only takes the scalar copies)
    for (int k = 0; k < n; ++k) {
        if (t.depth[k] < 1 || t.depth[k] > BCD_SPIKE_INPLACE_MAX_DEPTH) return hipErrorInvalidValue;
        if (((uintptr_t)t.img[k] & 15) == 0) vec16 |= 1ull << k;
    }
    const dim3 grid((moved + 63u) / 64u, n), block(64);
    hipLaunchKernelGGL(k_spike_stage<false>, grid, block, 0, st, t, list, moved, stage, vec16);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_spike_stage<true>, grid, block, 0, st, t, list, moved, stage, vec16); // (the kernel boundary: every source is staged before a pixel is written)
    return hipGetLastError();
}
