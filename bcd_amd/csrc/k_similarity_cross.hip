// k_similarity_cross.hip -- similar-patch selection BETWEEN two frames: for every main pixel p of a frame, the main pixels q of
// a neighbouring frame of the sequence inside p's clipped window whose patch is within tau of p's patch.
//
// The distance is histogramPatchDistance -> pixelSummedHistogramDistance (src/core/DenoisingUnit.cpp:336-386) with the first patch read from the frame
// and the second from the neighbour, in the reference's operations: per patch offset, row-major, the sequential sum over the bins with b1 + b2 > 1 of
// (n2 b1 - n1 b2)^2 / (n1 n2 (b1 + b2)), n1 from the frame and n2 from the neighbour, integer bin counts, one IEEE division, NaN never similar.  The
// decomposition is that of k_similarity.hip:
//   d(p, q = p + delta) = (((T_delta(p + o0) + T_delta(p + o1)) + ...) / (float)(sum_o C_delta(p + o)),   o over the patch, row-major
//   T_delta(x) = the sequential-in-bin sum between pixel x of the frame and pixel x + delta of the neighbour, C_delta(x) its bin count.
// Between two frames T_delta(x) and T_-delta(x + delta) are different pixel pairs, so ALL (2b+1)^2 displacements are evaluated and there is no symmetric
// completion: plane k = (dl + b)(2b + 1) + (dc + b) is mask bit k.  Kernel 1 writes the planes, kernel 2 box-sums them straight into masks and counts.
// Compiled with -ffp-contract=off like k_similarity.hip: the membership test d <= tau is discrete.
#include "bcd_common.h"
#include <algorithm>
#include <atomic>

namespace {

constexpr int PX_TW = 64; // tile width
constexpr int PX_TH = 4;  // tile height (4 wavefronts per workgroup)
constexpr int PX_CW = 12; // widest span of column displacements served by one staged window

// LDS pixel stride (floats): D/4 odd keeps ds_read_b128 at a per-lane stride of D*4 bytes conflict-free (k_pairdist)
template <int D> struct PxStride { static constexpr int value = ((D / 4) % 2 == 1) ? D : D + 4; };

// ---------------------------------------------------------------------------------------------------
// kernel 1: pair-distance planes between two frames.  k_pairdist's exact form: one thread per pixel x of a 4x64 tile with its own histogram (frame A)
// in VGPRs; the neighbour's (frame B's) rows are staged through LDS once per displacement row dl and re-used for the displacements of that row.
// The compiler's IEEE division serves every operand (no range guard, no redo).
// ---------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void k_pairdist_cross(const float *__restrict__ histA, const float *__restrict__ nsA,
                                                         const float *__restrict__ histB, const float *__restrict__ nsB,
                                                         int W, int H, int b, float *__restrict__ T, uint8_t *__restrict__ Cn)
{
    constexpr int DS = PxStride<D>::value;
    constexpr int Q = D / 4;
    extern __shared__ float4 lds4[];
    // the displacements of a line are evaluated in chunks of at most PX_CW + 1 columns, each with its own staged column window of 64 + PX_CW pixels
    const int ncols = PX_TW + min(2 * b, PX_CW);
    float *lds_n = reinterpret_cast<float *>(lds4 + PX_TH * ncols * (DS / 4));

    // a wavefront covers a compact 16 x 4 pixel patch of the tile: neighbouring pixels in 2-D share their occupied bins (the wave-uniform skip below)
    const int lane_ = threadIdx.x & 63, wave_ = threadIdx.x >> 6;
    const int tx = (wave_ << 4) | (lane_ & 15), ty = lane_ >> 4;
    // the tile order of k_pairdist: workgroups that share an L2 get one contiguous band of tiles (speed only)
    int tile;
    {
        const int nt = gridDim.x * gridDim.y, id = blockIdx.y * gridDim.x + blockIdx.x;
        const int xcd = id & 7, k = id >> 3, q = nt >> 3, rem = nt & 7;
        tile = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + k;
    }
    const int col0 = (tile % gridDim.x) * PX_TW, row0 = (tile / gridDim.x) * PX_TH;
    const int c = col0 + tx, r = row0 + ty;
    const bool inside = (c < W) && (r < H);
    const size_t plane = (size_t)W * H;
    const size_t pix = (size_t)r * W + c;
    const int side = 2 * b + 1;

    float h1[D];
    float n1 = 1.f;
    {
        const float4 *src = reinterpret_cast<const float4 *>(histA) + (inside ? pix * Q : 0);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            float4 v = inside ? src[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            h1[4 * q] = v.x; h1[4 * q + 1] = v.y; h1[4 * q + 2] = v.z; h1[4 * q + 3] = v.w;
        }
        if (inside) n1 = nsA[pix];
    }

    for (int dl = -b; dl <= b; ++dl)
      for (int cbeg = -b; cbeg <= b; cbeg += PX_CW + 1) {
        const int cend = min(b, cbeg + PX_CW);
        __syncthreads();
        // stage the neighbour's rows row0+dl .. row0+dl+3, columns col0+cbeg .. col0+63+cend (zeros outside the image: their results are not written)
        const int npix = PX_TH * ncols;
        for (int i = threadIdx.x; i < npix * Q; i += 256) {
            int p = i / Q, q = i - p * Q;
            int lr = p / ncols, lc = p - lr * ncols;
            int gr = row0 + dl + lr, gc = col0 + cbeg + lc;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gr >= 0 && gr < H && gc >= 0 && gc < W) v = reinterpret_cast<const float4 *>(histB)[((size_t)gr * W + gc) * Q + q];
            lds4[p * (DS / 4) + q] = v;
        }
        for (int i = threadIdx.x; i < npix; i += 256) {
            int lr = i / ncols, lc = i - lr * ncols;
            int gr = row0 + dl + lr, gc = col0 + cbeg + lc;
            lds_n[i] = (gr >= 0 && gr < H && gc >= 0 && gc < W) ? nsB[(size_t)gr * W + gc] : 1.f;
        }
        __syncthreads();

        for (int dc = cbeg; dc <= cend; ++dc) {
            const float4 *nb = lds4 + (ty * ncols + tx + dc - cbeg) * (DS / 4);
            const float n2 = lds_n[ty * ncols + tx + dc - cbeg];
            const float n12 = n1 * n2;
            float sum = 0.f;
            int cnt = 0;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float4 v = nb[q];
                const float b2[4] = { v.x, v.y, v.z, v.w };
                float s[4];
                bool u[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { s[j] = h1[4 * q + j] + b2[j]; u[j] = s[j] > 1.f; } // DenoisingUnit.cpp:379
                // wave-uniform skip of a group of 4 bins that is empty for all 64 pixels of the wavefront (exact: skipped bins contribute nothing)
                if (__builtin_amdgcn_ballot_w64(u[0] || u[1] || u[2] || u[3]) != 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float diff = n2 * h1[4 * q + j] - n1 * b2[j];
                        const float term = diff * diff / (n12 * s[j]);
                        sum = u[j] ? sum + term : sum; // bins in order: the reference's sequential sum
                        cnt += u[j] ? 1 : 0;
                    }
                }
            }
            const int nc = c + dc, nr = r + dl;
            if (inside && nc >= 0 && nc < W && nr >= 0 && nr < H) {
                const size_t di = (size_t)((dl + b) * side + (dc + b));
                T[di * plane + pix] = sum;
                Cn[di * plane + pix] = (uint8_t)cnt;
            }
        }
      }
}

// generic-depth variant (any D <= 255): both histograms read from global memory, no staging.
__global__ __launch_bounds__(256) void k_pairdist_cross_generic(const float *__restrict__ histA, const float *__restrict__ nsA,
                                                                 const float *__restrict__ histB, const float *__restrict__ nsB,
                                                                 int W, int H, int D, int b, float *__restrict__ T, uint8_t *__restrict__ Cn)
{
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= W || r >= H) return;
    const size_t plane = (size_t)W * H, pix = (size_t)r * W + c;
    const float *h1 = histA + pix * D;
    const float n1 = nsA[pix];
    size_t di = 0;
    for (int dl = -b; dl <= b; ++dl)
        for (int dc = -b; dc <= b; ++dc, ++di) {
            int nc = c + dc, nr = r + dl;
            if (nc < 0 || nc >= W || nr < 0 || nr >= H) continue;
            size_t q = (size_t)nr * W + nc;
            const float *h2 = histB + q * D;
            float n2 = nsB[q], n12 = n1 * n2, sum = 0.f;
            int cnt = 0;
            for (int k = 0; k < D; ++k) {
                float b1 = h1[k], b2 = h2[k], s = b1 + b2;
                if (s <= 1.f) continue;
                ++cnt;
                float diff = n2 * b1 - n1 * b2;
                sum += diff * diff / (n12 * s);
            }
            T[di * plane + pix] = sum;
            Cn[di * plane + pix] = (uint8_t)cnt;
        }
}

// the patch distance of main pixel (r, c) to the neighbour's main pixel (r + dl, c + dc): the (2w+1)^2 plane entries in the reference's patch order,
// the counts as integers, one IEEE division (0 / 0 = NaN).  Both patches lie inside the image, so every entry read was written by kernel 1.
__device__ inline float cross_patch_distance(const float *__restrict__ T, const uint8_t *__restrict__ Cn, size_t base, int W, int w, int r, int c)
{
    float s = 0.f;
    int n = 0;
    for (int ol = -w; ol <= w; ++ol)
        for (int oc = -w; oc <= w; ++oc) {
            const size_t idx = base + (size_t)(r + ol) * W + (c + oc);
            s += T[idx];
            n += Cn[idx];
        }
    return s / (float)n;
}

// ---------------------------------------------------------------------------------------------------
// kernel 2: cross masks and counts.  One thread per pixel (adjacent lanes read adjacent plane entries); the window is PixelWindow(center, radius b,
// border w) (DenoisingUnit.cpp:200-203), clipped, displacement (0, 0) included.  Pixels that are not main pixels get empty masks and count 0.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_masks_cross(const float *__restrict__ T, const uint8_t *__restrict__ Cn, int W, int H, int w, int b, float tau,
                                                     int words, uint32_t *__restrict__ mask, int32_t *__restrict__ count)
{
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= W || r >= H) return;
    const size_t plane = (size_t)W * H, pix = (size_t)r * W + c;
    const int side = 2 * b + 1, nbits = side * side;
    const bool is_main = (r >= w && r <= H - 1 - w && c >= w && c <= W - 1 - w);
    int total = 0;
    for (int word = 0; word < words; ++word) {
        uint32_t m = 0;
        if (is_main) {
            for (int bit = 0; bit < 32; ++bit) {
                const int k = word * 32 + bit;
                if (k >= nbits) break;
                const int qr = r + k / side - b, qc = c + k % side - b;
                if (qr < w || qr > H - 1 - w || qc < w || qc > W - 1 - w) continue;
                const float d = cross_patch_distance(T, Cn, (size_t)k * plane, W, w, r, c);
                if (d <= tau) m |= 1u << bit; // NaN: not similar
            }
        }
        mask[pix * words + word] = m;
        total += __popc(m);
    }
    count[pix] = total;
}

// nsim += the cross count of one neighbour: |S| = |S_0| + sum_f |S_f|
__global__ void k_add_counts(int32_t *__restrict__ nsim, const int32_t *__restrict__ add, int64_t npix)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < npix) nsim[i] += add[i];
}

// debug / parity: raw cross distances of one main pixel to its window, +inf outside
__global__ void k_window_distances_cross(const float *__restrict__ T, const uint8_t *__restrict__ Cn, int W, int H, int w, int b, int r, int c,
                                         float *__restrict__ out)
{
    const int side = 2 * b + 1;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= side * side) return;
    const int qr = r + k / side - b, qc = c + k % side - b;
    float d = INFINITY;
    if (!(qr < w || qr > H - 1 - w || qc < w || qc > W - 1 - w)) d = cross_patch_distance(T, Cn, (size_t)k * (size_t)W * H, W, w, r, c);
    out[k] = d;
}

size_t pairdist_cross_lds_bytes(int D, int b)
{
    const int DS = ((D / 4) % 2 == 1) ? D : D + 4;
    return (size_t)PX_TH * (PX_TW + (2 * b < PX_CW ? 2 * b : PX_CW)) * (DS + 1) * sizeof(float);
}

} // namespace

// ---- launchers (called from bcd_temporal.hip) ---------------------------------------------------------
// T: (2b+1)^2 planes of W*H floats, Cn: as many planes of W*H bytes; entries whose neighbour pixel leaves the image are not written
hipError_t bcd_launch_pairdist_cross(const float *histA, const float *nsA, const float *histB, const float *nsB, int W, int H, int D, int b,
                                     float *T, uint8_t *Cn, hipStream_t st)
{
    dim3 grid((W + PX_TW - 1) / PX_TW, (H + PX_TH - 1) / PX_TH), block(256);
    const size_t lds = pairdist_cross_lds_bytes(D, b);
    const bool tiled = (D % 4 == 0) && lds <= 160 * 1024;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
#define BCD_PX_CASE(DD)                                                                                              \
    case DD: {                                                                                                       \
        static std::atomic<size_t> granted[64]; /* per instantiation and device: make the attribute call once per size */ \
        if (lds > 64 * 1024 && (dev < 0 || dev >= 64 || granted[dev].load() < lds)) {                                \
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pairdist_cross<DD>),                \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);               \
            if (e != hipSuccess) return e;                                                                           \
            if (dev >= 0 && dev < 64) granted[dev].store(lds);                                                       \
        }                                                                                                            \
        hipLaunchKernelGGL((k_pairdist_cross<DD>), grid, block, lds, st, histA, nsA, histB, nsB, W, H, b, T, Cn);    \
        return hipGetLastError();                                                                                    \
    }
    if (tiled) switch (D) {
        BCD_PX_CASE(60)
        BCD_PX_CASE(120)
        BCD_PX_CASE(36)
        BCD_PX_CASE(24)
        BCD_PX_CASE(12)
        default: break;
    }
#undef BCD_PX_CASE
    hipLaunchKernelGGL(k_pairdist_cross_generic, grid, block, 0, st, histA, nsA, histB, nsB, W, H, D, b, T, Cn);
    return hipGetLastError();
}

hipError_t bcd_launch_masks_cross(const float *T, const uint8_t *Cn, int W, int H, int w, int b, float tau, uint32_t *mask, int32_t *count, hipStream_t st)
{
    const int side = 2 * b + 1, words = (side * side + 31) / 32;
    hipLaunchKernelGGL(k_masks_cross, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, st, T, Cn, W, H, w, b, tau, words, mask, count);
    return hipGetLastError();
}

hipError_t bcd_launch_add_counts(int32_t *nsim, const int32_t *add, int64_t npix, hipStream_t st)
{
    hipLaunchKernelGGL(k_add_counts, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, nsim, add, npix);
    return hipGetLastError();
}

hipError_t bcd_launch_window_distances_cross(const float *T, const uint8_t *Cn, int W, int H, int w, int b, int r, int c, float *out, hipStream_t st)
{
    const int n = (2 * b + 1) * (2 * b + 1);
    hipLaunchKernelGGL(k_window_distances_cross, dim3((n + 63) / 64), dim3(64), 0, st, T, Cn, W, H, w, b, r, c, out);
    return hipGetLastError();
}
