// k_warp.hip -- neighbour frames reprojected into the frame's pixel grid by a motion field ("Motion").
//
// A motion field is W*H*2 floats, (dx, dy) per pixel of frame t: pixel (l, c) of frame t shows what pixel (l + ry, c + rx) of the neighbour shows,
// rx = rintf(dx), ry = rintf(dy), round to nearest even.  The pixel is VALID when dx and dy are finite, |dx|, |dy| < 2^24 and the source pixel lies inside
// the image.  A valid pixel of the warped neighbour takes the source pixel's values bit for bit (nothing is interpolated, so every statistic of a sample
// survives), an invalid one is +0.0f in every image.  A NULL field is zero motion.
//   k_warp_frame<D>      colours, sample counts, histograms, covariances of one neighbour and the validity byte
//   k_warp_layers        the colours and covariances of L layers of one neighbour and the validity byte
//   k_warp_features<F>   the feature image of a neighbour's guide (F floats per pixel) and, when it has one, the variance image, and the validity byte
//   k_valid_down         validity of the next pyramid level: every child the reducers read (k_pointwise.hip: 2l, 2l + 1 x 2c, 2c + 1) is valid
//   k_valid_patch        pvalid(q) = AND of valid(q + o) over the patch, 0 where q is not a main pixel
//   k_masks_gate_valid   bit delta of the cross mask of main pixel p is cleared unless pvalid(p + delta); the new |S_f|
// The gather kernels serve 256 consecutive pixels per workgroup: a lane reads the motion vector of its own pixel ONCE and leaves the source index in LDS;
// every image is then moved as one flat run of elements (16 bytes per lane for the histograms with D % 4 == 0), so that the stores of a wavefront are
// contiguous whatever the sources are.  The source addresses are wave-divergent by nature.
#include "bcd_common.h"
#include "bcd_launch.h"

namespace {

constexpr int WARP_BLOCK = 256;
constexpr uint32_t NO_SOURCE = 0xffffffffu;

// linear index of the source pixel of pixel (l, c), NO_SOURCE for an invalid pixel
__device__ inline uint32_t warp_source(const float *__restrict__ mv, size_t pix, int l, int c, int W, int H)
{
    float dx = 0.f, dy = 0.f;
    if (mv) { dx = mv[2 * pix]; dy = mv[2 * pix + 1]; }
    if (!(fabsf(dx) < 16777216.f && fabsf(dy) < 16777216.f)) return NO_SOURCE; // (NaN and the infinities fail the comparison)
    const int sc = c + (int)rintf(dx), sl = l + (int)rintf(dy);                    // (|.| <= 2^24: exact as int, no overflow with W, H < 2^30)
    if (sc < 0 || sc >= W || sl < 0 || sl >= H) return NO_SOURCE;
    return (uint32_t)sl * (uint32_t)W + (uint32_t)sc;
}

// the source table of the workgroup's pixels [base, base + n) and their validity bytes
__device__ inline void warp_sources(const float *__restrict__ mv, int W, int H, size_t base, int n, uint32_t *s_src, uint8_t *__restrict__ valid)
{
    const int t = threadIdx.x;
    if (t < n) {
        const size_t pix = base + t;
        const int l = (int)((uint32_t)pix / (uint32_t)W), c = (int)((uint32_t)pix - (uint32_t)l * (uint32_t)W); // (W * H < 2^32: check_params)
        const uint32_t s = warp_source(mv, pix, l, c, W, H);
        s_src[t] = s;
        valid[pix] = s != NO_SOURCE ? 1 : 0;
    }
    __syncthreads();
}

// E floats per pixel of the workgroup's n pixels as one flat run: out[base * E + i] for i in [0, n * E)
template <int E>
__device__ inline void warp_move(const float *__restrict__ in, float *__restrict__ out, const uint32_t *s_src, size_t base, int n)
{
    for (int i = threadIdx.x; i < n * E; i += WARP_BLOCK) {
        const int p = i / E, e = i - p * E;
        const uint32_t s = s_src[p];
        out[base * E + i] = s != NO_SOURCE ? in[(size_t)s * E + e] : 0.f;
    }
}

// D > 0: D % 4 == 0 and 16-byte aligned histogram images, moved as float4; D == 0: any depth `depth`, moved element by element
template <int D>
__global__ __launch_bounds__(WARP_BLOCK) void k_warp_frame(const float *__restrict__ col, const float *__restrict__ ns, const float *__restrict__ hist,
                                                           const float *__restrict__ cov, const float *__restrict__ mv, int W, int H, int depth,
                                                           float *__restrict__ ocol, float *__restrict__ ons, float *__restrict__ ohist, float *__restrict__ ocov,
                                                           uint8_t *__restrict__ valid)
{
    __shared__ uint32_t s_src[WARP_BLOCK];
    const size_t npix = (size_t)W * H, base = (size_t)blockIdx.x * WARP_BLOCK;
    const int n = (int)(npix - base < (size_t)WARP_BLOCK ? npix - base : (size_t)WARP_BLOCK);
    warp_sources(mv, W, H, base, n, s_src, valid);
    warp_move<3>(col, ocol, s_src, base, n);
    warp_move<1>(ns, ons, s_src, base, n);
    warp_move<6>(cov, ocov, s_src, base, n);
    if constexpr (D > 0) {
        constexpr int Q = D > 0 ? D / 4 : 1;
        const float4 *in4 = reinterpret_cast<const float4 *>(hist);
        float4 *out4 = reinterpret_cast<float4 *>(ohist);
        for (int i = threadIdx.x; i < n * Q; i += WARP_BLOCK) {
            const int p = i / Q, q = i - p * Q;
            const uint32_t s = s_src[p];
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (s != NO_SOURCE) v = in4[(size_t)s * Q + q];
            out4[base * Q + i] = v;
        }
    } else {
        for (int i = threadIdx.x; i < n * depth; i += WARP_BLOCK) { // (n <= 256, depth <= 255)
            const int p = i / depth, e = i - p * depth;
            const uint32_t s = s_src[p];
            ohist[base * depth + i] = s != NO_SOURCE ? hist[(size_t)s * depth + e] : 0.f;
        }
    }
}

// t.col / t.cov: the layers' images of the neighbour, t.ocol / t.ocov: their warped twins; the table travels by value and is indexed by the (uniform)
// loop counter, which the compiler serves with scalar loads from the kernel arguments
__global__ __launch_bounds__(WARP_BLOCK) void k_warp_layers(BcdWarpLayerTable t, int layers, const float *__restrict__ mv, int W, int H, uint8_t *__restrict__ valid)
{
    __shared__ uint32_t s_src[WARP_BLOCK];
    const size_t npix = (size_t)W * H, base = (size_t)blockIdx.x * WARP_BLOCK;
    const int n = (int)(npix - base < (size_t)WARP_BLOCK ? npix - base : (size_t)WARP_BLOCK);
    warp_sources(mv, W, H, base, n, s_src, valid);
    for (int k = 0; k < layers; ++k) {
        warp_move<3>(t.col[k], t.ocol[k], s_src, base, n);
        warp_move<6>(t.cov[k], t.ocov[k], s_src, base, n);
    }
}

// the gather of k_warp_layers for one (var, ovar null) or two images of F floats per pixel, F = 1 .. BCD_GUIDE_MAX_CHANNELS ("Features")
template <int F>
__global__ __launch_bounds__(WARP_BLOCK) void k_warp_features(const float *__restrict__ feat, const float *__restrict__ var, const float *__restrict__ mv, int W, int H,
                                                              float *__restrict__ ofeat, float *__restrict__ ovar, uint8_t *__restrict__ valid)
{
    __shared__ uint32_t s_src[WARP_BLOCK];
    const size_t npix = (size_t)W * H, base = (size_t)blockIdx.x * WARP_BLOCK;
    const int n = (int)(npix - base < (size_t)WARP_BLOCK ? npix - base : (size_t)WARP_BLOCK);
    warp_sources(mv, W, H, base, n, s_src, valid);
    warp_move<F>(feat, ofeat, s_src, base, n);
    if (var) warp_move<F>(var, ovar, s_src, base, n);
}

// validity of the (W / 2) x (H / 2) level from that of the W x H level
__global__ __launch_bounds__(256) void k_valid_down(const uint8_t *__restrict__ valid, int W, int H, uint8_t *__restrict__ out)
{
    const int w2 = W / 2, h2 = H / 2;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)w2 * h2) return;
    const int l = (int)(i / (uint32_t)w2), c = (int)(i - (size_t)l * w2);
    const size_t p = (size_t)(2 * l) * W + 2 * c; // (2l + 1 <= H - 1 and 2c + 1 <= W - 1 for every block of the level)
    out[i] = valid[p] & valid[p + 1] & valid[p + W] & valid[p + W + 1] & 1;
}

__global__ __launch_bounds__(256) void k_valid_patch(const uint8_t *__restrict__ valid, int W, int H, int w, uint8_t *__restrict__ pvalid)
{
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= W || r >= H) return;
    uint8_t v = 0;
    if (r >= w && r <= H - 1 - w && c >= w && c <= W - 1 - w) {
        v = 1;
        for (int ol = -w; ol <= w; ++ol)
            for (int oc = -w; oc <= w; ++oc) v &= valid[(size_t)(r + ol) * W + (c + oc)];
    }
    pvalid[(size_t)r * W + c] = v;
}

// One thread per pixel, the window clipped as in k_masks_cross: a bit survives when its pixel q = p + delta is a main pixel with pvalid(q).  Pixels that
// are not main pixels get empty masks and count 0, as k_masks_cross leaves them.
__global__ __launch_bounds__(256) void k_masks_gate_valid(uint32_t *__restrict__ mask, int32_t *__restrict__ count, const uint8_t *__restrict__ pvalid, int W, int H,
                                                          int w, int b, int words)
{
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= W || r >= H) return;
    const size_t pix = (size_t)r * W + c;
    const int side = 2 * b + 1, nbits = side * side;
    const bool is_main = (r >= w && r <= H - 1 - w && c >= w && c <= W - 1 - w);
    int total = 0;
    for (int word = 0; word < words; ++word) {
        uint32_t m = is_main ? mask[pix * words + word] : 0u, keep = 0u;
        while (m) {
            const int bit = __ffs(m) - 1;
            m &= m - 1;
            const int k = word * 32 + bit;
            if (k >= nbits) break;
            const int qr = r + k / side - b, qc = c + k % side - b;
            if (qr < w || qr > H - 1 - w || qc < w || qc > W - 1 - w) continue;
            if (pvalid[(size_t)qr * W + qc]) keep |= 1u << bit;
        }
        mask[pix * words + word] = keep;
        total += __popc(keep);
    }
    count[pix] = total;
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

} // namespace

// ---- launchers (called from bcd_temporal.hip and bcd_temporal_layers.hip) ------------------------------
hipError_t bcd_launch_warp_frame(const float *col, const float *ns, const float *hist, const float *cov, const float *mv, int W, int H, int D, float *ocol, float *ons,
                                 float *ohist, float *ocov, uint8_t *valid, hipStream_t st)
{
    const dim3 grid((unsigned)(((size_t)W * H + WARP_BLOCK - 1) / WARP_BLOCK)), block(WARP_BLOCK);
#define BCD_WARP_CASE(DD)                                                                                                                             \
    case DD: hipLaunchKernelGGL((k_warp_frame<DD>), grid, block, 0, st, col, ns, hist, cov, mv, W, H, D, ocol, ons, ohist, ocov, valid); return hipGetLastError();
    if (D % 4 == 0 && aligned16(hist) && aligned16(ohist)) switch (D) {
        BCD_WARP_CASE(60)
        BCD_WARP_CASE(120)
        BCD_WARP_CASE(36)
        BCD_WARP_CASE(24)
        BCD_WARP_CASE(12)
        default: break;
    }
#undef BCD_WARP_CASE
    hipLaunchKernelGGL((k_warp_frame<0>), grid, block, 0, st, col, ns, hist, cov, mv, W, H, D, ocol, ons, ohist, ocov, valid);
    return hipGetLastError();
}

hipError_t bcd_launch_warp_layers(const BcdWarpLayerTable &t, int layers, const float *mv, int W, int H, uint8_t *valid, hipStream_t st)
{
    hipLaunchKernelGGL(k_warp_layers, dim3((unsigned)(((size_t)W * H + WARP_BLOCK - 1) / WARP_BLOCK)), dim3(WARP_BLOCK), 0, st, t, layers, mv, W, H, valid);
    return hipGetLastError();
}

// feat, ofeat: W*H*F floats; var, ovar: the same, or both null
hipError_t bcd_launch_warp_features(const float *feat, const float *var, int F, const float *mv, int W, int H, float *ofeat, float *ovar, uint8_t *valid, hipStream_t st)
{
    if (W <= 0 || H <= 0 || !feat || !ofeat || !valid || (var == nullptr) != (ovar == nullptr)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(((size_t)W * H + WARP_BLOCK - 1) / WARP_BLOCK)), block(WARP_BLOCK);
#define BCD_WARPF_CASE(FF) \
    case FF: hipLaunchKernelGGL((k_warp_features<FF>), grid, block, 0, st, feat, var, mv, W, H, ofeat, ovar, valid); return hipGetLastError();
    switch (F) {
        BCD_WARPF_CASE(1)
        BCD_WARPF_CASE(2)
        BCD_WARPF_CASE(3)
        BCD_WARPF_CASE(4)
        BCD_WARPF_CASE(5)
        BCD_WARPF_CASE(6)
        BCD_WARPF_CASE(7)
        BCD_WARPF_CASE(8)
        default: break;
    }
#undef BCD_WARPF_CASE
    return hipErrorInvalidValue;
}

// out: (W / 2) x (H / 2) bytes; nothing to do (and nothing launched) when that level is empty
hipError_t bcd_launch_valid_down(const uint8_t *valid, int W, int H, uint8_t *out, hipStream_t st)
{
    const size_t n = (size_t)(W / 2) * (H / 2);
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_valid_down, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, valid, W, H, out);
    return hipGetLastError();
}

hipError_t bcd_launch_valid_patch(const uint8_t *valid, int W, int H, int w, uint8_t *pvalid, hipStream_t st)
{
    hipLaunchKernelGGL(k_valid_patch, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, st, valid, W, H, w, pvalid);
    return hipGetLastError();
}

hipError_t bcd_launch_masks_gate_valid(uint32_t *mask, int32_t *count, const uint8_t *pvalid, int W, int H, int w, int b, hipStream_t st)
{
    const int side = 2 * b + 1, words = (side * side + 31) / 32;
    hipLaunchKernelGGL(k_masks_gate_valid, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, st, mask, count, pvalid, W, H, w, b, words);
    return hipGetLastError();
}
