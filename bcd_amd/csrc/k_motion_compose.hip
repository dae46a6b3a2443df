// k_motion_compose.hip -- two motion fields composed into one ("Sequences with motion"; bcd_hip_compose_motion).
//
// a is the field frame t -> frame u, b the field frame u -> frame v in frame-u pixel order, out the field t -> v; each is W*H*2 floats, (dx, dy) per pixel, in
// the convention of k_warp.hip.  Per pixel p = (l, c):
//   (dx1, dy1) = a(p); p is BROKEN when dx1 or dy1 is not finite or |.| >= 2^24, or when q = (l + rintf(dy1), c + rintf(dx1)) lies outside the image;
//   otherwise (dx2, dy2) = b(q), and p is broken when these are not finite or |.| >= 2^24;
//   otherwise sx = rintf(dx1) + rintf(dx2), sy likewise, as int32, and p is broken when |sx| or |sy| >= 2^24.
// A broken pixel stores (NaN, NaN), any other ((float)sx, (float)sy): the output is integer-valued, so the rounding of the warp that reads it changes nothing,
// and warp(warp(X, b), a) == warp(X, out) bit for bit with validity valid_a(p) AND valid_b(q(p)).  Whether p + (sy, sx) lies inside the image is the warp's
// own rule.
//   k_motion_compose<VEC>   one thread per pixel: its own vector, one dependent gather from b, one store.  VEC: every field is 8-byte aligned and a vector is
//                           one 8-byte access; otherwise (a view one float into a buffer) two 4-byte accesses -- the pointer is never reinterpreted.
// No LDS, no float arithmetic beyond rintf and the conversions.
#include "bcd_common.h"
#include "bcd_launch.h"

namespace {

constexpr int COMPOSE_BLOCK = 256;
constexpr float MOTION_LIMIT = 16777216.f; // 2^24, as k_warp.hip

template <bool VEC>
__device__ inline float2 load_vector(const float *__restrict__ f, size_t pix)
{
    if constexpr (VEC) return reinterpret_cast<const float2 *>(f)[pix];
    return make_float2(f[2 * pix], f[2 * pix + 1]);
}

template <bool VEC>
__global__ __launch_bounds__(COMPOSE_BLOCK) void k_motion_compose(const float *__restrict__ a, const float *__restrict__ b, int W, int H, float *__restrict__ out)
{
    const size_t pix = (size_t)blockIdx.x * COMPOSE_BLOCK + threadIdx.x;
    if (pix >= (size_t)W * H) return;
    const int l = (int)((uint32_t)pix / (uint32_t)W), c = (int)((uint32_t)pix - (uint32_t)l * (uint32_t)W); // (W * H < 2^30: the launcher's callers)
    const float nan = __builtin_nanf("");
    float2 o = make_float2(nan, nan);
    const float2 v1 = load_vector<VEC>(a, pix);
    if (fabsf(v1.x) < MOTION_LIMIT && fabsf(v1.y) < MOTION_LIMIT) { // (NaN and the infinities fail the comparison)
        const int rx1 = (int)rintf(v1.x), ry1 = (int)rintf(v1.y);   // (|.| <= 2^24: exact as int, no overflow with W, H < 2^30)
        const int sc = c + rx1, sl = l + ry1;
        if (sc >= 0 && sc < W && sl >= 0 && sl < H) {
            const float2 v2 = load_vector<VEC>(b, (size_t)sl * W + sc);
            if (fabsf(v2.x) < MOTION_LIMIT && fabsf(v2.y) < MOTION_LIMIT) {
                const int sx = rx1 + (int)rintf(v2.x), sy = ry1 + (int)rintf(v2.y); // (|.| <= 2^25)
                if (abs(sx) < (1 << 24) && abs(sy) < (1 << 24)) o = make_float2((float)sx, (float)sy);
            }
        }
    }
    if constexpr (VEC) {
        reinterpret_cast<float2 *>(out)[pix] = o;
    } else {
        out[2 * pix] = o.x;
        out[2 * pix + 1] = o.y;
    }
}

inline bool aligned8(const void *p) { return ((uintptr_t)p & 7) == 0; }

} // namespace

// a, b, out: W*H*2 floats each, W*H < 2^30, out overlapping neither input
hipError_t bcd_launch_motion_compose(const float *a, const float *b, int W, int H, float *out, hipStream_t st)
{
    if (W <= 0 || H <= 0 || !a || !b || !out || (int64_t)W * H >= (1ll << 30)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(((size_t)W * H + COMPOSE_BLOCK - 1) / COMPOSE_BLOCK)), block(COMPOSE_BLOCK);
    if (aligned8(a) && aligned8(b) && aligned8(out))
        hipLaunchKernelGGL((k_motion_compose<true>), grid, block, 0, st, a, b, W, H, out);
    else
        hipLaunchKernelGGL((k_motion_compose<false>), grid, block, 0, st, a, b, W, H, out);
    return hipGetLastError();
}
