// k_similarity_guide.hip -- the feature gate of the similar-patch selection: pair-distance planes from auxiliary feature buffers
// (albedo, normal, depth, object id, ...), a third producer of the T / C planes that k_masks and k_fwd_masks_w1* (k_similarity.hip) box-sum into
// masks, and the kernel that ANDs such feature masks into a selection's masks.
//
// For pixels x and y = x + delta, channels k = 0 .. F-1 in order, from s = 0.f, n = 0 (f: the features, v: the variance of the pixel's feature mean or
// absent, eps_k: the floor of channel k):
//     d = f_k(x) - f_k(y)
//     q = (v_k(x) + v_k(y)) + eps_k                        (v absent: q = 0.f + eps_k)
//     if (q > 0.f) { t = (d * d) / q;  if (t == t) { s = s + t; n = n + 1; } }
//     T_delta(x) = s, C_delta(x) = n
// A NaN term is skipped (depth inf against depth inf), an infinite term is counted (inf against a finite depth).  Every operation is commutative in
// (x, y) up to the sign of d, which the square removes: T / C are bitwise symmetric, so the half plane of displacements suffices.  The planes have the
// layout of k_pairdist: fp32 T, byte C, delta-major (bcd_delta_index), entries whose neighbour leaves the image not written.
// This file is compiled with -ffp-contract=off and the correctly rounded fp32 division (tests/guide_ref.py states these operations in NumPy float32).
#include "bcd_common.h"

#include <atomic>

namespace {

constexpr int PG_TW = 64; // tile width (one wavefront per tile line)
constexpr int PG_TH = 4;  // tile height (4 wavefronts per workgroup)
constexpr size_t PG_LDS_LIMIT = 160 * 1024;

struct GuideFloors { float e[BCD_GUIDE_MAX_CHANNELS]; };

// One thread per pixel of a 64 x 4 tile, as k_pairdist_moments: the tile's F (2F with variances) values per pixel with its halo -- b lines below, b
// columns either side -- are staged through LDS once, one plane per value (consecutive lanes read consecutive words), and serve all
// bcd_delta_count(b) displacements; the thread's own values stay in registers.  5 bytes are written per (pixel, displacement).
template <int F, bool VAR>
__global__ __launch_bounds__(256) void k_pairdist_guide(const float *__restrict__ f, const float *__restrict__ v, int W, int H, int b, GuideFloors eps,
                                                         float *__restrict__ T, uint8_t *__restrict__ Cn)
{
    extern __shared__ float lds[];
    constexpr int NV = VAR ? 2 * F : F;
    const int ncols = PG_TW + 2 * b, nrows = PG_TH + b, np = ncols * nrows;
    const int col0 = blockIdx.x * PG_TW, row0 = blockIdx.y * PG_TH;
    for (int i = threadIdx.x; i < np; i += 256) {
        const int lr = i / ncols, lc = i - lr * ncols;
        const int gr = row0 + lr, gc = col0 - b + lc;
        float x[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) x[k] = 0.f;
        if (gr < H && gc >= 0 && gc < W) {
            const size_t p = ((size_t)gr * W + gc) * F;
#pragma unroll
            for (int k = 0; k < F; ++k) {
                x[k] = f[p + k];
                if (VAR) x[F + k] = v[p + k];
            }
        }
#pragma unroll
        for (int k = 0; k < NV; ++k) lds[k * np + i] = x[k];
    }
    __syncthreads();

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = col0 + tx, r = row0 + ty;
    const bool inside = c < W && r < H;
    const size_t plane = (size_t)W * H, pix = (size_t)r * W + c;
    const int own = ty * ncols + tx + b;
    float f1[F], v1[F];
#pragma unroll
    for (int k = 0; k < F; ++k) { f1[k] = lds[k * np + own]; v1[k] = VAR ? lds[(F + k) * np + own] : 0.f; }

    int didx = 0;
    for (int dl = 0; dl <= b; ++dl)
        for (int dc = (dl == 0) ? 0 : -b; dc <= b; ++dc, ++didx) {
            const int nb = own + dl * ncols + dc;
            float s = 0.f;
            int n = 0;
#pragma unroll
            for (int k = 0; k < F; ++k) {
                const float d = f1[k] - lds[k * np + nb];
                const float q = (VAR ? v1[k] + lds[(F + k) * np + nb] : 0.f) + eps.e[k];
                if (q > 0.f) {
                    const float t = (d * d) / q;
                    if (t == t) { s = s + t; n = n + 1; }
                }
            }
            const int nc = c + dc, nr = r + dl;
            if (inside && nc >= 0 && nc < W && nr < H) {
                T[(size_t)didx * plane + pix] = s;
                Cn[(size_t)didx * plane + pix] = (uint8_t)n;
            }
        }
}

// mask[p][j] &= gate[p][j] for the `words` words of pixel p, nsim[p] = the set bits that remain.  One thread per pixel, V words per load and store
// (V divides `words`, so a pixel's row starts on a V-word boundary).
template <int V> struct WordVec;
template <> struct WordVec<1> { typedef uint32_t type; };
template <> struct WordVec<2> { typedef uint2 type; };
template <> struct WordVec<4> { typedef uint4 type; };

__device__ inline uint32_t and_popc(uint32_t &m, uint32_t g) { m &= g; return __popc(m); }
__device__ inline uint32_t and_popc(uint2 &m, uint2 g) { m.x &= g.x; m.y &= g.y; return __popc(m.x) + __popc(m.y); }
__device__ inline uint32_t and_popc(uint4 &m, uint4 g)
{
    m.x &= g.x; m.y &= g.y; m.z &= g.z; m.w &= g.w;
    return __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w);
}

template <int V>
__global__ __launch_bounds__(256) void k_gate_masks(uint32_t *__restrict__ mask, const uint32_t *__restrict__ gate, int32_t *__restrict__ nsim, uint32_t npix, int words)
{
    typedef typename WordVec<V>::type vec;
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= npix) return;
    const int nv = words / V;
    vec *m = reinterpret_cast<vec *>(mask) + (size_t)p * nv;
    const vec *g = reinterpret_cast<const vec *>(gate) + (size_t)p * nv;
    uint32_t n = 0;
    for (int j = 0; j < nv; ++j) {
        vec x = m[j];
        n += and_popc(x, g[j]);
        m[j] = x;
    }
    nsim[p] = (int32_t)n;
}

// x[i] = x[i] * a (the variances of a pyramid level: the average of four, times 0.25f)
__global__ __launch_bounds__(256) void k_scale_values(float *__restrict__ x, float a, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] = x[i] * a;
}

typedef void (*pairdist_guide_fn)(const float *, const float *, int, int, int, GuideFloors, float *, uint8_t *);

template <bool VAR> pairdist_guide_fn pairdist_guide_kernel(int F)
{
    switch (F) {
    case 1: return k_pairdist_guide<1, VAR>;
    case 2: return k_pairdist_guide<2, VAR>;
    case 3: return k_pairdist_guide<3, VAR>;
    case 4: return k_pairdist_guide<4, VAR>;
    case 5: return k_pairdist_guide<5, VAR>;
    case 6: return k_pairdist_guide<6, VAR>;
    case 7: return k_pairdist_guide<7, VAR>;
    case 8: return k_pairdist_guide<8, VAR>;
    }
    return nullptr;
}

size_t pairdist_guide_lds(int F, bool var, int b) { return (size_t)(var ? 2 * F : F) * (PG_TW + 2 * b) * (PG_TH + b) * sizeof(float); }

} // namespace

// Can k_pairdist_guide be launched for F channels (with variances or not) at search radius b on the current device?  F = 8 with variances needs
// 48.6 KB of LDS at b = 6, 90 KB at b = 12 and 114 KB at b = 15: above 64 KiB the kernel's dynamic-LDS limit is raised, once per kernel and
// device, to the 160 KiB a gfx950 CU has.  No launch is made: callers ask before any device work.
hipError_t bcd_pairdist_guide_launchable(int F, int has_var, int b)
{
    if (F < 1 || F > BCD_GUIDE_MAX_CHANNELS || b < 0 || b > 15) return hipErrorInvalidValue;
    const size_t lds = pairdist_guide_lds(F, has_var != 0, b);
    if (lds <= 64 * 1024) return hipSuccess;
    if (lds > PG_LDS_LIMIT) return hipErrorInvalidValue; // (F = 8 with variances at b = 15 is 114 304 B: nothing check_params admits gets here)
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    static std::atomic<int> granted[64][2][BCD_GUIDE_MAX_CHANNELS + 1]; // per device and instantiation: make the attribute call once
    if (dev >= 0 && dev < 64 && granted[dev][has_var != 0][F].load() != 0) return hipSuccess;
    const pairdist_guide_fn k = has_var ? pairdist_guide_kernel<true>(F) : pairdist_guide_kernel<false>(F);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PG_LDS_LIMIT);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) granted[dev][has_var != 0][F].store(1);
    return hipSuccess;
}

// T: bcd_delta_count(b) * W * H floats, Cn: as many bytes (the exact-path planes bcd_launch_masks reads with ap == nullptr); features W*H*F floats,
// variances the same or null; floors: F host floats
hipError_t bcd_launch_pairdist_guide(const float *features, const float *variances, int F, const float *floors, int W, int H, int b, float *T, uint8_t *Cn,
                                     hipStream_t st)
{
    if (W <= 0 || H <= 0 || !features || !floors) return hipErrorInvalidValue;
    const hipError_t e = bcd_pairdist_guide_launchable(F, variances != nullptr, b);
    if (e != hipSuccess) return e;
    GuideFloors eps = {};
    for (int k = 0; k < F; ++k) eps.e[k] = floors[k];
    const dim3 grid((W + PG_TW - 1) / PG_TW, (H + PG_TH - 1) / PG_TH);
    const size_t lds = pairdist_guide_lds(F, variances != nullptr, b);
    const pairdist_guide_fn k = variances ? pairdist_guide_kernel<true>(F) : pairdist_guide_kernel<false>(F);
    hipLaunchKernelGGL(k, grid, dim3(256), lds, st, features, variances, W, H, b, eps, T, Cn);
    return hipGetLastError();
}

// mask, gate: W*H rows of ((2b+1)^2 + 31) / 32 words; nsim: W*H counts (rewritten for every pixel)
hipError_t bcd_launch_gate_masks(uint32_t *mask, const uint32_t *gate, int32_t *nsim, int W, int H, int b, hipStream_t st)
{
    const int64_t npix = (int64_t)W * H;
    if (W <= 0 || H <= 0 || b < 0 || b > 15 || npix >= (int64_t)1 << 31) return hipErrorInvalidValue;
    const int side = 2 * b + 1, words = (side * side + 31) / 32;
    const dim3 grid((unsigned)((npix + 255) / 256));
    if (words % 4 == 0 && (((uintptr_t)mask | (uintptr_t)gate) & 15) == 0) hipLaunchKernelGGL(k_gate_masks<4>, grid, dim3(256), 0, st, mask, gate, nsim, (uint32_t)npix, words);
    else if (words % 2 == 0 && (((uintptr_t)mask | (uintptr_t)gate) & 7) == 0) hipLaunchKernelGGL(k_gate_masks<2>, grid, dim3(256), 0, st, mask, gate, nsim, (uint32_t)npix, words);
    else hipLaunchKernelGGL(k_gate_masks<1>, grid, dim3(256), 0, st, mask, gate, nsim, (uint32_t)npix, words);
    return hipGetLastError();
}

hipError_t bcd_launch_scale_inplace(float *x, float a, int64_t n, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    if (n >= ((int64_t)1 << 31) * 256) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_scale_values, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, a, n);
    return hipGetLastError();
}
