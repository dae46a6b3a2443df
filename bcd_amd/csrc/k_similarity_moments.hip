// k_similarity_moments.hip -- pair-distance planes from per-pixel means and covariances: a second producer of the T / C
// planes that k_masks and k_fwd_masks_w1* (k_similarity.hip) box-sum into the similarity masks, for frames whose producer keeps a running mean and
// variance per pixel and no sample histogram.
//
// For pixels x and y = x + delta, channels k = 0, 1, 2 in order, from s = 0.f, n = 0 (m: the guide's colours, v_k: the xx, yy, zz entries of its
// per-pixel covariances -- what bcd_hip_pixel_cov returns --, eps: the variance floor):
//     d = m_k(x) - m_k(y)
//     q = (v_k(x) + v_k(y)) + eps
//     if (q > 0.f) { s = s + (d * d) / q; n = n + 1; }        (IEEE division; a NaN q is not counted)
//     T_delta(x) = s, C_delta(x) = n
// Every operation is commutative in (x, y) up to the sign of d, which the square removes: T / C are bitwise symmetric (T_delta(x) == T_-delta(x+delta)),
// so the half plane of displacements suffices, as for the histograms.  The planes have the layout of k_pairdist: fp32 T, byte C, delta-major
// (bcd_delta_index), entries whose neighbour leaves the image not written.
// This file is compiled with -ffp-contract=off (the membership test d <= tau is discrete and tests/moments_ref.py states these operations in
// NumPy float32) and with the correctly rounded fp32 division: no reciprocal approximation, no binary16 plane.
#include "bcd_common.h"

namespace {

constexpr int PM_TW = 64; // tile width (one wavefront per tile line)
constexpr int PM_TH = 4;  // tile height (4 wavefronts per workgroup)

// One thread per pixel of a 64 x 4 tile.  The tile's six values per pixel with its halo -- b lines below, b columns either side: the half plane
// looks down and sideways only -- are staged through LDS once, one plane per value (consecutive lanes read consecutive words), and serve all
// bcd_delta_count(b) displacements.  5 bytes are written per (pixel, displacement) and 24 bytes read per pixel: the kernel is bound by its stores.
__global__ __launch_bounds__(256) void k_pairdist_moments(const float *__restrict__ m, const float *__restrict__ P, int W, int H, int b, float eps,
                                                           float *__restrict__ T, uint8_t *__restrict__ Cn)
{
    extern __shared__ float lds[];
    const int ncols = PM_TW + 2 * b, nrows = PM_TH + b, np = ncols * nrows;
    const int col0 = blockIdx.x * PM_TW, row0 = blockIdx.y * PM_TH;
    for (int i = threadIdx.x; i < np; i += 256) {
        const int lr = i / ncols, lc = i - lr * ncols;
        const int gr = row0 + lr, gc = col0 - b + lc;
        float v[6] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
        if (gr < H && gc >= 0 && gc < W) {
            const size_t p = (size_t)gr * W + gc;
            v[0] = m[p * 3]; v[1] = m[p * 3 + 1]; v[2] = m[p * 3 + 2];
            v[3] = P[p * 6]; v[4] = P[p * 6 + 1]; v[5] = P[p * 6 + 2]; // xx, yy, zz
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) lds[k * np + i] = v[k];
    }
    __syncthreads();

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = col0 + tx, r = row0 + ty;
    const bool inside = c < W && r < H;
    const size_t plane = (size_t)W * H, pix = (size_t)r * W + c;
    const int own = ty * ncols + tx + b;
    float m1[3], v1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { m1[k] = lds[k * np + own]; v1[k] = lds[(3 + k) * np + own]; }

    int didx = 0;
    for (int dl = 0; dl <= b; ++dl)
        for (int dc = (dl == 0) ? 0 : -b; dc <= b; ++dc, ++didx) {
            const int nb = own + dl * ncols + dc;
            float s = 0.f;
            int n = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float d = m1[k] - lds[k * np + nb];
                const float q = (v1[k] + lds[(3 + k) * np + nb]) + eps;
                if (q > 0.f) { s = s + (d * d) / q; n = n + 1; }
            }
            const int nc = c + dc, nr = r + dl;
            if (inside && nc >= 0 && nc < W && nr < H) {
                T[(size_t)didx * plane + pix] = s;
                Cn[(size_t)didx * plane + pix] = (uint8_t)n;
            }
        }
}

} // namespace

// T: bcd_delta_count(b) * W * H floats, Cn: as many bytes (the exact-path planes bcd_launch_masks reads with ap == nullptr); b <= 15 (check_params)
hipError_t bcd_launch_pairdist_moments(const float *colors, const float *pixcov, int W, int H, int b, float var_floor, float *T, uint8_t *Cn, hipStream_t st)
{
    if (W <= 0 || H <= 0 || b < 0 || b > 15) return hipErrorInvalidValue;
    const dim3 grid((W + PM_TW - 1) / PM_TW, (H + PM_TH - 1) / PM_TH);
    const size_t lds = (size_t)6 * (PM_TW + 2 * b) * (PM_TH + b) * sizeof(float); // b = 15: 42 864 bytes
    hipLaunchKernelGGL(k_pairdist_moments, grid, dim3(256), lds, st, colors, pixcov, W, H, b, var_floor, T, Cn);
    return hipGetLastError();
}
