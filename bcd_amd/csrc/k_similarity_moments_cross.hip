// k_similarity_moments_cross.hip -- the cross-frame selection from per-pixel means and covariances ("Moments"): pair distances
// between the guide layer of a frame and that of a neighbour frame, for producers that keep a running mean and variance per pixel and no sample histogram.
//
// For pixel x of the frame and pixel y = x + delta of the neighbour, y inside the image, channels k = 0, 1, 2 in order, from s = 0.f, n = 0 (m0, mj: the
// guide layer's colours of the frame and of the neighbour, v0, vj: the xx, yy, zz entries of their per-pixel covariances -- what bcd_hip_pixel_cov returns
// for that frame's covariances and its own sample counts --, eps: the variance floor):
//     d = m0_k(x) - mj_k(y)
//     q = (v0_k(x) + vj_k(y)) + eps
//     if (q > 0.f) { s = s + (d * d) / q; n = n + 1; }        (IEEE division; a NaN q is not counted, a NaN or infinite term IS counted)
//     T_delta(x) = s, C_delta(x) = n
// This is k_pairdist_moments' term with the second operand read from the neighbour -- NOT the feature term of k_pairdist_guide_cross, which skips a NaN
// term.  Between two frames there is no symmetry, so all (2b+1)^2 displacements are evaluated; displacement k = (dl + b)(2b + 1) + (dc + b) is mask bit k.
// A neighbour that IS the frame gives, bit for bit, the in-frame masks of k_pairdist_moments + k_masks.
//   k_pairdist_moments_cross      the planes form: T / C planes in the layout of k_pairdist_cross, for k_masks_cross and k_window_distances_cross
//   k_masks_moments_cross_fused   the form without planes (w = 1, b <= 6): terms, patch sums, the test and the mask bits in one kernel
// Both forms perform the same float32 operations in the same order, so their masks and counts are bit-identical.
// This file is compiled with -ffp-contract=off and the correctly rounded fp32 division (tests/moments_cross_ref.py states these operations in NumPy float32).
#include "bcd_common.h"

namespace {

constexpr int PMX_TW = 64; // tile width (one wavefront per tile line)
constexpr int PMX_TH = 4;  // tile height (4 wavefronts per workgroup)
constexpr size_t PMX_LDS_LIMIT = 64 * 1024; // what a kernel may ask for without raising its dynamic-LDS attribute

// the six values of one pixel: colours, then the xx, yy, zz entries of its per-pixel covariance; zeros outside the image
__device__ inline void load_moments(const float *__restrict__ m, const float *__restrict__ P, int W, int H, int gr, int gc, float v[6])
{
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = 0.f;
    if (gr >= 0 && gr < H && gc >= 0 && gc < W) {
        const size_t p = (size_t)gr * W + gc;
        v[0] = m[p * 3]; v[1] = m[p * 3 + 1]; v[2] = m[p * 3 + 2];
        v[3] = P[p * 6]; v[4] = P[p * 6 + 1]; v[5] = P[p * 6 + 2]; // xx, yy, zz
    }
}

// the term of one pixel pair: a[0..2] / a[3..5] the frame's means / variances, the neighbour's read from its LDS planes (plane stride np) at index nb
__device__ inline void moments_term(const float a[6], const float *__restrict__ lds, int np, int nb, float eps, float *s_out, int *n_out)
{
    float s = 0.f;
    int n = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float d = a[k] - lds[k * np + nb];
        const float q = (a[3 + k] + lds[(3 + k) * np + nb]) + eps;
        if (q > 0.f) { s = s + (d * d) / q; n = n + 1; }
    }
    *s_out = s; *n_out = n;
}

// ---------------------------------------------------------------------------------------------------
// The planes form.  k_pairdist_moments' tile and thread layout: one thread per pixel of a 64 x 4 tile, the FRAME's six values in registers.  The NEIGHBOUR's
// six values are staged through LDS, one plane per value (consecutive lanes read consecutive words: no bank conflict), for a BAND of `nl` displacement lines
// at a time, as k_pairdist_guide_cross stages its features: the band [dl0, dl0 + nl) needs the neighbour's lines row0 + dl0 .. row0 + dl0 + nl + 2 and the
// columns col0 - b .. col0 + 63 + b.  3 divisions, a 4-byte and a 1-byte store per (pixel, displacement): the kernel is bound by its stores.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pairdist_moments_cross(const float *__restrict__ mA, const float *__restrict__ PA, const float *__restrict__ mB,
                                                                 const float *__restrict__ PB, int W, int H, int b, int nl, float eps, float *__restrict__ T,
                                                                 uint8_t *__restrict__ Cn)
{
    extern __shared__ float lds[];
    const int ncols = PMX_TW + 2 * b, nrows = PMX_TH + nl - 1, np = ncols * nrows;
    const int col0 = blockIdx.x * PMX_TW, row0 = blockIdx.y * PMX_TH;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = col0 + tx, r = row0 + ty;
    const bool inside = c < W && r < H;
    const size_t plane = (size_t)W * H, pix = (size_t)r * W + c;
    const int side = 2 * b + 1;

    float a[6];
    load_moments(mA, PA, W, H, r, c, a);

    for (int dl0 = -b; dl0 <= b; dl0 += nl) {
        const int dl1 = min(b, dl0 + nl - 1);
        __syncthreads(); // (the previous band has been read)
        for (int i = threadIdx.x; i < np; i += 256) {
            const int lr = i / ncols, lc = i - lr * ncols;
            float v[6];
            load_moments(mB, PB, W, H, row0 + dl0 + lr, col0 - b + lc, v);
#pragma unroll
            for (int k = 0; k < 6; ++k) lds[k * np + i] = v[k];
        }
        __syncthreads();

        for (int dl = dl0; dl <= dl1; ++dl) {
            const int nr = r + dl;
            const int line = (ty + dl - dl0) * ncols + tx + b;
            for (int dc = -b; dc <= b; ++dc) {
                float s;
                int n;
                moments_term(a, lds, np, line + dc, eps, &s, &n);
                const int nc = c + dc;
                if (inside && nc >= 0 && nc < W && nr >= 0 && nr < H) {
                    const size_t di = (size_t)((dl + b) * side + (dc + b));
                    T[di * plane + pix] = s;
                    Cn[di * plane + pix] = (uint8_t)n;
                }
            }
        }
    }
}

size_t pairdist_moments_cross_lds(int b, int nl) { return (size_t)6 * (PMX_TW + 2 * b) * (PMX_TH + nl - 1) * sizeof(float); }

// ---------------------------------------------------------------------------------------------------
// The form without planes, patch radius 1 and search radius 1 .. 6.  One workgroup owns a 64 x 4 tile of main-pixel candidates.  It stages, one plane per
// value, the frame's six values for the tile plus a halo of 1 (66 x 6 positions) and the neighbour's for the tile plus a halo of b + 1 (b = 6: 78 x 18
// pixels, 33 696 bytes).  Then, per displacement: the workgroup computes the term tile T_delta, C_delta on the 66 x 6 positions into one half of a
// double-buffered LDS tile (so one barrier per displacement suffices: the half written at displacement k + 1 is the one read at k - 1, and every thread
// has passed the barrier of k since), and each thread adds its nine entries in patch row-major order from 0.f, sums the counts, divides once, tests
// <= tau, applies the main-pixel and clipped-window rules and sets the bit.  A mask word is stored when its 32 displacements are done (the displacement
// counter is uniform, so the store is too); 28 bytes leave the kernel per pixel instead of the 845 of the planes.
// A term whose pixel x or y lies outside the image is computed on staged zeros and never read: a bit is evaluated only when both patches lie inside.
// ---------------------------------------------------------------------------------------------------
constexpr int FX_TW = PMX_TW + 2, FX_TH = PMX_TH + 2, FX_NP = FX_TW * FX_TH; // the term tile: the tile plus the patch halo

__global__ __launch_bounds__(256) void k_masks_moments_cross_fused(const float *__restrict__ mA, const float *__restrict__ PA, const float *__restrict__ mB,
                                                                    const float *__restrict__ PB, int W, int H, int b, float eps, float tau, int words,
                                                                    uint32_t *__restrict__ mask, int32_t *__restrict__ count)
{
    extern __shared__ float lds[];
    const int ncols = FX_TW + 2 * b, nrows = FX_TH + 2 * b, np = ncols * nrows;
    float *nbv = lds;                  // 6 planes of np: the neighbour, origin (row0 - 1 - b, col0 - 1 - b)
    float *frv = nbv + 6 * np;         // 6 planes of FX_NP: the frame, origin (row0 - 1, col0 - 1)
    float *tT = frv + 6 * FX_NP;       // 2 term tiles
    int *tC = reinterpret_cast<int *>(tT + 2 * FX_NP); // 2 count tiles
    const int col0 = blockIdx.x * PMX_TW, row0 = blockIdx.y * PMX_TH;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = col0 + tx, r = row0 + ty;
    const bool inside = c < W && r < H;
    const bool is_main = inside && r >= 1 && r <= H - 2 && c >= 1 && c <= W - 2;
    const size_t pix = (size_t)r * W + c;
    const int side = 2 * b + 1, nbits = side * side;

    for (int i = threadIdx.x; i < np; i += 256) {
        const int lr = i / ncols, lc = i - lr * ncols;
        float v[6];
        load_moments(mB, PB, W, H, row0 - 1 - b + lr, col0 - 1 - b + lc, v);
#pragma unroll
        for (int k = 0; k < 6; ++k) nbv[k * np + i] = v[k];
    }
    for (int i = threadIdx.x; i < FX_NP; i += 256) {
        const int lr = i / FX_TW, lc = i - lr * FX_TW;
        float v[6];
        load_moments(mA, PA, W, H, row0 - 1 + lr, col0 - 1 + lc, v);
#pragma unroll
        for (int k = 0; k < 6; ++k) frv[k * FX_NP + i] = v[k];
    }
    __syncthreads();

    uint32_t cur = 0;
    int total = 0, k = 0;
    for (int dl = -b; dl <= b; ++dl)
        for (int dc = -b; dc <= b; ++dc, ++k) {
            float *bT = tT + (k & 1) * FX_NP;
            int *bC = tC + (k & 1) * FX_NP;
            for (int i = threadIdx.x; i < FX_NP; i += 256) {
                const int lr = i / FX_TW, lc = i - lr * FX_TW;
                float a[6];
#pragma unroll
                for (int j = 0; j < 6; ++j) a[j] = frv[j * FX_NP + i];
                float s;
                int n;
                moments_term(a, nbv, np, (lr + dl + b) * ncols + lc + dc + b, eps, &s, &n);
                bT[i] = s; bC[i] = n;
            }
            __syncthreads();
            const int qr = r + dl, qc = c + dc;
            if (is_main && qr >= 1 && qr <= H - 2 && qc >= 1 && qc <= W - 2) {
                float s = 0.f;
                int n = 0;
#pragma unroll
                for (int ol = 0; ol < 3; ++ol)
#pragma unroll
                    for (int oc = 0; oc < 3; ++oc) {
                        const int idx = (ty + ol) * FX_TW + tx + oc;
                        s += bT[idx];
                        n += bC[idx];
                    }
                const float d = s / (float)n;
                if (d <= tau) cur |= 1u << (k & 31); // NaN: not similar
            }
            if ((k & 31) == 31 || k == nbits - 1) {
                if (inside) mask[pix * words + (k >> 5)] = cur;
                total += __popc(cur);
                cur = 0;
            }
        }
    if (inside) count[pix] = total;
}

size_t masks_moments_cross_fused_lds(int b)
{
    return ((size_t)6 * (FX_TW + 2 * b) * (FX_TH + 2 * b) + 6 * FX_NP + 4 * FX_NP) * sizeof(float);
}

} // namespace

// The displacement lines one staging of k_pairdist_moments_cross serves: the most that keep the dynamic LDS within 64 KiB, spread evenly over the bands
// (b <= 13: all 2b + 1 lines in one band; b = 14: 15 + 14; b = 15: 16 + 15).  0: b outside what the stage calls accept -- nothing is launched.
int bcd_pairdist_moments_cross_band(int b)
{
    if (b < 0 || b > 15) return 0;
    const int side = 2 * b + 1;
    const size_t line_bytes = pairdist_moments_cross_lds(b, 1) / PMX_TH; // one staged line of every plane
    const int max_nl = (int)(PMX_LDS_LIMIT / line_bytes) - (PMX_TH - 1);
    if (max_nl < 1) return 0;
    const int bands = (side + max_nl - 1) / max_nl;
    return (side + bands - 1) / bands;
}

// does the form without planes serve this geometry?
int bcd_masks_moments_cross_fused_applies(int w, int b) { return w == 1 && b >= 1 && b <= 6; }

// T: (2b+1)^2 planes of W*H floats, Cn: as many planes of W*H bytes (what bcd_launch_masks_cross reads); colours W*H*3 and per-pixel covariances W*H*6 floats of
// the frame (A) and of the neighbour (B)
hipError_t bcd_launch_pairdist_moments_cross(const float *colA, const float *pixcovA, const float *colB, const float *pixcovB, int W, int H, int b, float var_floor,
                                             float *T, uint8_t *Cn, hipStream_t st)
{
    if (W <= 0 || H <= 0 || !colA || !pixcovA || !colB || !pixcovB || !T || !Cn) return hipErrorInvalidValue;
    const int nl = bcd_pairdist_moments_cross_band(b);
    if (nl < 1) return hipErrorInvalidValue;
    const size_t lds = pairdist_moments_cross_lds(b, nl);
    if (lds > PMX_LDS_LIMIT) return hipErrorInvalidValue;
    const dim3 grid((W + PMX_TW - 1) / PMX_TW, (H + PMX_TH - 1) / PMX_TH);
    hipLaunchKernelGGL(k_pairdist_moments_cross, grid, dim3(256), lds, st, colA, pixcovA, colB, pixcovB, W, H, b, nl, var_floor, T, Cn);
    return hipGetLastError();
}

// mask: W*H*words, count: W*H, as bcd_launch_masks_cross writes them; patch radius 1, 1 <= b <= 6 (bcd_masks_moments_cross_fused_applies)
hipError_t bcd_launch_masks_moments_cross_fused(const float *colA, const float *pixcovA, const float *colB, const float *pixcovB, int W, int H, int b, float tau,
                                                float var_floor, uint32_t *mask, int32_t *count, hipStream_t st)
{
    if (W <= 0 || H <= 0 || !colA || !pixcovA || !colB || !pixcovB || !mask || !count || !bcd_masks_moments_cross_fused_applies(1, b)) return hipErrorInvalidValue;
    const size_t lds = masks_moments_cross_fused_lds(b);
    if (lds > PMX_LDS_LIMIT) return hipErrorInvalidValue;
    const int side = 2 * b + 1, words = (side * side + 31) / 32;
    const dim3 grid((W + PMX_TW - 1) / PMX_TW, (H + PMX_TH - 1) / PMX_TH);
    hipLaunchKernelGGL(k_masks_moments_cross_fused, grid, dim3(256), lds, st, colA, pixcovA, colB, pixcovB, W, H, b, var_floor, tau, words, mask, count);
    return hipGetLastError();
}
