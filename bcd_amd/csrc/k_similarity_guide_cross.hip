// k_similarity_guide_cross.hip -- the feature gate of the cross-frame selection ("Features"): pair-distance planes between the
// feature buffers of a frame and those of a neighbour frame, the producer of the T / C planes that k_masks_cross (k_similarity_cross.hip) box-sums into the
// cross feature mask G_j, which k_gate_masks (k_similarity_guide.hip) ANDs into the neighbour's cross mask.
//
// For pixel x of the frame and pixel y = x + delta of the neighbour, y inside the image, channels k = 0 .. F-1 in order, from s = 0.f, n = 0 (f0, v0: the
// frame's features and the variances of their means, fj, vj: the neighbour's, eps_k: the floor of channel k):
//     d = f0_k(x) - fj_k(y)
//     q = (v0_k(x) + vj_k(y)) + eps_k                      (no variances: q = 0.f + eps_k)
//     if (q > 0.f) { t = (d * d) / q;  if (t == t) { s = s + t; n = n + 1; } }
//     T_delta(x) = s, C_delta(x) = n
// This is k_pairdist_guide's term with the second operand read from the neighbour: a NaN term is skipped, an infinite term is counted.  Between two
// frames there is no symmetry, so all (2b+1)^2 displacements are evaluated; plane k = (dl + b)(2b + 1) + (dc + b) is mask bit k, the layout of
// k_pairdist_cross, entries whose y leaves the image are not written.  A neighbour that IS the frame gives, bit for bit, the planes of k_pairdist_guide.
// This file is compiled with -ffp-contract=off and the correctly rounded fp32 division (tests/guide_cross_ref.py states these operations in NumPy float32).
#include "bcd_common.h"

namespace {

constexpr int PGX_TW = 64; // tile width (one wavefront per tile line)
constexpr int PGX_TH = 4;  // tile height (4 wavefronts per workgroup)
constexpr size_t PGX_LDS_LIMIT = 64 * 1024; // what a kernel may ask for without raising its dynamic-LDS attribute

struct GuideCrossFloors { float e[BCD_GUIDE_MAX_CHANNELS]; };

// One thread per pixel of a 64 x 4 tile.  The thread's own F (2F with variances) values of the FRAME stay in registers.  The NEIGHBOUR's values are staged
// through LDS, one plane per value (consecutive lanes read consecutive words: no bank conflict), for a BAND of `nl` displacement lines at a time: the band
// [dl0, dl0 + nl) needs the neighbour's lines row0 + dl0 .. row0 + dl0 + nl + 2 and the columns col0 - b .. col0 + 63 + b.  The whole halo (b lines above
// and below) would be 204 544 B at F = 8 with variances and b = 15; the band keeps every geometry within 64 KiB (bcd_pairdist_guide_cross_band).
// F divisions, a 4-byte and a 1-byte store per (pixel, displacement).
template <int F, bool VAR>
__global__ __launch_bounds__(256) void k_pairdist_guide_cross(const float *__restrict__ fA, const float *__restrict__ vA, const float *__restrict__ fB,
                                                               const float *__restrict__ vB, int W, int H, int b, int nl, GuideCrossFloors eps,
                                                               float *__restrict__ T, uint8_t *__restrict__ Cn)
{
    extern __shared__ float lds[];
    constexpr int NV = VAR ? 2 * F : F;
    const int ncols = PGX_TW + 2 * b, nrows = PGX_TH + nl - 1, np = ncols * nrows;
    const int col0 = blockIdx.x * PGX_TW, row0 = blockIdx.y * PGX_TH;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = col0 + tx, r = row0 + ty;
    const bool inside = c < W && r < H;
    const size_t plane = (size_t)W * H, pix = (size_t)r * W + c;
    const int side = 2 * b + 1;

    float f1[F], v1[F];
#pragma unroll
    for (int k = 0; k < F; ++k) {
        f1[k] = inside ? fA[pix * F + k] : 0.f;
        v1[k] = (VAR && inside) ? vA[pix * F + k] : 0.f;
    }

    for (int dl0 = -b; dl0 <= b; dl0 += nl) {
        const int dl1 = min(b, dl0 + nl - 1);
        __syncthreads(); // (the previous band has been read)
        // the neighbour's lines row0 + dl0 .. and columns col0 - b .., zeros outside the image: their results are not written
        for (int i = threadIdx.x; i < np; i += 256) {
            const int lr = i / ncols, lc = i - lr * ncols;
            const int gr = row0 + dl0 + lr, gc = col0 - b + lc;
            float x[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) x[k] = 0.f;
            if (gr >= 0 && gr < H && gc >= 0 && gc < W) {
                const size_t p = ((size_t)gr * W + gc) * F;
#pragma unroll
                for (int k = 0; k < F; ++k) {
                    x[k] = fB[p + k];
                    if (VAR) x[F + k] = vB[p + k];
                }
            }
#pragma unroll
            for (int k = 0; k < NV; ++k) lds[k * np + i] = x[k];
        }
        __syncthreads();

        for (int dl = dl0; dl <= dl1; ++dl) {
            const int nr = r + dl;
            const int line = (ty + dl - dl0) * ncols + tx + b;
            for (int dc = -b; dc <= b; ++dc) {
                const int nb = line + dc;
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

typedef void (*pairdist_guide_cross_fn)(const float *, const float *, const float *, const float *, int, int, int, int, GuideCrossFloors, float *, uint8_t *);

template <bool VAR> pairdist_guide_cross_fn pairdist_guide_cross_kernel(int F)
{
    switch (F) {
    case 1: return k_pairdist_guide_cross<1, VAR>;
    case 2: return k_pairdist_guide_cross<2, VAR>;
    case 3: return k_pairdist_guide_cross<3, VAR>;
    case 4: return k_pairdist_guide_cross<4, VAR>;
    case 5: return k_pairdist_guide_cross<5, VAR>;
    case 6: return k_pairdist_guide_cross<6, VAR>;
    case 7: return k_pairdist_guide_cross<7, VAR>;
    case 8: return k_pairdist_guide_cross<8, VAR>;
    }
    return nullptr;
}

size_t pairdist_guide_cross_lds(int F, bool var, int b, int nl) { return (size_t)(var ? 2 * F : F) * (PGX_TW + 2 * b) * (PGX_TH + nl - 1) * sizeof(float); }

} // namespace

// The displacement lines one staging of k_pairdist_guide_cross serves: the most that keep the dynamic LDS within 64 KiB, spread evenly over the bands
// (b = 6: all 13 lines up to F = 6 with variances, 7 + 6 at F = 7 and 8 with variances; b = 15, F = 8 with variances: 7 lines, 5 bands).  0: F or b outside
// what the stage calls accept -- nothing is launched for such a geometry.  (F = 8 with variances at b = 15 still fits 7 lines: every accepted geometry
// has a band.)
int bcd_pairdist_guide_cross_band(int F, int has_var, int b)
{
    if (F < 1 || F > BCD_GUIDE_MAX_CHANNELS || b < 0 || b > 15) return 0;
    const int side = 2 * b + 1;
    const size_t line_bytes = pairdist_guide_cross_lds(F, has_var != 0, b, 1) / PGX_TH; // one staged line of every plane
    const int max_nl = (int)(PGX_LDS_LIMIT / line_bytes) - (PGX_TH - 1);
    if (max_nl < 1) return 0;
    const int bands = (side + max_nl - 1) / max_nl;
    return (side + bands - 1) / bands;
}

// T: (2b+1)^2 planes of W*H floats, Cn: as many planes of W*H bytes (what bcd_launch_masks_cross reads); features W*H*F floats of the frame (A) and of the
// neighbour (B), variances the same for both or null for both; floors: F host floats
hipError_t bcd_launch_pairdist_guide_cross(const float *featA, const float *varA, const float *featB, const float *varB, int F, const float *floors, int W, int H,
                                           int b, float *T, uint8_t *Cn, hipStream_t st)
{
    if (W <= 0 || H <= 0 || !featA || !featB || !floors || !T || !Cn || (varA == nullptr) != (varB == nullptr)) return hipErrorInvalidValue;
    const bool var = varA != nullptr;
    const int nl = bcd_pairdist_guide_cross_band(F, var, b);
    if (nl < 1) return hipErrorInvalidValue;
    const size_t lds = pairdist_guide_cross_lds(F, var, b, nl);
    if (lds > PGX_LDS_LIMIT) return hipErrorInvalidValue;
    GuideCrossFloors eps = {};
    for (int k = 0; k < F; ++k) eps.e[k] = floors[k];
    const dim3 grid((W + PGX_TW - 1) / PGX_TW, (H + PGX_TH - 1) / PGX_TH);
    const pairdist_guide_cross_fn k = var ? pairdist_guide_cross_kernel<true>(F) : pairdist_guide_cross_kernel<false>(F);
    hipLaunchKernelGGL(k, grid, dim3(256), lds, st, featA, varA, featB, varB, W, H, b, nl, eps, T, Cn);
    return hipGetLastError();
}
