// k_masks_transpose.hip -- the cross masks of a frame pair with the roles of the two frames swapped ("Sequences").
//
// The cross distance d(p in A, q in B) of k_similarity_cross.hip is bit for bit d(q in B, p in A): `diff` changes sign exactly and is squared, n1 n2 and
// b1 + b2 commute, the bins and the patch offsets are summed in the same order.  So the masks of (B -> A) are a transposition of the masks of (A -> B):
// with side = 2b + 1, nbits = side^2 and delta_k = (k / side - b, k % side - b),
//   out(p) bit k = in(p + delta_k) bit (nbits - 1 - k)   where p + delta_k lies in the image, else 0
// (displacement nbits - 1 - k is -delta_k: the bit of p + delta_k that points back at p).  No main-pixel rule: cross masks hold no bit at or towards a pixel
// that is not a main pixel, so the transposed masks hold none either.  Bits >= nbits of the last word are 0; count = popcount of the output mask.
//
// One thread per output pixel of the project's 64 x 4 tile.  The masks of the (4 + 2b) x (64 + 2b) pixels around the tile are staged into LDS once (zeros
// outside the image, which is the "else 0" above), with the per-pixel stride padded to an odd number of words: adjacent lanes read adjacent pixels, and an
// odd stride is coprime with the 32 banks of ds_read_b32, so the 32 lanes of a half wave hit 32 banks.  Every thread assembles its words from nbits
// single-bit LDS reads (word and bit index are compile-time constants of the unrolled loops); the words go back through LDS so that the tile's rows leave
// as contiguous runs of 64 * words words.  No float arithmetic; built with -ffp-contract=off like every file.
#include "bcd_launch.h"

namespace {

constexpr int TR_TW = 64; // tile width
constexpr int TR_TH = 4;  // tile height (4 wavefronts per workgroup)
constexpr int TR_MAX_B = 6;

constexpr int tr_words(int b) { return ((2 * b + 1) * (2 * b + 1) + 31) / 32; }
constexpr int tr_stride(int b) { return tr_words(b) | 1; } // odd: 1, 1, 3, 3, 5, 7 words for b = 1 .. 6

template <int B>
__global__ __launch_bounds__(256) void k_masks_transpose(const uint32_t *__restrict__ in, int W, int H, uint32_t *__restrict__ out, int32_t *__restrict__ count)
{
    constexpr int SIDE = 2 * B + 1, NBITS = SIDE * SIDE, WORDS = tr_words(B), STRIDE = tr_stride(B);
    constexpr int NCOLS = TR_TW + 2 * B, NROWS = TR_TH + 2 * B;
    __shared__ uint32_t lds[NROWS * NCOLS * STRIDE]; // b = 6: 16 x 76 x 7 words = 34 048 B
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int col0 = blockIdx.x * TR_TW, row0 = blockIdx.y * TR_TH;

    // stage: consecutive threads read consecutive words of a row segment of the input
    for (int i = threadIdx.x; i < NROWS * NCOLS * WORDS; i += 256) {
        const int p = i / WORDS, wd = i - p * WORDS;
        const int lr = p / NCOLS, lc = p - lr * NCOLS;
        const int gr = row0 - B + lr, gc = col0 - B + lc;
        uint32_t v = 0;
        if (gr >= 0 && gr < H && gc >= 0 && gc < W) v = in[((size_t)gr * W + gc) * WORDS + wd];
        lds[p * STRIDE + wd] = v;
    }
    __syncthreads();

    // out(p) bit k: the partner p + delta_k is local pixel (ty + k / SIDE, tx + k % SIDE) of the staged window, its bit NBITS - 1 - k
    uint32_t o[WORDS];
#pragma unroll
    for (int wd = 0; wd < WORDS; ++wd) o[wd] = 0;
#pragma unroll
    for (int kr = 0; kr < SIDE; ++kr) {
        const uint32_t *row = lds + ((ty + kr) * NCOLS + tx) * STRIDE;
#pragma unroll
        for (int kc = 0; kc < SIDE; ++kc) {
            const int k = kr * SIDE + kc, j = NBITS - 1 - k;
            const uint32_t bit = (row[kc * STRIDE + (j >> 5)] >> (j & 31)) & 1u;
            o[k >> 5] |= bit << (k & 31);
        }
    }
    int total = 0;
#pragma unroll
    for (int wd = 0; wd < WORDS; ++wd) total += __popc(o[wd]);
    const int c = col0 + tx, r = row0 + ty;
    if (count && c < W && r < H) count[(size_t)r * W + c] = total;

    // the words back through LDS (every thread has read what it needs of the staged window), then row-contiguous stores
    __syncthreads();
#pragma unroll
    for (int wd = 0; wd < WORDS; ++wd) lds[threadIdx.x * STRIDE + wd] = o[wd];
    __syncthreads();
    for (int i = threadIdx.x; i < 256 * WORDS; i += 256) {
        const int p = i / WORDS, wd = i - p * WORDS;
        const int oc = col0 + (p & 63), orow = row0 + (p >> 6);
        if (oc < W && orow < H) out[((size_t)orow * W + oc) * WORDS + wd] = lds[p * STRIDE + wd];
    }
}

// |mask(p)| of every pixel (bcd_hip_sequence_last_masks: the counts of kept masks)
__global__ void k_mask_popcount(const uint32_t *__restrict__ mask, int64_t npix, int words, int32_t *__restrict__ count)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    int total = 0;
    for (int wd = 0; wd < words; ++wd) total += __popc(mask[i * words + wd]);
    count[i] = total;
}

} // namespace

// out must not alias in; count may be null; b in 1 .. 6 (the caller checks)
hipError_t bcd_launch_masks_transpose(const uint32_t *in, int W, int H, int b, uint32_t *out, int32_t *count, hipStream_t st)
{
    static_assert(tr_stride(TR_MAX_B) == 7 && (TR_TH + 2 * TR_MAX_B) * (TR_TW + 2 * TR_MAX_B) * tr_stride(TR_MAX_B) * 4 <= 64 * 1024, "static LDS of the widest instantiation");
    const dim3 grid((W + TR_TW - 1) / TR_TW, (H + TR_TH - 1) / TR_TH), block(256);
    switch (b) {
#define BCD_TR_CASE(BB) case BB: hipLaunchKernelGGL((k_masks_transpose<BB>), grid, block, 0, st, in, W, H, out, count); break;
        BCD_TR_CASE(1) BCD_TR_CASE(2) BCD_TR_CASE(3) BCD_TR_CASE(4) BCD_TR_CASE(5) BCD_TR_CASE(6)
#undef BCD_TR_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t bcd_launch_mask_popcount(const uint32_t *mask, int64_t npix, int words, int32_t *count, hipStream_t st)
{
    hipLaunchKernelGGL(k_mask_popcount, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, mask, npix, words, count);
    return hipGetLastError();
}
