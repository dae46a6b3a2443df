// k_bayes_temporal.hip -- the estimate of a processed pixel whose similar set spans several frames of a sequence, patch radius 1,
// search radius 6.  The similar set is S = S_0 (in the frame itself) followed by S_1 .. S_F (in the neighbour frames, in the order given), each in window
// row-major order; the neighbours lend statistics only:
//   k_prepare27t           PREPARE  what k_bayes27<1> / k_bayes27w<1> do (k_bayes27.hip), over the members of all frames: computeNoiseCovPatchesMean
//                                   (:400-419, each member's per-pixel covariance from its own frame), the colour mean (:500-509) and the empirical covariance
//                                   (:511-536) in member order, the covariance on the f32 matrix core; the record it leaves -- A = C - N, C, N, m, the cleared
//                                   redo counter -- is the record of those kernels, so the unchanged solver (k_jacobi27_quads) and finish kernels (k_finish27w,
//                                   redo list k_bayes27w<2>) follow: they read the record, the IN-FRAME mask and the frame's colours, i.e. they compute and
//                                   aggregate the estimates of the members in S_0 only
//   k_bayes_weak_temporal  FALLBACK denoiseOnlyMainPatch (:455-481) with the average over the colour patches of all members of all frames, added to the main
//                                   patch only
//   k_bayes_weak_temporal_layers    the same for several colour layers on one selection (bcd_hip_denoise_temporal_layers): the masks walked once, G layers
//                                   summed in registers
// Members are gathered from global memory (the gather form of k_bayes27<1>): a member's frame is part of its code.
// The record, the work queues and noise_idx are those of the chain: bayes27_record.h.
#include "bcd_launch.h"
#include "bayes27_record.h"
#include <algorithm>

namespace {

// a frame's pointers by index: a chain of selects on the by-value table (a wave-uniform index keeps them on the scalar unit)
__device__ inline const float *frame_col(const BcdFrameTable &t, int f)
{
    const float *r = t.col[0];
#pragma unroll
    for (int i = 1; i <= BCD_MAX_NEIGHBOURS; ++i) r = f == i ? t.col[i] : r;
    return r;
}
__device__ inline const float *frame_pixcov(const BcdFrameTable &t, int f)
{
    const float *r = t.pixcov[0];
#pragma unroll
    for (int i = 1; i <= BCD_MAX_NEIGHBOURS; ++i) r = f == i ? t.pixcov[i] : r;
    return r;
}
__device__ inline const uint32_t *frame_mask(const BcdFrameTable &t, int f)
{
    const uint32_t *r = t.mask[0];
#pragma unroll
    for (int i = 1; i <= BCD_MAX_NEIGHBOURS; ++i) r = f == i ? t.mask[i] : r;
    return r;
}

// member code: frame << 12 | (dl + B) << 8 | (dc + B)
__device__ inline int code_frame(int code) { return code >> 12; }
template <int B> __device__ inline int code_pixel(int code, int p, int W) { return p + (((code >> 8) & 15) - B) * W + ((code & 255) - B); }

struct Records27t {
    float *A, *C, *aux; // [items][784], [items][784], [items][AUX27]  (V and the eigenvalues are the solver's)
    int *redo;          // the redo list of the finish kernel: its counter is cleared here
};

template <int B>
__global__ __launch_bounds__(64) void k_prepare27t(BcdFrameTable t, const int32_t *__restrict__ list, int first_item, int nb_items, int *work, int W,
                                                   Records27t rec)
{
    constexpr int SIDE = 2 * B + 1, WORDS = (SIDE * SIDE + 31) / 32, MAXM = SIDE * SIDE * (BCD_MAX_NEIGHBOURS + 1);
    static_assert(SIDE <= 16 && WORDS <= 32, "a window line and column fit four bits of the member code, the mask words one per lane of a half");
    __shared__ __attribute__((aligned(16))) float chunk[MSZ]; // member-staging chunk: CHUNK members x K components
    __shared__ __attribute__((aligned(16))) float noise[56], mean[KP];
    __shared__ uint16_t mem[(MAXM + 7) / 8 * 8];
    const int lane = threadIdx.x;
    if (blockIdx.x == 0 && lane == 0) rec.redo[0] = 0; // (the chunk's redo list is empty: the finish kernel appends to it two launches later)

    WorkCursor cursor = work_begin();
    for (;;) {
        const int slot = work_next(work, nb_items, lane, cursor);
        if (slot < 0) break;
        const int p = __builtin_amdgcn_readfirstlane(list[first_item + slot]);
        float *recA = rec.A + (size_t)slot * MSZ, *recC = rec.C + (size_t)slot * MSZ, *recX = rec.aux + (size_t)slot * AUX27;

        // ---- the members: S_0 in window order, then S_1 .. S_F, each in window order
        int n = 0;
        for (int f = 0; f < t.n; ++f) {
            uint32_t m = lane < WORDS ? frame_mask(t, f)[(size_t)p * WORDS + lane] : 0u;
            if (lane == WORDS - 1 && (SIDE * SIDE) % 32 != 0) m &= (1u << ((SIDE * SIDE) % 32)) - 1u; // (bits beyond the window are no members: the list holds MAXM)
            const int cntw = __popc(m);
            int pre = cntw;
            for (int off = 1; off < 32; off <<= 1) {
                const int v = __shfl_up(pre, off);
                if (lane >= off) pre += v;
            }
            const int total = __shfl(pre, WORDS - 1);
            int pos = n + pre - cntw;
            while (m) {
                const int bit = __ffs(m) - 1;
                m &= m - 1;
                const int k = lane * 32 + bit, kl = k / SIDE, kc = k - kl * SIDE;
                mem[pos++] = (uint16_t)((f << 12) | (kl << 8) | kc);
            }
            n += total;
        }
        __syncthreads();

        // ---- computeNoiseCovPatchesMean (:400-419) and empiricalMean (:500-509) in one sweep over the members: lanes 0..53 own one noise component, lanes
        // 0..26 also one colour component.  The loads of 8 members are issued back to back, the sums stay in member order.
        {
            const float n_inv = 1.f / (float)n;
            int noff, coff; // (idle lanes repeat the loads of the last owner: no branches around the loads)
            { const int l = min(lane, P * 6 - 1), o = l / 6, j = l - o * 6; noff = ((o / 3 - 1) * W + (o % 3 - 1)) * 6 + j; }
            { const int l = min(lane, K - 1), o = l / 3, ch = l - o * 3; coff = ((o / 3 - 1) * W + (o % 3 - 1)) * 3 + ch; }
            float accn = 0.f, accm = 0.f;
            for (int i = 0; i < n; i += 8) {
                float vn[8], vm[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int code = __builtin_amdgcn_readfirstlane((int)mem[min(i + u, n - 1)]); // (the same for every lane)
                    const int f = code_frame(code);
                    const long long q = code_pixel<B>(code, p, W);
                    vn[u] = frame_pixcov(t, f)[q * 6 + noff];
                    vm[u] = frame_col(t, f)[q * 3 + coff];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (i + u < n) { accn += vn[u]; accm += vm[u]; }
            }
            if (lane < P * 6) noise[lane] = accn * n_inv;
            if (lane < K) mean[lane] = accm * n_inv;
            __syncthreads();
        }

        // ---- centerPointCloud + empiricalCovarianceMatrix (:511-536) on the matrix core: C = Xc^T Xc, two members per v_mfma_f32_32x32x2_f32 (f32 in, f32
        // accumulate: a chain of fma in member order; both operands are the same centred value, so the result is bitwise symmetric).
        // Operand layout: lane l holds element i = l & 31 of member 2s + (l >> 5); rows / columns 27..31 are zero.
        {
            const int mi = lane & 31, mk = lane >> 5;
            const float my_mean = mi < K ? mean[mi] : 0.f;
            v16f acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
            for (int i0 = 0; i0 < n; i0 += CHUNK) {
                const int cn = min(CHUNK, n - i0);
                // pickColorPatchesFromColorImage (:483-498): members [i0, i0 + cn), each from its own frame
                for (int e = lane; e < cn * K; e += 64) {
                    const int i = e / K, k = e - i * K, o = k / 3, ch = k - o * 3;
                    const int code = mem[i0 + i];
                    const long long q = code_pixel<B>(code, p, W) + (o / 3 - 1) * W + (o % 3 - 1);
                    chunk[e] = frame_col(t, code_frame(code))[q * 3 + ch];
                }
                __syncthreads();
                for (int s2 = 0; s2 < cn; s2 += 2) {
                    const int m = s2 + mk;
                    const float a = (m < cn && mi < K) ? chunk[m * K + mi] - my_mean : 0.f;
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, a, acc, 0, 0, 0);
                }
                __syncthreads();
            }
            const float inv = 1.f / (float)(n - 1);
            // C/D layout: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  C goes to the record in the LD layout, C - N -- the matrix whose
            // negative eigenvalues are clamped, Step 1 (:421-436) -- in the eigensolver's 28 x 28 layout, padding row / column zero
            const int mo = mi / 3, mj = mi - 3 * mo;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = (e & 3) + 8 * (e >> 2) + 4 * mk;
                const float v = acc[e] * inv; // rows / columns 27..31 of the product are exactly zero (zero operands)
                if (r < K && mi < LD) recC[r * LD + mi] = v;
                if (r < KP && mi < KP) {
                    const int ro = r / 3, ri = r - 3 * ro;
                    const float nv = (ro == mo && r < K && mi < K) ? noise[ro * 6 + noise_idx(ri, mj)] : 0.f;
                    recA[r * JLD + mi] = v - nv;
                }
            }
        }
        // a non-finite entry of the noise mean makes the whole estimate of the item NaN in the reference: a NaN colour mean carries that through the
        // finish kernels (noise_poisons_item in k_bayes27.hip; all 64 lanes take part)
        const bool poisoned = __builtin_amdgcn_ballot_w64(lane < P * 6 && !isfinite(noise[lane])) != 0;
        if (lane < P * 6) recX[lane] = noise[lane];
        if (lane < K) recX[P * 6 + lane] = poisoned ? __builtin_nanf("") : mean[lane];
        __syncthreads(); // the next item reuses the LDS
    }
}

// denoiseOnlyMainPatch (:455-481) over several frames: one lane per (fallback pixel, patch pixel), seven pixels per wavefront; every lane walks the masks
// of its pixel frame by frame in window order -- the member order, so the three channel sums are sequential sums in member order -- and adds its patch
// pixel of every member.  No LDS, no barrier.  |S| = 0 gives 0 * inf = NaN like the reference.
template <int B>
__global__ __launch_bounds__(64) void k_bayes_weak_temporal(BcdFrameTable t, const int32_t *__restrict__ list, const int32_t *__restrict__ d_nlist, int W,
                                                            float *sum, int32_t *cnt)
{
    constexpr int SIDE = 2 * B + 1, WORDS = (SIDE * SIDE + 31) / 32, PER_WAVE = 64 / P;
    const int lane = threadIdx.x, slot = lane / P, o = lane - slot * P;
    const int nlist = *d_nlist;
    for (int base = blockIdx.x * PER_WAVE; base < nlist; base += gridDim.x * PER_WAVE) {
        const int item = base + slot;
        if (slot >= PER_WAVE || item >= nlist) continue;
        const int p = list[item];
        const long long pp = (long long)p + (o / 3 - 1) * W + (o % 3 - 1); // patch pixel o of the main patch
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        int n = 0;
        for (int f = 0; f < t.n; ++f) {
            const float *src = frame_col(t, f) + pp * 3;
            const uint32_t *mw = frame_mask(t, f) + (size_t)p * WORDS;
            for (int wd = 0; wd < WORDS; ++wd) {
                uint32_t m = mw[wd];
                while (m) {
                    const int k = wd * 32 + __ffs(m) - 1;
                    m &= m - 1;
                    const int kl = k / SIDE, kc = k - kl * SIDE;
                    const int rel = ((kl - B) * W + (kc - B)) * 3;
                    a0 += src[rel]; a1 += src[rel + 1]; a2 += src[rel + 2];
                    ++n;
                }
            }
        }
        const float n_inv = 1.f / (float)n;
        float *dst = sum + pp * 3;
        unsafeAtomicAdd(dst, n_inv * a0);
        unsafeAtomicAdd(dst + 1, n_inv * a1);
        unsafeAtomicAdd(dst + 2, n_inv * a2);
        if (cnt) atomicAdd(cnt + pp, 1);
    }
}

// k_bayes_weak_temporal for SEVERAL colour layers that share the selection (bcd_hip_denoise_temporal_layers): the lanes, the list walk and the mask walk are
// those of the kernel above, done ONCE; every decoded member adds its patch pixel of G layers to G x 3 register accumulators.  blockIdx.y takes layers
// [y G, y G + G).  The member order is the single-layer kernel's and so are the operations on a layer's three sums: before the atomics they are bit for
// bit those of k_bayes_weak_temporal run on that layer alone.  |S| = 0 gives NaN in every layer.  The layers share ONE count image: `cnt` (null: none) is
// filled by the first group, once.
// The pointers travel by value.  The group's (frame, layer) colour pointers are picked once, by select chains on blockIdx.y over statically indexed table
// entries; the frame's are picked per frame by select chains on the (wave-uniform) frame index, as frame_col does: nothing is indexed dynamically.
template <int B, int G>
__global__ __launch_bounds__(64) void k_bayes_weak_temporal_layers(BcdFrameLayerTable t, const int32_t *__restrict__ list, const int32_t *__restrict__ d_nlist,
                                                                   int W, int32_t *cnt)
{
    constexpr int SIDE = 2 * B + 1, WORDS = (SIDE * SIDE + 31) / 32, PER_WAVE = 64 / P, NF = BCD_MAX_NEIGHBOURS + 1, GROUPS = BCD_MAX_LAYERS / G;
    static_assert(BCD_MAX_LAYERS % G == 0, "the groups tile the table");
    const int lane = threadIdx.x, slot = lane / P, o = lane - slot * P;
    const int grp = blockIdx.y, ng = min(G, t.layers - grp * G);
    const float *gcol[NF][G];
    float *gsum[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const float *r = t.col[f][j];
#pragma unroll
            for (int z = 1; z < GROUPS; ++z) r = grp == z ? t.col[f][z * G + j] : r;
            gcol[f][j] = r;
        }
        float *s = t.sum[j];
#pragma unroll
        for (int z = 1; z < GROUPS; ++z) s = grp == z ? t.sum[z * G + j] : s;
        gsum[j] = s;
    }
    const int nlist = *d_nlist;
    for (int base = blockIdx.x * PER_WAVE; base < nlist; base += gridDim.x * PER_WAVE) {
        const int item = base + slot;
        if (slot >= PER_WAVE || item >= nlist) continue;
        const int p = list[item];
        const long long pp = (long long)p + (o / 3 - 1) * W + (o % 3 - 1); // patch pixel o of the main patch
        float a[G][3];
#pragma unroll
        for (int j = 0; j < G; ++j) { a[j][0] = 0.f; a[j][1] = 0.f; a[j][2] = 0.f; }
        int n = 0;
        for (int f = 0; f < t.n; ++f) {
            const float *src[G];
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const float *r = gcol[0][j];
#pragma unroll
                for (int i = 1; i < NF; ++i) r = f == i ? gcol[i][j] : r;
                src[j] = r + pp * 3;
            }
            const uint32_t *mw = t.mask[0];
#pragma unroll
            for (int i = 1; i < NF; ++i) mw = f == i ? t.mask[i] : mw;
            mw += (size_t)p * WORDS;
            for (int wd = 0; wd < WORDS; ++wd) {
                uint32_t m = mw[wd];
                while (m) {
                    const int k = wd * 32 + __ffs(m) - 1;
                    m &= m - 1;
                    const int kl = k / SIDE, kc = k - kl * SIDE;
                    const int rel = ((kl - B) * W + (kc - B)) * 3;
#pragma unroll
                    for (int j = 0; j < G; ++j) { a[j][0] += src[j][rel]; a[j][1] += src[j][rel + 1]; a[j][2] += src[j][rel + 2]; }
                    ++n;
                }
            }
        }
        const float n_inv = 1.f / (float)n;
#pragma unroll
        for (int j = 0; j < G; ++j) {
            if (j < ng) { // (uniform)
                float *dst = gsum[j] + pp * 3;
                unsafeAtomicAdd(dst, n_inv * a[j][0]);
                unsafeAtomicAdd(dst + 1, n_inv * a[j][1]);
                unsafeAtomicAdd(dst + 2, n_inv * a[j][2]);
            }
        }
        if (cnt && grp == 0) atomicAdd(cnt + pp, 1);
    }
}

} // namespace

// PREPARE of items [first_item, first_item + nb_items) of `list` into `records` (nb_items records as bcd_launch_bayes27 lays them out: A | V | C | aux | eig |
// redo list); d_work: the chunk's zeroed work queues, of which the kernel takes the prepare group
hipError_t bcd_launch_prepare27t(const BcdFrameTable &t, const int32_t *list, int first_item, int nb_items, int *d_work, int num_cus, int W, int b,
                                 float *records, hipStream_t st)
{
    if (nb_items <= 0) return hipSuccess;
    if (b != 6 || t.n < 1 || t.n > BCD_MAX_NEIGHBOURS + 1) return hipErrorInvalidValue;
    const Chunk27Records c = carve27(records, nb_items);
    const Records27t rec{ c.rec.A, c.rec.C, c.rec.aux, c.redo };
    hipLaunchKernelGGL(k_prepare27t<6>, dim3(std::min(nb_items, num_cus * 16)), dim3(64), 0, st, t, list, first_item, nb_items, work_group(d_work, WORK_PREPARE), W,
                       rec);
    return hipGetLastError();
}

hipError_t bcd_launch_bayes_weak_temporal(const BcdFrameTable &t, const int32_t *list, const int32_t *d_nlist, int blocks, int W, int b, float *sum,
                                          int32_t *cnt, hipStream_t st)
{
    if (blocks <= 0) return hipSuccess;
    if (b != 6 || t.n < 1 || t.n > BCD_MAX_NEIGHBOURS + 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bayes_weak_temporal<6>, dim3(blocks), dim3(64), 0, st, t, list, d_nlist, W, sum, cnt);
    return hipGetLastError();
}

// the fallback of every layer in one launch: t.n frames, t.layers layers; `blocks` wavefronts per group of layers; cnt: the shared count image or null
hipError_t bcd_launch_bayes_weak_temporal_layers(const BcdFrameLayerTable &t, const int32_t *list, const int32_t *d_nlist, int blocks, int W, int b, int32_t *cnt,
                                                 hipStream_t st)
{
    if (blocks <= 0) return hipSuccess;
    if (b != 6 || t.n < 1 || t.n > BCD_MAX_NEIGHBOURS + 1 || t.layers < 1 || t.layers > BCD_MAX_LAYERS) return hipErrorInvalidValue;
    BcdFrameLayerTable u = t;
    for (int f = 0; f <= BCD_MAX_NEIGHBOURS; ++f) { // idle slots of a group, unused frames: memory that exists
        if (f >= t.n) u.mask[f] = t.mask[0];
        for (int k = 0; k < BCD_MAX_LAYERS; ++k)
            if (f >= t.n || k >= t.layers) u.col[f][k] = t.col[0][0];
    }
    for (int k = t.layers; k < BCD_MAX_LAYERS; ++k) u.sum[k] = nullptr; // (never flushed)
    const int L = t.layers;
    if (L == 1)
        hipLaunchKernelGGL((k_bayes_weak_temporal_layers<6, 1>), dim3(blocks, 1), dim3(64), 0, st, u, list, d_nlist, W, cnt);
    else if (L == 2)
        hipLaunchKernelGGL((k_bayes_weak_temporal_layers<6, 2>), dim3(blocks, 1), dim3(64), 0, st, u, list, d_nlist, W, cnt);
    else
        hipLaunchKernelGGL((k_bayes_weak_temporal_layers<6, BCD_TEMPORAL_GROUP>), dim3(blocks, (L + BCD_TEMPORAL_GROUP - 1) / BCD_TEMPORAL_GROUP), dim3(64), 0, st, u,
                           list, d_nlist, W, cnt);
    return hipGetLastError();
}
