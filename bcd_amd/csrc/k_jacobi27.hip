// k_jacobi27.hip -- SOLVE of the 27-component estimate chain: the eigen-decomposition of every A = C - N of a chunk (clampNegativeEigenValues,
// DenoisingUnit.cpp:606-630), two matrices per wavefront, persistent single-wavefront workgroups that take pairs from the work queues:
//   k_jacobi27_quads   production: the rows go through LDS once per three rounds (its task is in bayes27_jacobi.h, shared with k_prepare_solve27)
//   k_jacobi27_batch   comparison (BCD_HIP_JACOBI_PAIRS=1): Brent-Luk ordering, the rows through LDS every round
// and their launcher bcd_launch_jacobi27_batch, which also serves the stand-alone entry points bcd_hip_eig27_batch*, with the two stopping rules.
#include "bcd_launch.h"
#include "bayes27_jacobi.h"
#include <atomic>

namespace {

// ---- parallel two-sided Jacobi, Brent-Luk ordering, rows held in registers ------------------------------
// Slots 0..27 (27 = zero padding) are paired (2i, 2i+1).  One round: lanes i < 14 compute the rotation of pair i from
// LDS; lanes 0..27 load ONE row of A each (7 x ds_read_b128), lanes 32..58 keep their row of V in registers; every lane applies
// the 14 column-pair rotations on registers with static indices, lane pairs (2i, 2i+1) exchange their rows with a DPP
// quad_perm (row rotation of A), and the rows of A are written back in place at their Brent-Luk permuted
// position: slot s moves to sigma(s), 0->0, 1->2, 2i->2i+2, 26->27, 2i+1->2i-1.  After 27 rounds every pair of slots
// has met once (one sweep).  Eigenvalues = diagonal of A (in slot order), eigenvectors = columns of V (same order):
// V f(diag) V^T needs no bookkeeping of the permutation.  Matrices here use a leading dimension of 28 floats.
__device__ inline float dpp_xor1(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1 /* quad_perm [1,0,3,2] */, 0xf, 0xf, true));
}

// x[k] += ms * (x[k] of lane ^ 1) for the 28 elements of a row, in place: 28 v_fmac_f32_dpp.  One asm block: the leading s_nop covers
// the two wait states the hardware wants between a VALU write of a VGPR and a DPP read of it (the compiler does not look inside an
// asm statement for that hazard); inside the block every instruction touches its own register only.
__device__ inline void rowrot_dpp(float (&x)[28], float ms)
{
#define BCD_F(i) "v_fmac_f32_dpp %" #i ", %" #i ", %28 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    asm volatile("s_nop 1\n\t"
                 BCD_F(0) BCD_F(1) BCD_F(2) BCD_F(3) BCD_F(4) BCD_F(5) BCD_F(6) BCD_F(7) BCD_F(8) BCD_F(9) BCD_F(10) BCD_F(11) BCD_F(12) BCD_F(13)
                 BCD_F(14) BCD_F(15) BCD_F(16) BCD_F(17) BCD_F(18) BCD_F(19) BCD_F(20) BCD_F(21) BCD_F(22) BCD_F(23) BCD_F(24) BCD_F(25) BCD_F(26) BCD_F(27)
                 : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]), "+v"(x[8]), "+v"(x[9]),
                   "+v"(x[10]), "+v"(x[11]), "+v"(x[12]), "+v"(x[13]), "+v"(x[14]), "+v"(x[15]), "+v"(x[16]), "+v"(x[17]), "+v"(x[18]), "+v"(x[19]),
                   "+v"(x[20]), "+v"(x[21]), "+v"(x[22]), "+v"(x[23]), "+v"(x[24]), "+v"(x[25]), "+v"(x[26]), "+v"(x[27])
                 : "v"(ms));
#undef BCD_F
}

__device__ inline int sigma_slot(int s)
{
    return s == 0 ? 0 : (s == 1 ? 2 : (s == 26 ? 27 : ((s & 1) ? s - 2 : s + 2)));
}

// ---------------------------------------------------------------------------------------------------------------------
// Batched eigensolver: the same Brent-Luk two-sided Jacobi, two matrices per wavefront and nothing else in the kernel.
// Matrix h of a pair lives in lanes 32 h .. 32 h + 27 (rows of A, moved through LDS every round) and, in a second register
// set of the same lanes, the rows of V (never move).  The LDS traffic and the row / column rotations of A are shared by the
// two matrices -- per matrix and round ~100 VALU and ~10 LDS instructions instead of ~140 and ~21 -- and with 6.5 KB of LDS
// per wavefront the residency is bound by registers only (3 wavefronts per SIMD = 24 matrices per CU instead of 12).
//   in:  A  [n][28 x 28] (JLD layout, row / column 27 zero)      out: eig [n][28] (slot order), V [n][28 x 28] (rows 0..26)
// ---------------------------------------------------------------------------------------------------------------------
__device__ inline float half_sum(float v)
{
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// LDS placement of row r of a matrix of the batched solver (bank facts: MI355X_MICROARCH.md, LDS).  ds_read_b128 serves the lane groups
// {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} of a half, banks (a / 4) mod 64; ds_write_b128 serves groups of 8 consecutive lanes, banks
// (a / 4) mod 32.  With the rows at a stride of 28 dwords the LOADS of a round (lane r <- row r) are conflict free, but (a) the idle lanes
// 28..31 used to re-read row 0, which shares its banks with row 16 of their group, and (b) the STORES go to the Brent-Luk permuted slots:
// lanes 0..7 write the rows {0, 2, 4, 1, 6, 3, 8, 5}, and rows 0 and 8 start on the same bank mod 32 -- together SQ_LDS_BANK_CONFLICT =
// 17 % of the LDS pipe's cycles (r3 counters).  Row 8 therefore lives behind the matrix at a start bank of its own (found by exhaustive
// search over the load and store groups: every group conflict free), and the idle lanes re-read row 16.
constexpr int JROW8 = 28 * 28 + 20;        // start of row 8: (JROW8 / 4) mod 16 = 9
constexpr int JMAT = JROW8 + 28;           // floats per matrix in LDS (832)
template <bool PAD> __device__ inline int jrow_t(int r) { return (PAD && r == 8) ? JROW8 : r * 28; }

template <bool PAD, bool FUSE>
__global__ __launch_bounds__(64, 3) void k_jacobi27_batch(const float *Ain, int n, int *work,
                                                          float *__restrict__ eig, float *__restrict__ Vout,
                                                          float conv2 /* stop at off^2 <= conv2 diag^2 */, float *Aout /* optional (may be Ain): the matrix as the sweeps left it, V^T A V */,
                                                          const int *d_n, int first_item)
{
    n = items_on_device(d_n, first_item, n);
    auto jrow = [](int r) { return jrow_t<PAD>(r); };
    __shared__ float4 lds4[(2 * JMAT + 4 * KP) / 4];
    float *Abuf = reinterpret_cast<float *>(lds4);
    float *cs = Abuf + 2 * JMAT;      // [matrix][28]: per slot pair (-beta, alpha) of the current round
    float *dv = cs + 2 * KP;          // [matrix][28]: scale of every slot (see below)
    const int lane = threadIdx.x, h = lane >> 5, r = lane & 31;
    float *Ah = Abuf + h * JMAT;
    float *cs_h = cs + h * KP, *dv_h = dv + h * KP;
    const bool isRow = r < KP;
    const float *src = Ah + jrow(isRow ? r : (PAD ? 16 : 0)); // (idle lanes: the address of a lane of their own ds_read_b128 group)
    float *dst = Ah + jrow(isRow ? sigma_slot(r) : 0);
    WorkCursor cursor = work_begin();
    for (;;) {
        const int pair = work_next(work, (n + 1) / 2, lane, cursor);
        if (pair < 0) break;
        const int first = 2 * pair;
        const int item = first + h;
        const bool live = item < n;
        // matrix -> LDS (an absent second matrix is the identity: converged from the start)
        {
            const float4 *g = reinterpret_cast<const float4 *>(Ain + (size_t)(live ? item : first) * (KP * JLD));
            for (int e = r; e < KP * JLD / 4; e += 32) {
                float4 v = g[e];
                const int e0 = 4 * e, rr = e0 / JLD, c0 = e0 - rr * JLD;
                if (!live) v = make_float4(rr == c0, rr == c0 + 1, rr == c0 + 2, rr == c0 + 3);
                *reinterpret_cast<float4 *>(Ah + jrow(rr) + c0) = v;
            }
            if (isRow) dv_h[r] = 1.f;
        }
        wave_sync();
        // Scaled ("fast") rotations: the matrices are kept as A = D A~ D and V = V~ D with a diagonal D (one scale per slot).
        // J = [[c, s], [-s, c]] = [[1, t], [-t, 1]] diag(c, c), so rotating the slot pair (p, q) is
        //     x' = x - beta y,  y' = y + alpha x   (beta = t d_q / d_p, alpha = t d_p / d_q)   and   d' = c d
        // -- two fused multiply-adds per element pair instead of four operations; D is folded back into A~ and V~ at the start of
        // every sweep (within a sweep a scale cannot fall below 2^(-27/2)).
        float vrow[JLD];
#pragma unroll
        for (int k = 0; k < JLD; ++k) vrow[k] = (k == r) ? 1.f : 0.f; // V = identity
        for (int sweep = 0; sweep < 12; ++sweep) {
            // fold the scales: A~ <- D A~ D, V~ <- V~ D, D <- I; off / diagonal norms of the true matrix on the way
            float off = 0.f, dg = 0.f;
            {
                float dk[JLD];
#pragma unroll
                for (int q4 = 0; q4 < JLD / 4; ++q4) {
                    float4 w4 = reinterpret_cast<const float4 *>(dv_h)[q4];
                    dk[4 * q4] = w4.x; dk[4 * q4 + 1] = w4.y; dk[4 * q4 + 2] = w4.z; dk[4 * q4 + 3] = w4.w;
                }
                const float dr = dv_h[isRow ? r : 0];
                float row[JLD];
#pragma unroll
                for (int q4 = 0; q4 < JLD / 4; ++q4) {
                    float4 v = reinterpret_cast<const float4 *>(src)[q4];
                    row[4 * q4] = v.x; row[4 * q4 + 1] = v.y; row[4 * q4 + 2] = v.z; row[4 * q4 + 3] = v.w;
                }
#pragma unroll
                for (int k = 0; k < JLD; ++k) {
                    row[k] *= dr * dk[k];
                    vrow[k] *= dk[k];
                    if (isRow) { if (k == r) dg = fmaf(row[k], row[k], dg); else off = fmaf(row[k], row[k], off); }
                }
                wave_sync(); // every lane has read the scales and its row
                if (isRow) {
#pragma unroll
                    for (int q4 = 0; q4 < JLD / 4; ++q4)
                        reinterpret_cast<float4 *>(Ah + jrow(r))[q4] = make_float4(row[4 * q4], row[4 * q4 + 1], row[4 * q4 + 2], row[4 * q4 + 3]);
                    dv_h[r] = 1.f;
                }
                wave_sync();
            }
            off = half_sum(off);
            dg = half_sum(dg);
            // off^2 <= 1e-12 diag^2: the positive part V max(0, lambda) V^T is Lipschitz in the matrix, so what is left off the diagonal moves it
            // by <= 1e-6 |A|.  (1e-10 saved 3 % of the solver and was fine on the 32-spp frames, but the 8-spp 4K frame of configs[3] then
            // differed from the oracle by 1.9e-5 -- its inverses are worse conditioned -- against 2.9e-6 with this threshold.)  A converged
            // matrix is frozen -- identity rotations -- while its partner finishes: its result does not depend on who shares the wavefront
            const bool settled = off <= conv2 * dg;
            if (__builtin_amdgcn_ballot_w64(!settled) == 0) break; // both matrices converged
            // fully unrolled: the Brent-Luk column move of the rows of V~ (a 27-cycle of the register names) costs no instruction
#pragma unroll
            for (int round = 0; round < KP - 1; ++round) {
                // lanes 0..13 of each half: rotation of the slot pair (2 r, 2 r + 1); the other lanes compute on a harmless copy of pair 0
                float mbeta = 0.f, alpha = 0.f;
                {
                    const int p = r < KP / 2 ? 2 * r : 0, q = p + 1;
                    const float2 d2 = reinterpret_cast<const float2 *>(dv_h)[p >> 1];
                    const float apq_s = Ah[jrow(p) + q], app_s = Ah[jrow(p) + p], aqq_s = Ah[jrow(q) + q];
                    float dp = d2.x, dq = d2.y;
                    if (apq_s != 0.f && !settled) {
                        const float apq = dp * dq * apq_s, app = dp * dp * app_s, aqq = dq * dq * aqq_s;
                        // 1-ulp hardware reciprocal / sqrt / rsqrt: a rotation only has to be orthogonal to working
                        // precision (c^2 + s^2 = 1 +- 1e-7), not the exact minimiser
                        const float theta = (aqq - app) * __builtin_amdgcn_rcpf(2.f * apq);
                        if (fabsf(theta) < 1e18f) { // (otherwise theta^2 overflows: the rotation is the identity to fp32)
                            float t = __builtin_amdgcn_rcpf(fabsf(theta) + __builtin_amdgcn_sqrtf(fmaf(theta, theta, 1.f)));
                            t = theta < 0.f ? -t : t;
                            const float c = __builtin_amdgcn_rsqf(fmaf(t, t, 1.f));
                            const float ratio = dq * __builtin_amdgcn_rcpf(dp);
                            mbeta = -t * ratio;
                            alpha = t * __builtin_amdgcn_rcpf(ratio);
                            dp *= c;
                            dq *= c;
                        }
                    }
                    float row[JLD];
#pragma unroll
                    for (int q4 = 0; q4 < JLD / 4; ++q4) {
                        float4 v = reinterpret_cast<const float4 *>(src)[q4];
                        row[4 * q4] = v.x; row[4 * q4 + 1] = v.y; row[4 * q4 + 2] = v.z; row[4 * q4 + 3] = v.w;
                    }
                    if (r < KP / 2) {
                        reinterpret_cast<float2 *>(cs_h)[r] = make_float2(mbeta, alpha);
                        dv_h[sigma_slot(p)] = dp; // the scales move with their slots
                        dv_h[sigma_slot(q)] = dq;
                    }
                    wave_sync();
                    float rot[JLD];
#pragma unroll
                    for (int q4 = 0; q4 < JLD / 4; ++q4) {
                        float4 w4 = reinterpret_cast<const float4 *>(cs_h)[q4];
                        rot[4 * q4] = w4.x; rot[4 * q4 + 1] = w4.y; rot[4 * q4 + 2] = w4.z; rot[4 * q4 + 3] = w4.w;
                    }
                    const float2 pcs = reinterpret_cast<const float2 *>(cs_h)[isRow ? (r >> 1) : 0];
                    // column rotations of A~
#pragma unroll
                    for (int j = 0; j < KP / 2; ++j) {
                        const float x = row[2 * j], y = row[2 * j + 1];
                        row[2 * j] = fmaf(rot[2 * j], y, x);
                        row[2 * j + 1] = fmaf(rot[2 * j + 1], x, y);
                    }
                    // row rotations of A~: rows (2i, 2i+1) live in lanes (2i, 2i+1) of their half and take the rotation of pair i
                    {
                        const float ms = (r & 1) ? pcs.y : pcs.x;
                        // row[k] += ms * row[k] of the partner lane: ONE v_fmac_f32 with the lane exchange as its DPP modifier (the
                        // compiler emits v_mov_b32_dpp + v_fma_f32; VOP3 has no DPP form on gfx9)
                        float out[JLD];
                        if (FUSE) {
                            rowrot_dpp(row, ms);
#pragma unroll
                            for (int k = 0; k < JLD; ++k) out[sigma_slot(k)] = row[k]; // Brent-Luk column move (register renaming)
                        } else {
#pragma unroll
                            for (int k = 0; k < JLD; ++k) out[sigma_slot(k)] = fmaf(ms, dpp_xor1(row[k]), row[k]);
                        }
                        if (isRow) {
#pragma unroll
                            for (int q4 = 0; q4 < JLD / 4; ++q4)
                                reinterpret_cast<float4 *>(dst)[q4] = make_float4(out[4 * q4], out[4 * q4 + 1], out[4 * q4 + 2], out[4 * q4 + 3]);
                        }
                    }
                    // the same column rotations (and column move) on the rows of V~
                    {
                        float out[JLD];
#pragma unroll
                        for (int j = 0; j < KP / 2; ++j) {
                            const float x = vrow[2 * j], y = vrow[2 * j + 1];
                            out[sigma_slot(2 * j)] = fmaf(rot[2 * j], y, x);
                            out[sigma_slot(2 * j + 1)] = fmaf(rot[2 * j + 1], x, y);
                        }
#pragma unroll
                        for (int k = 0; k < JLD; ++k) vrow[k] = out[k];
                    }
                }
                wave_sync(); // the rows of A~ are back in LDS before the next round reads its pivots
            }
        }
        if (live) {
            if (isRow) eig[(size_t)item * KP + r] = Ah[jrow(r) + r];
        }
        if (Aout) { // (wave-uniform)
            if (isRow) cs_h[r] = Ah[jrow(r) + r];
            wave_sync();
            if (isRow && live) jacobi_write_correction(Aout + (size_t)item * (KP * JLD) + r * JLD, Ah + jrow(r), cs_h, r);
        }
        if (live) {
            if (r < K) {
                float4 *o = reinterpret_cast<float4 *>(Vout + (size_t)item * (KP * JLD) + r * JLD);
#pragma unroll
                for (int q4 = 0; q4 < JLD / 4; ++q4) o[q4] = make_float4(vrow[4 * q4], vrow[4 * q4 + 1], vrow[4 * q4 + 2], vrow[4 * q4 + 3]);
            }
        }
        wave_sync(); // the next pair reuses the LDS
    }
}

__global__ __launch_bounds__(64, 3) void k_jacobi27_quads(const float *Ain, int n, int *work, float *__restrict__ eig,
                                                          float *__restrict__ Vout, float conv2, float *Aout, const int *d_n, int first_item)
{
    n = items_on_device(d_n, first_item, n);
    __shared__ float4 lds4[JQ_LDS / 4];
    const int lane = threadIdx.x;
    const JqLane L = jq_lane_setup(reinterpret_cast<float *>(lds4), lane);
    wave_sync();
    WorkCursor cursor = work_begin();
    for (;;) {
        const int pair = work_next(work, (n + 1) / 2, lane, cursor);
        if (pair < 0) break;
        jacobi_quads_pair(L, pair, n, Ain, eig, Vout, conv2, Aout);
    }
}

// the stopping rules (off^2 <= conv2 diag^2; what the looser one leaves is corrected to first order by the finish kernels: pos_part_lds in k_bayes27.hip)
constexpr float JACOBI_CONV2_CORRECTED = 2e-9f; // off / diag <= 4.5e-5
constexpr float JACOBI_CONV2_STRICT = 1e-12f;   // the round-3 rule: one sweep more, the correction then has nothing left to do

} // namespace

// Stopping rule of the estimate chain's eigensolver: 2e-9 + first-order correction (production), or -- strict mode, BCD_HIP_STRICT_EIGEN=1 or
// bcd_hip_set_strict_eigensolver -- the fully converged 1e-12 (the looser rule spends accuracy on ill-conditioned low-spp frames, 9.8e-6
// instead of 2.9e-6 on the 4K 8-spp frame; a caller who wants the margin back can have it for ~1.5 % of the step)
static std::atomic<int> g_strict_eigen{ -1 }; // (-1: the setter was not called, the environment decides)
void bcd_bayes27_set_strict_eigensolver(int on) { g_strict_eigen.store(on ? 1 : 0); }
float bcd_bayes27_chain_conv2() { const int v = g_strict_eigen.load(); return bcd_bayes27_conv2(v < 0 ? bcd_bayes27_switches().strict_eigen : v); }

// the two rules by name, for the stand-alone eigensolver entry point (bcd_hip_eig27_batch_rule)
float bcd_bayes27_conv2(int strict) { return strict ? JACOBI_CONV2_STRICT : JACOBI_CONV2_CORRECTED; }

// eigen-decomposition of n symmetric 27 x 27 matrices (28 x 28 zero-padded, row-major): persistent wavefronts, two matrices each
hipError_t bcd_launch_jacobi27_batch(const float *A, int n, int *d_work, int blocks, float *eig, float *V, hipStream_t st, float conv2, float *Aout,
                                     const int *d_n /* optional: the number of matrices is min(n, *d_n - first_item), read on the device */, int first_item)
{
    if (blocks <= 0) return hipSuccess;
    // <padded row placement, DPP-fused row rotation>: measured on 65 536 matrices 31.3 ns per matrix without either, 31.1 with the
    // placement alone (bank conflicts 17 % -> 0.4 % of the LDS cycles), 29.8 with the fused rotation alone (-17 % vector instructions),
    // 29.4 with both
    // (the comparison kernel keeps the plain rule: its residual is then far below what the correction of the finish kernels would notice)
    if (bcd_bayes27_switches().jacobi_pairs)
        hipLaunchKernelGGL((k_jacobi27_batch<true, true>), dim3(blocks), dim3(64), 0, st, A, n, d_work, eig, V, 1e-12f, Aout, d_n, first_item);
    else hipLaunchKernelGGL(k_jacobi27_quads, dim3(blocks), dim3(64), 0, st, A, n, d_work, eig, V, conv2, Aout, d_n, first_item);
    return hipGetLastError();
}
