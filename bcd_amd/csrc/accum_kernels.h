// accum_kernels.h -- what the accumulator's kernel files (k_accumulate.hip, k_accum_features.hip) share: the leading planes of the state and
// the gather machinery of the splatted add (the definition is in include/bcd_hip.h, the design in DESIGN.md section 10).  Everything here is
// local to the file that includes it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// planes of the state: weight sum, squared-weight sum, 3 weighted colour sums, 6 weighted second moments, then the bins
enum { ACC_W = 0, ACC_W2 = 1, ACC_M = 2, ACC_C = 5, ACC_H = 11 };

struct SplatFilter {
    float rx, ry, inv_rx, inv_ry;
    int ts;     // the table is ts x ts
    int kx, ky; // K of the definition: the key frame is extended by it, the candidate pixels of a sample are c0 +- kx, l0 +- ky
    int nx, ny; // cells further than this from a pixel hold no sample that passes dx < rx (nx <= kx: smallest m with m + 0.5 >= rx)
};

// the filter value of the definition for pixel (col, line) and a sample at (x, y); 0: the pixel is not in the sample's footprint
__device__ inline float splat_weight(const SplatFilter &F, const float *T, float x, float y, int col, int line)
{
    const float dx = fabsf(((float)col + 0.5f) - x), dy = fabsf(((float)line + 0.5f) - y);
    if (!(dx < F.rx && dy < F.ry)) return 0.f;
    int ix = (int)(dx * F.inv_rx * (float)F.ts), iy = (int)(dy * F.inv_ry * (float)F.ts);
    ix = ix < F.ts - 1 ? ix : F.ts - 1;
    iy = iy < F.ts - 1 ? iy : F.ts - 1;
    return T[iy * F.ts + ix];
}

// A workgroup of 256 threads owns a tile of SPLAT_TX x SPLAT_TY destination pixels (a wavefront: 2 lines of 32 pixels, 128
// consecutive bytes of every plane per line).  Its RING: the cells of the tile's pixels plus (nx, ny) on each side, row-major.
#define SPLAT_TX 32
#define SPLAT_TY 8
#define SPLAT_MAX_NB 3                                                                       // nx, ny <= 3 (radii <= 3)
#define SPLAT_RING_MAX ((SPLAT_TX + 2 * SPLAT_MAX_NB) * (SPLAT_TY + 2 * SPLAT_MAX_NB))       // 38 x 14 = 532 cells
#define SPLAT_ROWS_MAX (2 * SPLAT_MAX_NB + 1)
#define SPLAT_LDS_BYTES (64 * 1024)
#define SPLAT_NONE 0xffffffffu

// the batch positions and the sample positions of the ring's cells: STAGED in LDS (index = slot in the staged arrays), or read from the
// sorted arrays in global memory (index = place in the sorted batch) when the ring's samples do not fit the staging arrays -- the same
// values in the same order
template <bool STAGED>
struct SplatKeys {
    const uint32_t *g0, *b0;                          // LDS, per ring cell: start in the sorted batch; start in the staged arrays (b0[rc + 1]: end)
    const uint32_t *s_pos;                            // LDS staging arrays
    const float *s_x, *s_y;
    const uint32_t *vals;                             // the sorted batch positions and the batch's sample positions
    const float *xy;
    __device__ uint32_t begin(int rc) const { return STAGED ? b0[rc] : g0[rc]; }
    __device__ uint32_t count(int rc) const { return b0[rc + 1] - b0[rc]; }
    __device__ uint32_t pos(uint32_t i) const { return STAGED ? s_pos[i] : vals[i]; }
    __device__ void position(uint32_t i, float &x, float &y) const
    {
        if (STAGED) { x = s_x[i]; y = s_y[i]; }
        else { const int64_t e = vals[i]; x = xy[2 * e]; y = xy[2 * e + 1]; }
    }
};

// the earliest sample at batch position >= next, in the 2 nx + 1 cells rc0.. of one ring row, that has pixel (col, line) in its footprint:
// its position (SPLAT_NONE: none), index and filter value.  Every run ascends in position.
template <class RUNS>
__device__ inline void splat_row_next(const RUNS &S, const SplatFilter &F, const float *T, int rc0, int col, int line, uint32_t next,
                                      uint32_t &bpos, uint32_t &bidx, float &bf)
{
    bpos = SPLAT_NONE; bidx = 0; bf = 0.f;
    for (int c = 0; c <= 2 * F.nx; ++c) {
        const uint32_t b = S.begin(rc0 + c), cnt = S.count(rc0 + c);
        uint32_t lo = 0, hi = cnt;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (S.pos(b + mid) < next) lo = mid + 1;
            else hi = mid;
        }
        for (uint32_t k = lo; k < cnt; ++k) {
            const uint32_t p = S.pos(b + k);
            if (p >= bpos) break; // (later than the best of the cells before)
            float x, y;
            S.position(b + k, x, y);
            const float f = splat_weight(F, T, x, y, col, line);
            if (f != 0.f) { bpos = p; bidx = b + k; bf = f; break; }
        }
    }
}

// one destination pixel: merges the 2 ny + 1 ring rows' candidates by batch position and hands each contribution -- its index in the
// runs and its filter value -- to sink(idx, f), in stream order.  rc0: the ring cell at the top left of the pixel's neighbourhood; RW:
// cells per ring row
template <class RUNS, class SINK>
__device__ inline void splat_merge(const RUNS &S, const SplatFilter &F, const float *T, int rc0, int RW, int col, int line, SINK &&sink)
{
    uint32_t cpos[SPLAT_ROWS_MAX], cidx[SPLAT_ROWS_MAX];
    float cf[SPLAT_ROWS_MAX];
#pragma unroll
    for (int r = 0; r < SPLAT_ROWS_MAX; ++r) { cpos[r] = SPLAT_NONE; cidx[r] = 0; cf[r] = 0.f; }
    for (int r = 0; r <= 2 * F.ny; ++r) {
        uint32_t np, ni;
        float nf;
        splat_row_next(S, F, T, rc0 + r * RW, col, line, 0u, np, ni, nf);
#pragma unroll
        for (int q = 0; q < SPLAT_ROWS_MAX; ++q)
            if (q == r) { cpos[q] = np; cidx[q] = ni; cf[q] = nf; }
    }
    for (;;) {
        uint32_t best = SPLAT_NONE, idx = 0;
        float f = 0.f;
        int br = 0;
#pragma unroll
        for (int q = 0; q < SPLAT_ROWS_MAX; ++q)
            if (cpos[q] < best) { best = cpos[q]; idx = cidx[q]; f = cf[q]; br = q; }
        if (best == SPLAT_NONE) break;
        sink(idx, f);
        uint32_t np, ni;
        float nf;
        splat_row_next(S, F, T, rc0 + br * RW, col, line, best + 1u, np, ni, nf);
#pragma unroll
        for (int q = 0; q < SPLAT_ROWS_MAX; ++q)
            if (q == br) { cpos[q] = np; cidx[q] = ni; cf[q] = nf; }
    }
}

// the start of a splat workgroup (256 threads, all of them): the table into s_T, the runs of the tile's ring cells into s_g0 (start in
// the sorted batch) and s_b0 (exclusive scan of the counts; s_b0[RC]: the ring's total, which is returned).  Pixel (col, line) is cell
// (col + kx, line + ky) of the extended frame.  Ends with a barrier.
__device__ inline uint32_t splat_ring_load(const uint2 *__restrict__ cells, const float *__restrict__ T, const SplatFilter &F, int W, int H, int px0,
                                           int py0, float *s_T, uint32_t *s_g0, uint32_t *s_b0)
{
    const int t = threadIdx.x, tt = F.ts * F.ts;
    const int RW = SPLAT_TX + 2 * F.nx, RC = RW * (SPLAT_TY + 2 * F.ny);
    const int We = W + 2 * F.kx, He = H + 2 * F.ky;
    for (int e = t; e < tt; e += 256) s_T[e] = T[e];
    for (int rc = t; rc < RC; rc += 256) {
        const int ex = px0 + F.kx - F.nx + rc % RW, ey = py0 + F.ky - F.ny + rc / RW;
        uint2 c = make_uint2(0u, 0u);
        if (ex < We && ey < He) c = cells[(int64_t)ey * We + ex];
        s_g0[rc] = c.x;
        s_b0[rc] = c.y - c.x;
    }
    __syncthreads();
    if (t < 64) { // counts -> exclusive scan (one wavefront, `per` consecutive cells per lane)
        const int per = (RC + 63) / 64, a = t * per;
        uint32_t sum = 0;
        for (int k = 0; k < per; ++k)
            if (a + k < RC) sum += s_b0[a + k];
        uint32_t incl = sum;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(incl, o);
            if (t >= o) incl += v;
        }
        uint32_t run = incl - sum;
        for (int k = 0; k < per; ++k)
            if (a + k < RC) {
                const uint32_t c = s_b0[a + k];
                s_b0[a + k] = run;
                run += c;
            }
        if (t == 63) s_b0[RC] = incl;
    }
    __syncthreads();
    return s_b0[RC];
}

// the batch position of staging slot j: the cell of the slot is the last one with b0 <= j
__device__ inline int64_t splat_slot_sample(const uint32_t *s_g0, const uint32_t *s_b0, int RC, const uint32_t *__restrict__ vals, uint32_t j)
{
    int lo = 0, hi = RC;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s_b0[mid] <= j) lo = mid;
        else hi = mid;
    }
    return vals[s_g0[lo] + (j - s_b0[lo])];
}

SplatFilter splat_filter(const float *f, const int *g)
{
    SplatFilter F;
    F.rx = f[0]; F.ry = f[1]; F.inv_rx = f[2]; F.inv_ry = f[3];
    F.ts = g[0]; F.kx = g[1]; F.ky = g[2]; F.nx = g[3]; F.ny = g[4];
    return F;
}

// LDS of a splat workgroup before its staging arrays: the table (ts * ts), g0[SPLAT_RING_MAX], b0[SPLAT_RING_MAX + 4]
size_t splat_fixed_lds(int ts) { return ((size_t)ts * ts + 2 * SPLAT_RING_MAX + 4) * sizeof(float); }

inline unsigned nblk(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

} // namespace
