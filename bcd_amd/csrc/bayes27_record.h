// bayes27_record.h -- the contract of the 27-component estimate chain, written down once: the constants of a patch vector and its matrices, the
// per-item record in HBM between the chain's kernels and how a chunk's `records` buffer is carved into it, the frame geometry the kernels get by
// value, and the work queues of the persistent kernels.  Included by k_bayes27.hip, k_jacobi27.hip (through bayes27_jacobi.h), k_bayes_temporal.hip
// and bcd_selftest.hip.  Everything is `inline` or constant in an anonymous namespace: no symbol becomes public.
#pragma once
#include "bcd_common.h"
#include <stddef.h>

namespace {

constexpr int K = 27, KP = 28, LD = 29, P = 9, MSZ = KP * KP, CHUNK = MSZ / K; // matrix buffer: 784 floats; 29 members per staging chunk
constexpr int JLD = 28;   // leading dimension of the eigensolver's matrices (row / column 27: zero padding)
constexpr int AUX27 = 96; // noise 54, mean 27, padding
static_assert(MSZ >= KP * JLD && MSZ >= (K - 1) * LD + K, "a matrix buffer holds 28 x 28 (Jacobi layout) or 27 rows of stride 29");

typedef float v16f __attribute__((ext_vector_type(16)));

// ---- the frame and its search window, as the kernels get them
struct Geom27 {
    int W, H, b, side, words, maxS;
};
inline Geom27 geom27(int W, int H, int b) { const int side = 2 * b + 1; return Geom27{ W, H, b, side, (side * side + 31) / 32, side * side }; }

// ---- the records of a chunk: A | V | C | aux | eig | redo list, each slice holding all items of the chunk
struct Records27 {
    float *A, *V, *C, *aux, *eig; // [items][784], [items][784], [items][784], [items][AUX27], [items][28]
};
// floats of an item in front of each slice, and in front of the redo list (ints: [0] the count, [1..] the items the register-resident finish hands over)
constexpr size_t REC27_V = MSZ, REC27_C = REC27_V + MSZ, REC27_AUX = REC27_C + MSZ, REC27_EIG = REC27_AUX + AUX27, RECORD27_FLOATS = REC27_EIG + KP;
constexpr size_t RECORD27_BYTES = RECORD27_FLOATS * sizeof(float) + 2 * sizeof(int); // bcd_bayes27_record_bytes(): + the item's share of the redo list
struct Chunk27Records { Records27 rec; int *redo; };
inline Chunk27Records carve27(float *records, int nb_items)
{
    const size_t n = (size_t)nb_items;
    return Chunk27Records{ { records, records + n * REC27_V, records + n * REC27_C, records + n * REC27_AUX, records + n * REC27_EIG },
                           reinterpret_cast<int *>(records + n * RECORD27_FLOATS) };
}
static_assert(RECORD27_BYTES - RECORD27_FLOATS * sizeof(float) >= 2 * sizeof(int), "behind the slices: a counter and one int per item (nb_items >= 1)");
static_assert(REC27_V % 4 == 0 && REC27_C % 4 == 0 && REC27_AUX % 4 == 0 && REC27_EIG % 4 == 0 && RECORD27_FLOATS % 4 == 0, "every slice starts on 16 bytes");

// ---- work distribution of the persistent kernels.  One counter serves 50-90 same-address atomics per microsecond: with a single counter per
// kernel the 36 000 grabs of a 1080p scale were 0.4 ms (finish kernel with its body skipped) to 0.7 ms (prepare kernel) on their own.
// Items are dealt round-robin to BCD_WORK_QUEUES counters in cache lines of their own (item = queue + 8 k); a wavefront starts on
// the queue of its XCD (workgroups go round-robin over the 8 XCDs) and moves on to the next queue when one is empty, so nothing is
// left behind and the tail stays balanced.
struct WorkCursor { int q, tried; };
__device__ inline WorkCursor work_begin() { return WorkCursor{ (int)(blockIdx.x % BCD_WORK_QUEUES), 0 }; }
__device__ inline int work_next(int *work, int nb_items, int lane, WorkCursor &c)
{
    while (c.tried < BCD_WORK_QUEUES) {
        int k = 0;
        if (lane == 0) k = atomicAdd(work + c.q * BCD_WORK_STRIDE, 1);
        k = __builtin_amdgcn_readfirstlane(k);
        const int item = c.q + BCD_WORK_QUEUES * k;
        if (item < nb_items) return item;
        c.q = (c.q + 1) % BCD_WORK_QUEUES;
        ++c.tried;
    }
    return -1;
}
// every kernel of a chunk's chain has a group of queues of its own in the chunk's BCD_WORK_INTS zeroed ints
enum WorkGroup27 { WORK_PREPARE = 0, WORK_SOLVE, WORK_FINISH, WORK_REDO, WORK_GROUPS };
constexpr int WORK_GROUP_INTS = BCD_WORK_QUEUES * BCD_WORK_STRIDE;
static_assert(BCD_WORK_INTS == WORK_GROUPS * WORK_GROUP_INTS, "prepare | solve | finish | finish of the redo list");
inline int *work_group(int *d_work, WorkGroup27 which) { return d_work + which * WORK_GROUP_INTS; }

// Round 6: the host launches the estimate kernels of a chunk BEFORE it knows how many items the list holds (the count is still on its way back:
// bayes() in bcd_api.hip); `d_n` then points at the list's length on the device and `nb_items` is the capacity the records were sized for.
__device__ inline int items_on_device(const int *d_n, int first_item, int nb_items) { return d_n ? max(0, min(nb_items, *d_n - first_item)) : nb_items; }

__device__ inline int noise_idx(int i, int j) { return i == j ? i : (i + j == 1 ? 5 : (i + j == 2 ? 4 : 3)); } // 3x3 symmetric block from xx,yy,zz,yz,xz,xy

} // namespace
