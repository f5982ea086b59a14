// One sample of one tensor through the augmentation's index map (flip, then quarter turns, with a frame permutation): the part that
// csrc/kernels_augment.hip (a training batch: LR, HR and mask) and csrc/kernels_ensemble.hip (the LR variants of an inference patch) share.
// The index form, the LDS staging and the access pattern are described at the head of kernels_augment.hip.
#pragma once
#include "probav_common.h"

namespace probav {

namespace {

constexpr int AUG_THREADS = 256, AUG_MAX_T = 64, AUG_MAX_SIDE = 1024, AUG_MAX_C = 16;
constexpr size_t AUG_LDS_LIMIT = 64 * 1024;

inline size_t aug_round16(size_t b) { return (b + 15) & ~(size_t)15; }

// staged sample + table of one workgroup
inline size_t aug_part_lds(int side, int TC, size_t elem_bytes)
{
    return aug_round16((size_t)side * side * TC * elem_bytes) + (size_t)side * TC * sizeof(int);
}

// source pixel (row-major index) of output pixel (y, x): flip f, then k quarter turns
__device__ __forceinline__ int aug_src_pixel(int y, int x, int side, int f, int k)
{
    const int n = side - 1;
    int a = y, b = x;
    if (k == 1) { a = x; b = n - y; }
    else if (k == 2) { a = n - y; b = n - x; }
    else if (k == 3) { a = n - x; b = y; }
    if (f & 1) a = n - a;
    if (f & 2) b = n - b;
    return a * side + b;
}

template <typename E, int V>
struct alignas(sizeof(E) * V) AugVec { E v[V]; };

// the staged sample and its row table inside one workgroup's LDS (aug_part_lds bytes)
template <typename E>
__device__ __forceinline__ E* aug_tile(unsigned char* smem) { return reinterpret_cast<E*>(smem); }
template <typename E>
__device__ __forceinline__ int* aug_table(unsigned char* smem, int elems)
{
    return reinterpret_cast<int*>(smem + (((size_t)elems * sizeof(E) + 15) & ~(size_t)15));
}

// the second half of augment_part, for a sample that is ALREADY staged in LDS as tile [side][side][TC] (by the caller, by any loads: a
// barrier is taken here before the tile is read): build the row table, then write dst in order through the affine source map.
// csrc/kernels_crops.hip stages windows cut out of whole scenes and writes them with this.
template <typename E, int V>
__device__ __forceinline__ void augment_emit(E* __restrict__ dst, int side, int TC, int C, const int32_t* __restrict__ perm, int f, int k,
                                             unsigned char* smem)
{
    const int row = side * TC, elems = side * row;
    E* tile = aug_tile<E>(smem);
    int* tab = aug_table<E>(smem, elems);
    const int P0 = aug_src_pixel(0, 0, side, f, k);
    const int PI = aug_src_pixel(1, 0, side, f, k) - P0, PJ = aug_src_pixel(0, 1, side, f, k) - P0;
    for (int j = threadIdx.x; j < row; j += AUG_THREADS) {
        const int x = j / TC, e = j - x * TC, t = e / C, c = e - t * C;
        tab[j] = TC * x * PJ + (perm ? perm[t] : t) * C + c;
    }
    __syncthreads();
    const int rowstep = TC * PI;
    for (int q = threadIdx.x; q < elems / V; q += AUG_THREADS) {
        const int o = q * V;
        int y = o / row, j = o - y * row;
        int base = TC * P0 + y * rowstep;
        AugVec<E, V> out;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if (j == row) { j = 0; base += rowstep; }
            out.v[v] = tile[base + tab[j]];
            ++j;
        }
        *reinterpret_cast<AugVec<E, V>*>(dst + o) = out;
    }
}

// one sample of one tensor: src [side][side][TC] -> dst, TC = frames x channels (1 for HR / mask), perm = the recipe's frame
// permutation in global memory (null: identity)
template <typename E, int V>
__device__ __forceinline__ void augment_part(const E* __restrict__ src, E* __restrict__ dst, int side, int TC, int C,
                                             const int32_t* __restrict__ perm, int f, int k, unsigned char* smem)
{
    const int elems = side * (side * TC);
    E* tile = aug_tile<E>(smem);
    if (V > 1) {
        const uint4* s16 = reinterpret_cast<const uint4*>(src);
        uint4* t16 = reinterpret_cast<uint4*>(smem);
        const int n16 = (int)((size_t)elems * sizeof(E) / 16);
        for (int q = threadIdx.x; q < n16; q += AUG_THREADS) t16[q] = s16[q];
    } else {
        for (int q = threadIdx.x; q < elems; q += AUG_THREADS) tile[q] = src[q];
    }
    augment_emit<E, V>(dst, side, TC, C, perm, f, k, smem);
}

inline bool aug_aligned16(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

}  // namespace

}  // namespace probav
