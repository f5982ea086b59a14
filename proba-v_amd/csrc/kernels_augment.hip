// Batch augmentation (gfx950): one launch builds a training batch from the device-resident UN-augmented patches.  It replaces the
// materialised augmentation of the reference's dataset builder (utils/dataGenerator.py:227-273: augmentByShufflingLRImgs,
// augmentByFlipping, augmentByRotating -- (numPermute + 1) x 4 x 4 copies of the training set, dumped to disk and held in host memory).
// proba-v_amd/augment.py makes the recipes and drives it.
//
// Per output sample b the recipe row (int32 [3 + T]) is {i, f, k, perm[0..T)}: base sample i, flip code f (0 none, 1 axis 0, 2 axis 1,
// 3 both), k counter-clockwise quarter turns, and the frame permutation.  In numpy terms, on the axes of one sample:
//     lr_b[b]   = rot90(flip(lr[i][:, :, perm], FL[f]), k)        hr_b[b] = rot90(flip(hr[i], FL[f]), k)      mask_b[b] likewise
// flip first, then rotate: the order in which stage 5 of the builder composes them.  Bits are moved, never computed with.
//
// Index form.  With n = side - 1, rot90 reads (a, b) = (y, x) | (x, n - y) | (n - y, n - x) | (n - x, y) for k = 0..3 at output pixel
// (y, x), and the flip mirrors a and / or b.  The source pixel is therefore AFFINE in (y, x): p = P0 + y PI + x PJ, and the source
// element of output element (y, j), j = x TC + t C + c the offset inside the output row, is  TC (P0 + y PI) + tab[j]  with
//     tab[j] = TC x PJ + perm[t] C + c
// one table of side x TC entries per sample (198 at H = 22, T = 9), built once per workgroup: the two divisions by TC and C happen
// there, not per element.
//
// Shape.  Grid (B, 3): one workgroup of 256 threads per (output sample, tensor: LR / HR / mask).  The workgroup copies its source
// sample into LDS with 16-byte loads along the sample (17 424 B / 9 216 B / 2 304 B at the shipped shapes: consecutive lanes,
// consecutive 16 B), waits once, and writes the output sample in order, 4 elements per lane (16 B of fp32, 4 B of mask), each element
// gathered from LDS through the table.  Global memory sees only unit-stride full-width accesses on both sides whatever the code; the
// transpose of the odd rotations and the 36-byte frame granules are LDS addressing.  A 4-element store may straddle two output rows
// (a row is 198 floats at H = 22, T = 9: 8-byte, not 16-byte, multiples), so the row / offset pair is carried per element: one integer
// division per store.  Samples whose byte size is not a multiple of 16 take the element-wise instance of the same code.
// No atomics, no hand-off between workgroups: every output byte has one writer, so the result does not depend on the launch.
//
// Safety.  A recipe row whose base index, code or permutation entry is out of range is skipped by all three of its workgroups before
// anything is read (the decision is uniform across the workgroup): a bad recipe cannot read outside the base arrays.  The host
// validates recipes before launching (augment.py); this guard is the second line.
//
// The per-sample part (augment_part and its index helpers) lives in augment_part.h: kernels_ensemble.hip uses it for the LR variants of
// inference patches.
#include "probav_common.h"
#include "augment_part.h"
#include "../../include/probav_hip.h"

namespace probav {

namespace {

struct AugGeom {
    int64_t n_base;
    int H, T, C, S;
    int lr_vec, hr_vec, mask_vec;       // 1: the sample's byte size is a multiple of 16 and the arrays are 16-byte aligned
};

__global__ __launch_bounds__(AUG_THREADS) void augment_batch_kernel(const float* __restrict__ lr, const float* __restrict__ hr,
                                                                     const uint8_t* __restrict__ mask, const int32_t* __restrict__ recipe,
                                                                     AugGeom g, float* __restrict__ lr_b, float* __restrict__ hr_b,
                                                                     uint8_t* __restrict__ mask_b)
{
    extern __shared__ __align__(16) unsigned char aug_smem[];
    const size_t b = blockIdx.x;
    const int32_t* r = recipe + b * (size_t)(3 + g.T);
    const int i = r[0], f = r[1], k = r[2];
    bool bad = i < 0 || (int64_t)i >= g.n_base || (unsigned)f > 3u || (unsigned)k > 3u;
    for (int t = 0; t < g.T; ++t) bad |= (unsigned)r[3 + t] >= (unsigned)g.T;
    if (bad) return;                                        // the same answer in every thread of the sample's three workgroups
    if (blockIdx.y == 0) {
        const size_t n = (size_t)g.H * g.H * g.T * g.C;
        if (g.lr_vec) augment_part<float, 4>(lr + (size_t)i * n, lr_b + b * n, g.H, g.T * g.C, g.C, r + 3, f, k, aug_smem);
        else augment_part<float, 1>(lr + (size_t)i * n, lr_b + b * n, g.H, g.T * g.C, g.C, r + 3, f, k, aug_smem);
    } else if (blockIdx.y == 1) {
        const size_t n = (size_t)g.S * g.S;
        if (g.hr_vec) augment_part<float, 4>(hr + (size_t)i * n, hr_b + b * n, g.S, 1, 1, nullptr, f, k, aug_smem);
        else augment_part<float, 1>(hr + (size_t)i * n, hr_b + b * n, g.S, 1, 1, nullptr, f, k, aug_smem);
    } else {
        const size_t n = (size_t)g.S * g.S;
        if (g.mask_vec) augment_part<uint8_t, 4>(mask + (size_t)i * n, mask_b + b * n, g.S, 1, 1, nullptr, f, k, aug_smem);
        else augment_part<uint8_t, 1>(mask + (size_t)i * n, mask_b + b * n, g.S, 1, 1, nullptr, f, k, aug_smem);
    }
}

}  // namespace

}  // namespace probav

using namespace probav;

extern "C" int probav_augment_batch(const float* lr, const float* hr, const uint8_t* mask, int64_t n_base, int H, int T, int C, int S,
                                    const int32_t* recipe, int64_t batch, float* lr_b, float* hr_b, uint8_t* mask_b, void* stream)
{
    if (!lr || !hr || !mask || !recipe || !lr_b || !hr_b || !mask_b || n_base < 1 || n_base > 0x7fffffff || batch < 1 || batch > 0x7fffffff ||
        H < 1 || H > AUG_MAX_SIDE || S < 1 || S > AUG_MAX_SIDE || T < 1 || T > AUG_MAX_T || C < 1 || C > AUG_MAX_C) {
        set_error("probav_augment_batch: null/invalid argument (1 <= n_base, batch < 2^31, 1 <= H, S <= 1024, 1 <= T <= 64, 1 <= C <= 16)", hipSuccess);
        return PROBAV_EINVAL;
    }
    const size_t lds_lr = aug_part_lds(H, T * C, sizeof(float)), lds_hr = aug_part_lds(S, 1, sizeof(float)), lds_mk = aug_part_lds(S, 1, 1);
    const size_t lds = lds_lr > lds_hr ? (lds_lr > lds_mk ? lds_lr : lds_mk) : (lds_hr > lds_mk ? lds_hr : lds_mk);
    if (lds > AUG_LDS_LIMIT) {
        set_error("probav_augment_batch: one sample (LR H*H*T*C or HR S*S floats, plus a row table) must fit 64 KiB of LDS", hipSuccess);
        return PROBAV_EINVAL;
    }
    AugGeom g;
    g.n_base = n_base; g.H = H; g.T = T; g.C = C; g.S = S;
    g.lr_vec = ((size_t)H * H * T * C) % 4 == 0 && aug_aligned16(lr, lr_b);
    g.hr_vec = ((size_t)S * S) % 4 == 0 && aug_aligned16(hr, hr_b);
    g.mask_vec = ((size_t)S * S) % 16 == 0 && aug_aligned16(mask, mask_b);
    hipLaunchKernelGGL(augment_batch_kernel, dim3((unsigned)batch, 3), dim3(AUG_THREADS), lds, (hipStream_t)stream, lr, hr, mask, recipe, g,
                       lr_b, hr_b, mask_b);
    return check_launch("augment_batch_kernel");
}
