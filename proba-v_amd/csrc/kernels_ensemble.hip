// Test-time self-ensemble (gfx950): the two data-movement ends of  E(x) = (1 / V) sum_v G_v^-1( round( clip( net(A_v(x)) ) ) ), the geometric
// self-ensemble of the EDSR / WDSR papers in the form the reference's resolveBySampleAveraging averages its predictions (test.py:137-146: every
// member clipped and rounded before the mean).  proba-v_amd/ensemble.py makes the variant tables and drives both kernels; the V forward passes
// between them are the engine's.
//
// A variant is a recipe row {i, f, k, perm[0..T)} in the convention of kernels_augment.hip: flip code f, then k counter-clockwise quarter
// turns, frame order perm.  Row n V + v of the recipe is variant v of base patch n.
//
// Expand.  lr [N][H][H][T][C] -> [rows][H][H][T][C], out[b] = rot90(flip(lr[i][:, :, perm], FL[f]), k): the LR third of augment_batch_kernel
// (augment_part of augment_part.h: the sample staged in LDS by 16-byte loads, written in order through a per-row table), one workgroup per
// output sample, with its guard against rows that point outside the base array.
//
// Reduce.  sr [N V][S][S] (raw network output) -> out[n] = (1 / V) sum_{v < V} G_v^-1( rint( clip( sr[n V + v], lo, hi ) ) ), optionally rounded
// once more.  G_v^-1(m) = flip(rot90(m, -k), FL[f]); at output pixel (y, x) it reads m at (y', x') with
//     (a, b) = (f & 1 ? n - y : y,  f & 2 ? n - x : x),   (y', x') = (a, b) | (n - b, a) | (n - a, n - b) | (b, n - a)   for k = 0..3, n = S - 1
// (the inverse of aug_src_pixel), affine in (y, x) like the forward map.  One workgroup of 256 threads per base patch: for v = 0 .. V - 1 in
// that order it stages member v in LDS (16-byte loads along the member; rows padded to an odd stride, so that the column walks of the odd
// turns spread over the banks), and every thread adds the clipped, rounded value of its own output pixels to its own slots of an LDS
// accumulator.  Members are integers in [0, 65536] and V <= 256, so the fp32 sum is exact (<= 2^24).  Then one correctly rounded division
// (__fdiv_rn), the optional rint, one store: 16 B per lane along the output row.  The output is either the patches [N][S][S] or, given the
// grid width g, the stitched images [N / g^2][g S][g S] in the row-major block layout of test.py:149-160 (patch n is block (n / g) % g, n % g
// of image n / g^2).  Global memory sees unit-stride accesses on both sides whatever the code; the transposes are LDS addressing.
// No atomics, one writer per output element, no hand-off between workgroups: the result does not depend on the launch.
//
// Safety.  A base patch one of whose V rows carries f or k outside 0..3 is skipped by its workgroup before anything is written (a uniform
// decision); the host validates recipes first (ensemble.py).  Neither kernel reads the recipe's base index to address the predictions.
#include "probav_common.h"
#include "augment_part.h"
#include "image_math.h"
#include "../../include/probav_hip.h"

namespace probav {

namespace {

constexpr int ENS_MAX_V = 256;

__global__ __launch_bounds__(AUG_THREADS) void ensemble_expand_kernel(const float* __restrict__ lr, const int32_t* __restrict__ recipe, int64_t n_base,
                                                                       int H, int T, int C, int vec, float* __restrict__ out)
{
    extern __shared__ __align__(16) unsigned char ens_smem[];
    const size_t b = blockIdx.x;
    const int32_t* r = recipe + b * (size_t)(3 + T);
    const int i = r[0], f = r[1], k = r[2];
    bool bad = i < 0 || (int64_t)i >= n_base || (unsigned)f > 3u || (unsigned)k > 3u;
    for (int t = 0; t < T; ++t) bad |= (unsigned)r[3 + t] >= (unsigned)T;
    if (bad) return;                                        // the same answer in every thread of the workgroup
    const size_t n = (size_t)H * H * T * C;
    if (vec) augment_part<float, 4>(lr + (size_t)i * n, out + b * n, H, T * C, C, r + 3, f, k, ens_smem);
    else augment_part<float, 1>(lr + (size_t)i * n, out + b * n, H, T * C, C, r + 3, f, k, ens_smem);
}

struct EnsGeom {
    int V, S, rs;                       // members per base patch, side of a prediction, ints per recipe row
    int grid;                           // 0: patches [N][S][S]; g >= 1: stitched images [N / g^2][g S][g S]
    int final_round;
    float lo, hi;
};

inline size_t ens_reduce_lds(int S)
{
    return aug_round16((size_t)S * S * sizeof(float)) + (size_t)S * (S | 1) * sizeof(float);
}

// member pixel (index into rows of stride ld) that G^-1 puts at output pixel (y, x): undo the flip f, then the k quarter turns
__device__ __forceinline__ int ens_inv_pixel(int y, int x, int side, int f, int k, int ld)
{
    const int n = side - 1;
    const int a = (f & 1) ? n - y : y, b = (f & 2) ? n - x : x;
    int yy = a, xx = b;
    if (k == 1) { yy = n - b; xx = a; }
    else if (k == 2) { yy = n - a; xx = n - b; }
    else if (k == 3) { yy = b; xx = n - a; }
    return yy * ld + xx;
}

// W = 4: S is a multiple of 4 and the arrays are 16-byte aligned (a group of 4 pixels lies in one row on both sides); W = 1: any S
template <int W>
__global__ __launch_bounds__(AUG_THREADS) void ensemble_reduce_kernel(const float* __restrict__ sr, const int32_t* __restrict__ recipe, EnsGeom g,
                                                                       float* __restrict__ out)
{
    extern __shared__ __align__(16) unsigned char ens_smem[];
    const int S = g.S, px = S * S, ld = S | 1, V = g.V;
    float* acc = reinterpret_cast<float*>(ens_smem);                                     // [S][S]: slot e belongs to the thread that owns pixel e
    float* tile = reinterpret_cast<float*>(ens_smem + (((size_t)px * sizeof(float) + 15) & ~(size_t)15));      // [S][ld]
    const size_t b = blockIdx.x;
    const int32_t* rows = recipe + b * (size_t)V * g.rs;
    for (int q = threadIdx.x; q < px / W; q += AUG_THREADS) {
#pragma unroll
        for (int j = 0; j < W; ++j) acc[q * W + j] = 0.f;
    }
    const float* member = sr + b * (size_t)V * px;
    for (int v = 0; v < V; ++v, member += px) {
        const int f = rows[(size_t)v * g.rs + 1], k = rows[(size_t)v * g.rs + 2];
        if ((unsigned)f > 3u || (unsigned)k > 3u) return;       // the same answer in every thread; nothing has been written yet
        for (int q = threadIdx.x; q < px / W; q += AUG_THREADS) {
            const int e = q * W, y = e / S, x = e - y * S;
            const AugVec<float, W> in = *reinterpret_cast<const AugVec<float, W>*>(member + e);
#pragma unroll
            for (int j = 0; j < W; ++j) tile[y * ld + x + j] = in.v[j];
        }
        __syncthreads();
        const int Q0 = ens_inv_pixel(0, 0, S, f, k, ld);
        const int QI = ens_inv_pixel(1, 0, S, f, k, ld) - Q0, QJ = ens_inv_pixel(0, 1, S, f, k, ld) - Q0;
        for (int q = threadIdx.x; q < px / W; q += AUG_THREADS) {
            const int e = q * W, y = e / S, x = e - y * S;
            const int src = Q0 + y * QI + x * QJ;
            AugVec<float, W> a = *reinterpret_cast<AugVec<float, W>*>(acc + e);
#pragma unroll
            for (int j = 0; j < W; ++j) a.v[j] += clip_rint(tile[src + j * QJ], g.lo, g.hi);
            *reinterpret_cast<AugVec<float, W>*>(acc + e) = a;
        }
        __syncthreads();
    }
    const float den = (float)V;
    size_t obase = b * (size_t)px, orow = (size_t)S;
    if (g.grid) {
        const size_t gg = (size_t)g.grid * g.grid, img = b / gg, blk = b - img * gg, bi = blk / g.grid, bj = blk - bi * g.grid;
        orow = (size_t)g.grid * S;
        obase = img * gg * px + bi * S * orow + bj * S;
    }
    for (int q = threadIdx.x; q < px / W; q += AUG_THREADS) {
        const int e = q * W, y = e / S, x = e - y * S;
        AugVec<float, W> a = *reinterpret_cast<AugVec<float, W>*>(acc + e);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            a.v[j] = __fdiv_rn(a.v[j], den);
            if (g.final_round) a.v[j] = rintf(a.v[j]);
        }
        *reinterpret_cast<AugVec<float, W>*>(out + obase + y * orow + x) = a;
    }
}

}  // namespace

}  // namespace probav

using namespace probav;

extern "C" int probav_ensemble_expand(const float* lr, int64_t n_base, int H, int T, int C, const int32_t* recipe, int64_t rows, float* out, void* stream)
{
    if (!lr || !recipe || !out || n_base < 1 || n_base > 0x7fffffff || rows < 1 || rows > 0x7fffffff || H < 1 || H > AUG_MAX_SIDE || T < 1 ||
        T > AUG_MAX_T || C < 1 || C > AUG_MAX_C) {
        set_error("probav_ensemble_expand: null/invalid argument (1 <= n_base, rows < 2^31, 1 <= H <= 1024, 1 <= T <= 64, 1 <= C <= 16)", hipSuccess);
        return PROBAV_EINVAL;
    }
    const size_t lds = aug_part_lds(H, T * C, sizeof(float));
    if (lds > AUG_LDS_LIMIT) {
        set_error("probav_ensemble_expand: one LR sample (H*H*T*C floats, plus a row table) must fit 64 KiB of LDS", hipSuccess);
        return PROBAV_EINVAL;
    }
    const int vec = ((size_t)H * H * T * C) % 4 == 0 && aug_aligned16(lr, out);
    hipLaunchKernelGGL(ensemble_expand_kernel, dim3((unsigned)rows), dim3(AUG_THREADS), lds, (hipStream_t)stream, lr, recipe, n_base, H, T, C, vec, out);
    return check_launch("ensemble_expand_kernel");
}

extern "C" int probav_ensemble_reduce(const float* sr, const int32_t* recipe, int64_t n_base, int V, int T, int S, float lo, float hi, int final_round,
                                      int grid, float* out, void* stream)
{
    if (!sr || !recipe || !out || n_base < 1 || n_base > 0x7fffffff || T < 1 || T > AUG_MAX_T || S < 1 || S > AUG_MAX_SIDE || grid < 0 || grid > 1024 ||
        !(lo <= hi)) {
        set_error("probav_ensemble_reduce: null/invalid argument (1 <= n_base < 2^31, 1 <= T <= 64, 1 <= S <= 1024, 0 <= grid <= 1024, lo <= hi)", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (V < 1 || V > ENS_MAX_V) {
        set_error("probav_ensemble_reduce: 1 <= V <= 256 members (integers up to 2^16 each: 256 of them sum exactly in fp32, more need not)", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (grid && n_base % ((int64_t)grid * grid)) {
        set_error("probav_ensemble_reduce: a stitched output takes whole images, n_base must be a multiple of grid * grid", hipSuccess);
        return PROBAV_EINVAL;
    }
    const size_t lds = ens_reduce_lds(S);
    if (lds > AUG_LDS_LIMIT) {
        set_error("probav_ensemble_reduce: one prediction (S*S floats) and its accumulator must fit 64 KiB of LDS (S <= 90)", hipSuccess);
        return PROBAV_EINVAL;
    }
    EnsGeom g;
    g.V = V; g.S = S; g.rs = 3 + T; g.grid = grid; g.final_round = final_round ? 1 : 0; g.lo = lo; g.hi = hi;
    if (S % 4 == 0 && aug_aligned16(sr, out))
        hipLaunchKernelGGL(ensemble_reduce_kernel<4>, dim3((unsigned)n_base), dim3(AUG_THREADS), lds, (hipStream_t)stream, sr, recipe, g, out);
    else
        hipLaunchKernelGGL(ensemble_reduce_kernel<1>, dim3((unsigned)n_base), dim3(AUG_THREADS), lds, (hipStream_t)stream, sr, recipe, g, out);
    return check_launch("ensemble_reduce_kernel");
}
