// Device helpers shared by kernels_small.hip and kernels_loss.hip: the wavefront and workgroup sums, and the sign of the L1 derivatives.
#pragma once
#include <hip/hip_runtime.h>

namespace probav {

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// sign(e) of the L1 terms' derivatives: -1, 0, 1 -- and NaN for NaN.  `e > 0 ? 1 : (e < 0 ? -1 : 0)` calls a NaN zero: one NaN in a
// prediction made every e of its sample NaN, hence every sign and the whole gradient exactly 0 beside a NaN loss ('Non-finite values')
__device__ __forceinline__ double sign_keep_nan(double e) { return e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : (e == e ? 0.0 : e)); }
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the sum over a 256-thread workgroup, in every thread; red: four doubles of LDS
__device__ __forceinline__ double block_sum(double v, double* red, int tid)
{
    v = wave_sum(v);
    __syncthreads();                       // red may still be read by the previous reduction
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

}  // namespace probav
