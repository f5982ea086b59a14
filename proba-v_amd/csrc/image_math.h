// The integer image arithmetic the inference kernels share: the clip and round of a prediction, the half-to-even integer mean and the
// 4-wide / 1-wide launch of kernels_tile.hip and kernels_windows.hip.  proba-v_amd/intmath.py states the two functions in numpy.
#pragma once
#include <type_traits>
#include "probav_common.h"

namespace probav {

namespace {

struct alignas(16) Vec4f { float v[4]; };

// probav_clip_round's arithmetic: clip to [lo, hi], round half to even.  fmaxf drops a NaN, so NaN -> lo ('Non-finite values')
__device__ __forceinline__ float clip_rint(float x, float lo, float hi)
{
    return rintf(fminf(fmaxf(x, lo), hi));
}

// N / D rounded half to even in 64-bit integers, D > 0: q = floor(N / D), r = N - q D, q + 1 when 2 r > D or when 2 r == D and q is odd
__device__ __forceinline__ float round_div_half_even(long long N, long long D)
{
    long long q = N / D, r = N % D;     // C++ truncates, the definition floors
    if (r < 0) { r += D; q -= 1; }
    if (2 * r > D || (2 * r == D && (q & 1))) q += 1;
    return (float)q;
}

// One thread per group of 4 consecutive pixels (16-byte loads and stores) when the caller's sizes are `divisible` by 4 and both arrays are
// 16-byte aligned, per pixel otherwise.  launch(width, blocks, groups) starts the kernel's instance of that width (an
// std::integral_constant<int, 4 or 1>); more than 2^31 - 1 blocks are refused with the caller's message.
template <int THREADS, typename Launch>
inline int launch_pixel_groups(bool divisible, const void* in, const void* out, size_t pixels, const char* too_many, const char* name, Launch launch)
{
    const bool vec = divisible && (reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
    const size_t groups = vec ? pixels / 4 : pixels;
    const size_t blocks = (groups + THREADS - 1) / THREADS;
    if (blocks > 0x7fffffff) {
        set_error(too_many, hipSuccess);
        return PROBAV_EINVAL;
    }
    if (vec) launch(std::integral_constant<int, 4>(), (unsigned)blocks, groups);
    else launch(std::integral_constant<int, 1>(), (unsigned)blocks, groups);
    return check_launch(name);
}

}  // namespace

}  // namespace probav
