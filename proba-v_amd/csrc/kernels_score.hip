// Scoring kernels (gfx950): the ESA PROBA-V shift-compensated clear PSNR (cPSNR) of whole images, the measure of the "Score" column
// of the reference's README.  evaluate.py and proba-v_amd/scoring.py drive them; they replace the unfinished evaluate.py:76-87 of the
// reference, which calls models/loss.py:37-53 (Losses.shiftCompensatedcPSNR).
//
// The metric.  Per image: SR (prediction) and HR (ground truth) uint16 S x S, M the clear mask of HR (nonzero = clear), border b.
// L = S - 2b, P = SR[b:b+L, b:b+L] (fixed crop).  For every shift (u, v) in [0, 2b]^2, row-major:
//     d = HR[u:u+L, v:v+L] - P (integers)      m = M[u:u+L, v:v+L]
//     n = sum m      s1 = sum m d      s2 = sum m d^2                    (exact integers)
//     cMSE(u, v) = (n s2 - s1^2) / n^2                                     (bias b = s1 / n folded in; raw 16-bit units)
//     cPSNR = 10 log10(65535^2 / min cMSE)                                 shift = the first (u, v) attaining the minimum
// This is the ESA / HighRes-net shift_cPSNR (HR normalised by 2^16 - 1, the reference's Losses.numBytes).  It differs from Losses only in
// that HR is masked too.  A shift with n = 0 is skipped; an image where every shift has n = 0 gets NaN (shift -1, -1); cMSE = 0 gives +inf.
//
// Exactness.  |d| <= 65535, so d^2 < 2^32 is one 24-bit multiply (|d| has 16 bits) zero-extended into a uint64 partial (written as
// (uint64_t)(a * a): with __umul24 the compiler sign-extended the product into the 64-bit sum, wrong for d^2 >= 2^31); a lane sums at most R * ceil(L / 64) <= 512 pixels per
// shift, so its s1 partial stays below 2^26 in int32; s2 partials are uint64.  The wave sums are widened to 64 bits and added into the
// image's moments with 64-bit INTEGER atomics: the moments are integers, so the result does not depend on the launch shape or the order.
// n s2 - s1^2 (up to ~9e19 at S = 384, past int64; >= 0 by Cauchy-Schwarz) is formed in unsigned __int128 from the 64-bit moments
// (n s2 < 2^76, s1^2 < 2^68 for S <= 2048).  Shifts are compared exactly: cMSE_a < cMSE_b  <=>  num_a n_b^2 < num_b n_a^2, each product
// < 2^120.  Only the winner is rounded: num to fp64 (hi * 2^64 + lo, relative error < 2^-51), divided by n^2 (exact in fp64), log10 in
// fp64 -- the cPSNR is within ~1e-13 dB of the exact value.
//
// Shape.  score_moments_kernel: one workgroup per (image, band of R crop rows), 2b + 1 waves, wave u owns shift row u.  The band's HR rows
// with their 2b halo are staged in LDS as words hr | (mask != 0) << 16, and its crop rows of SR as uint16.  Lane j walks the columns j,
// j + 64, ... of each crop row and slides v over the 2b + 1 neighbours in registers: per pixel-shift one ds_read_b32 and 7 VALU ops in the
// gfx950 code (v_sub_u32_sdwa, v_cmp, v_cndmask, v_add_u32_sdwa for n, v_add for s1, v_mul_i32_i24, v_lshl_add_u64 for s2).  score_select_kernel: one wave per image, serial exact
// selection in lane 0 (49 candidates).
//
// Cost model (S = 384, b = 3, 1 160 images): 49 shifts x 378^2 pixels x 1 160 = 8.1e9 pixel-shift visits, ~7 VALU ops each = 5.7e10 int
// ops, ~0.7 ms at the 78.6 Tops/s int32 VALU rate; the images as 16-bit (~0.9 GB with the halo re-reads) need ~0.15 ms of HBM.  The
// kernel was meant to be VALU-bound; tools/score_bench.py reports the measured time and its share of that bound.
// Measured on one MI355X: 1.95 ms for 1 160 images (1.68 us per image), 37 % of the VALU bound.  Why it lands there (reasoned from the
// code, not profiled): the model counts VALU only, but every pixel-shift also issues one ds_read_b32, 2 LDS cycles of a CU's one LDS for
// each wave-instruction.  Per crop pixel a wave spends ~56 VALU ops on its own SIMD and 7 reads = 14 LDS cycles, and the CU's four SIMDs
// share the LDS: ~56 LDS cycles per four waves, as much as the VALU work.  On top come the staging (halo re-reads, one division per
// staged SR pixel), a barrier per band and the 64-bit integer atomics of 147 moments per workgroup.
#include "probav_common.h"
#include "../../include/probav_hip.h"

namespace probav {

namespace {

constexpr int SCORE_MAX_S = 2048, SCORE_MAX_R = 16;
constexpr size_t SCORE_LDS_LIMIT = 64 * 1024;

inline size_t score_lds_bytes(int S, int border, int R)
{
    const int L = S - 2 * border;
    return (size_t)(R + 2 * border) * S * sizeof(uint32_t) + (((size_t)R * L * sizeof(uint16_t) + 15) & ~(size_t)15);
}

// rows of the crop per workgroup: the most (up to 16) whose staging fits 64 KiB of LDS; 0 if not even one row fits
inline int score_band_rows(int S, int border)
{
    int R = SCORE_MAX_R;
    while (R > 0 && score_lds_bytes(S, border, R) > SCORE_LDS_LIMIT) --R;
    return R;
}

template <int BD>
__global__ __launch_bounds__(64 * (2 * BD + 1)) void score_moments_kernel(const uint16_t* __restrict__ sr, const uint16_t* __restrict__ hr,
                                                                           const uint8_t* __restrict__ mask, int S, int R,
                                                                           unsigned long long* __restrict__ moments)
{
    constexpr int NS = 2 * BD + 1;
    extern __shared__ __align__(16) unsigned char score_smem[];
    const int L = S - 2 * BD;
    const int r0 = blockIdx.x * R, rows = min(R, L - r0), hrows = rows + 2 * BD;
    const int64_t img = blockIdx.y;
    uint32_t* w = reinterpret_cast<uint32_t*>(score_smem);                        // [hrows][S]
    uint16_t* p = reinterpret_cast<uint16_t*>(w + (size_t)(R + 2 * BD) * S);      // [rows][L]
    const size_t base = (size_t)img * S * S;
    const size_t hb = base + (size_t)r0 * S;                                      // HR rows r0 .. r0 + hrows - 1 (<= S - 1): contiguous
    for (int k = threadIdx.x; k < hrows * S; k += blockDim.x)
        w[k] = (uint32_t)hr[hb + k] | ((uint32_t)(mask[hb + k] != 0) << 16);
    for (int k = threadIdx.x; k < rows * L; k += blockDim.x) {
        const int i = k / L, j = k - i * L;
        p[k] = sr[base + (size_t)(r0 + BD + i) * S + BD + j];
    }
    __syncthreads();

    const int u = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int n[NS], s1[NS];
    uint64_t s2[NS];
#pragma unroll
    for (int v = 0; v < NS; ++v) { n[v] = 0; s1[v] = 0; s2[v] = 0; }
    for (int i = 0; i < rows; ++i) {
        const uint32_t* wr = w + (i + u) * S;
        const uint16_t* pr = p + i * L;
        for (int j = lane; j < L; j += 64) {
            const int pv = pr[j];
#pragma unroll
            for (int v = 0; v < NS; ++v) {
                const uint32_t x = wr[j + v];
                const int mm = (int)(x >> 16);
                const int d = mm ? (int)(x & 0xffffu) - pv : 0;
                const unsigned a = (unsigned)abs(d);
                n[v] += mm;
                s1[v] += d;
                s2[v] += (uint64_t)(a * a);                                  // < 2^32: a has 16 bits
            }
        }
    }
    // wave sums (64-bit) -> the image's moments [nshift][3], integer atomics (two's complement for s1)
#pragma unroll
    for (int v = 0; v < NS; ++v) {
        long long a = n[v], b = s1[v];
        unsigned long long c = s2[v];
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_xor(a, o, 64);
            b += __shfl_xor(b, o, 64);
            c += __shfl_xor(c, o, 64);
        }
        if (lane == 0) {
            unsigned long long* m = moments + ((size_t)img * NS * NS + u * NS + v) * 3;
            atomicAdd(m + 0, (unsigned long long)a);
            atomicAdd(m + 1, (unsigned long long)b);
            atomicAdd(m + 2, c);
        }
    }
}

__device__ __forceinline__ double u128_to_double(unsigned __int128 x)
{
    return (double)(uint64_t)(x >> 64) * 18446744073709551616.0 + (double)(uint64_t)x;
}

// one wave per image: exact first minimum of cMSE over the shifts, then the fp64 outputs of the winner
__global__ __launch_bounds__(64) void score_select_kernel(const int64_t* __restrict__ moments, int nshift, int ns, double* __restrict__ cpsnr,
                                                          int32_t* __restrict__ shift, double* __restrict__ bias, int64_t* __restrict__ n_clear)
{
    if (threadIdx.x != 0) return;
    const int64_t img = blockIdx.x;
    const int64_t* m = moments + (size_t)img * nshift * 3;
    int best = -1;
    unsigned __int128 bnum = 0, bn2 = 1;
    for (int k = 0; k < nshift; ++k) {
        const int64_t n = m[3 * k], s1 = m[3 * k + 1];
        const uint64_t s2 = (uint64_t)m[3 * k + 2];
        if (n <= 0) continue;
        const uint64_t as1 = (uint64_t)(s1 < 0 ? -s1 : s1);
        const unsigned __int128 num = (unsigned __int128)(uint64_t)n * s2 - (unsigned __int128)as1 * as1;
        const unsigned __int128 n2 = (unsigned __int128)((uint64_t)n * (uint64_t)n);
        if (best < 0 || num * bn2 < bnum * n2) { best = k; bnum = num; bn2 = n2; }
    }
    if (best < 0) {
        const double nan = __builtin_nan("");
        cpsnr[img] = nan; bias[img] = nan; n_clear[img] = 0;
        shift[2 * img] = -1; shift[2 * img + 1] = -1;
        return;
    }
    const int64_t n = m[3 * best], s1 = m[3 * best + 1];
    const double cmse = u128_to_double(bnum) / (double)((uint64_t)n * (uint64_t)n);
    cpsnr[img] = bnum == 0 ? __builtin_inf() : 10.0 * log10(65535.0 * 65535.0 / cmse);
    bias[img] = (double)s1 / (double)n;
    n_clear[img] = n;
    shift[2 * img] = best / ns;
    shift[2 * img + 1] = best % ns;
}

template <int BD>
int launch_moments(const uint16_t* sr, const uint16_t* hr, const uint8_t* mask, int64_t N, int S, int R, int64_t* moments, hipStream_t s)
{
    const int L = S - 2 * BD, bands = (L + R - 1) / R;
    hipLaunchKernelGGL(score_moments_kernel<BD>, dim3((unsigned)bands, (unsigned)N), dim3(64 * (2 * BD + 1)), score_lds_bytes(S, BD, R), s, sr, hr,
                       mask, S, R, reinterpret_cast<unsigned long long*>(moments));
    return check_launch("score_moments_kernel");
}

}  // namespace

}  // namespace probav

using namespace probav;

extern "C" int probav_score_moments(const uint16_t* sr, const uint16_t* hr, const uint8_t* mask, int64_t n_images, int S, int border,
                                    int64_t* moments, void* stream)
{
    if (!sr || !hr || !mask || !moments || n_images < 1 || n_images > 65535 || border < 0 || border > 3 || S <= 2 * border ||
        S > SCORE_MAX_S) {
        set_error("probav_score_moments: null/invalid argument (1 <= n_images <= 65535, 0 <= border <= 3, 2 border < S <= 2048)", hipSuccess);
        return PROBAV_EINVAL;
    }
    const int R = score_band_rows(S, border);
    if (R < 1) { set_error("probav_score_moments: image too wide for the LDS staging", hipSuccess); return PROBAV_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const int ns = 2 * border + 1;
    hipError_t e = hipMemsetAsync(moments, 0, (size_t)n_images * ns * ns * 3 * sizeof(int64_t), s);
    if (e != hipSuccess) { set_error("probav_score_moments: hipMemsetAsync", e); return PROBAV_EHIP; }
    switch (border) {
        case 0: return launch_moments<0>(sr, hr, mask, n_images, S, R, moments, s);
        case 1: return launch_moments<1>(sr, hr, mask, n_images, S, R, moments, s);
        case 2: return launch_moments<2>(sr, hr, mask, n_images, S, R, moments, s);
        default: return launch_moments<3>(sr, hr, mask, n_images, S, R, moments, s);
    }
}

extern "C" int probav_score_select(const int64_t* moments, int64_t n_images, int border, double* cpsnr, int32_t* shift, double* bias,
                                   int64_t* n_clear, void* stream)
{
    if (!moments || !cpsnr || !shift || !bias || !n_clear || n_images < 1 || n_images > 0x7fffffff || border < 0 || border > 3) {
        set_error("probav_score_select: null/invalid argument", hipSuccess);
        return PROBAV_EINVAL;
    }
    const int ns = 2 * border + 1;
    hipLaunchKernelGGL(score_select_kernel, dim3((unsigned)n_images), dim3(64), 0, (hipStream_t)stream, moments, ns * ns, ns, cpsnr, shift, bias, n_clear);
    return check_launch("score_select_kernel");
}
