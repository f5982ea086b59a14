// Bicubic-mean baseline (gfx950): every LR frame of an image set upscaled 3 x by the Keys cubic and the chosen frames averaged -- the
// number every PROBA-V result is quoted against.  It replaces the reference's unfinished bicubicMean / padding (evaluate.py:142-197) and the
// baseline upscaling of utils/utils.py:534-586; the statement the kernel equals bit for bit is probav_amd.baseline.baseline_numpy.
//
// The statement.  Keys cubic, a = -1/2, half-pixel centres, scale 3: HR index Y sits at the LR coordinate (Y - 1) / 3, so with
// i0 = floor((Y - 1) / 3) and the phase ph = (Y - 1) mod 3 it reads the rows clamp(i0 - 1 .. i0 + 2, 0, H - 1) with the weights over 27
//     ph 0: (0, 27, 0, 0)      ph 1: (-2, 21, 9, -1)      ph 2: (-1, 9, 21, -2)
// and columns likewise: U_f[Y][X] = sum_ij wy_i wx_j p_f[row_i][col_j], an integer over 729.  N = sum over the chosen frames of U_f,
// D = 729 K, out = clip(N / D rounded half to even, 0, 65535).  esa mode chooses the frames whose clear count equals the set's largest
// (K per set); clear mode chooses, per HR pixel, the frames that are clear at LR pixel (Y / 3, X / 3), or all of them where none is.
//
// The sum is taken before the upscale.  U is linear with integer weights and the choice of frames is the same for the nine HR pixels of
// one LR pixel (r, c) -- they all read LR rows r - 2 .. r + 2 and columns c - 2 .. c + 2 (Y = 3 r has i0 = r - 1 at phase 2, Y = 3 r + 1
// has i0 = r at phase 0, Y = 3 r + 2 has i0 = r at phase 1) -- so
//     N[3 r + y][3 c + x] = sum_ij wy_i wx_j S_ij(r, c),     S_ij(r, c) = sum over the frames chosen at (r, c) of p_f[clamp(r + i)][clamp(c + j)]
// exactly, in integers: the same terms in another order.  Per frame a thread therefore only ADDS its 5 x 5 neighbourhood into 25 sums
// (clear mode: S += p * clear, one 24-bit multiply-add each), and the two separable passes, the division and the clip run once per set.
// In esa mode the chosen frames are the same for every pixel, S_ij(r, c) is the plain total T[r + i][c + j], and a frame costs one add
// per pixel.  In clear mode T is kept as well: where no frame is clear at (r, c) every S_ij(r, c) is still 0 and the statement's
// fallback to all frames is S_ij = T[r + i][c + j].
//
// Exactness.  Every value is an integer.  A sum of at most 4096 uint16 samples is below 2^28: S and T are uint32.  The row pass gives
// |h| <= 33 * 2^28 and the column pass |N| <= 1089 * 4096 * 65535 < 2^39: both passes run in int64 (35 frames at the largest overshoot,
// 35 * 65535 * 1089, already pass 2^31).  The division: |N / D| <= 65535 * 1089 / 729 < 2^17, so N' = N + 2^17 D is non-negative and
// floor(N' / D) = floor(N / D) + 2^17 with the same remainder; D = 729 K, and for positive divisors floor(floor(N' / 729) / K) =
// floor(N' / (729 K)), where floor(N' / 729) < 4096 * (2^17 + 2^17) = 2^30 is a uint32: one 64-bit division by the constant 729, one
// 32-bit division by K, the remainder N' - q' D formed exactly and compared against D, ties to even.  No floating-point value and no
// atomic takes part in the result: the image does not depend on the grid, the band height or the order of the frames.
//
// Shape.  A workgroup owns a band of BL = 8 LR rows (24 HR rows) by TW = 128 LR columns of one set; a thread owns one LR pixel of it,
// i.e. a 3 x 3 block of HR pixels.  The band needs the (BL + 4) x (TW + 4) window of LR samples, halo of 2 included, indices clamped; its
// 1584 elements are dealt to the 1024 threads once (element e to thread e mod 1024: the clamped source offset is the same in every
// frame), and the owner of an element fetches it from every chosen frame and keeps its total T in a register.  Each LR pixel of a
// chosen frame is thus fetched once per band, plus the halo; in esa mode frames that are not chosen are skipped before anything of
// them is fetched (wave 0 lists the chosen frames in LDS first, in frame order), and nothing else happens per frame: no LDS, no barrier.
// A frame's work is far shorter than a trip to memory, so the loop fetches BSL_AHEAD frames' elements (and clear bytes) into registers
// before it uses the first of them (8 in esa mode, 4 in clear mode, whose 25 sums need the registers).  In clear mode the fetched window
// also goes to LDS (one sample per dword, 6.3 KB; two buffers, so one barrier per frame) and every thread adds its 5 x 5 neighbourhood,
// times its clear flag, into its 25 sums (a wave reads 64 consecutive dwords of a row per step: no bank conflict, and no read straddles
// a dword; a sample below 2^16 times 0 / 1 is one 24-bit multiply-add).  The clear byte of
// (f, r, c) has exactly one reader, the thread that owns (r, c): it is read straight into that thread's register (a wave reads 64
// consecutive bytes), not through LDS.  At the end the totals go to LDS once (the window of T), every thread runs the two passes on its
// 25 sums, and the nine results go through LDS (24 x 384 fp32; lane stride 3 dwords: no conflict) so that the band is written as whole
// rows of consecutive fp32.
//
// The per-frame clear counts are one launch of prep_count_kernel (probav_prep_count_nonzero) into the caller's scratch; every workgroup of
// a set then finds the set's maximum and K itself from at most 4096 int32 (L2-resident): nothing comes back to the host.
#include "probav_common.h"
#include "../../include/probav_hip.h"

namespace probav {

namespace {

constexpr int BSL_BL = 8, BSL_TW = 128, BSL_THREADS = BSL_BL * BSL_TW, BSL_WAVES = BSL_THREADS / 64;
constexpr int BSL_WR = BSL_BL + 4, BSL_WC = BSL_TW + 4;               // the staged window: halo of 2 on every side
constexpr int BSL_MAX_FRAMES = 4096, BSL_MAX_HR = 1 << 20;

__device__ __forceinline__ int bsl_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// the three HR samples between LR positions: p0 .. p4 are positions c - 2 .. c + 2 -> (X = 3 c, 3 c + 1, 3 c + 2), each over 27
__device__ __forceinline__ void bsl_pass(long long p0, long long p1, long long p2, long long p3, long long p4, long long& a, long long& b, long long& c)
{
    a = -p0 + 9 * p1 + 21 * p2 - 2 * p3;                   // phase 2 from i0 = c - 1
    b = 27 * p2;                                           // phase 0
    c = -2 * p1 + 21 * p2 + 9 * p3 - p4;                   // phase 1 from i0 = c
}

// N / (729 K) rounded half to even, 1 <= K <= 4096, |N| <= 1089 * 65535 * K; clipped to [0, 65535]
// (not image_math.h's round_div_half_even: a narrower algorithm, unsigned 32-bit steps with the fixed divisor 729 taken first)
__device__ __forceinline__ float bsl_mean(long long N, unsigned K)
{
    const unsigned D = 729u * K;                           // < 2^22
    const unsigned long long Np = (unsigned long long)(N + ((long long)D << 17));     // >= 0: |N / D| < 2^17
    const unsigned q1 = (unsigned)(Np / 729u);             // < 2^30
    const unsigned qp = q1 / K;                            // floor(N / D) + 2^17
    const unsigned r = (unsigned)(Np - (unsigned long long)qp * D);                   // 0 <= r < D
    int q = (int)qp - (1 << 17);
    if (2 * r > D || (2 * r == D && (q & 1))) q += 1;
    q = q < 0 ? 0 : (q > 65535 ? 65535 : q);
    return (float)q;                                       // an integer below 2^16: exact
}

template <int MODE>
__global__ __launch_bounds__(BSL_THREADS) void baseline_upscale_mean_kernel(const uint16_t* __restrict__ frames, const uint8_t* __restrict__ clear,
                                                                            const int64_t* __restrict__ set_offsets, int n_sets, int64_t n_frames,
                                                                            int H, int W, int n_bands, int n_ctiles,
                                                                            const int32_t* __restrict__ counts, float* __restrict__ out,
                                                                            int32_t* __restrict__ k_used)
{
    __shared__ unsigned win[2][BSL_WR * BSL_WC];          // clear mode: the window of the frame at hand, one sample per dword
    __shared__ unsigned tot[BSL_WR * BSL_WC];              // the window of totals T, once at the end
    __shared__ float stage[3 * BSL_BL * 3 * BSL_TW];
    __shared__ int red[BSL_WAVES];
    __shared__ uint16_t sel[BSL_MAX_FRAMES];               // esa mode: the chosen frames of the set

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ct = blockIdx.x % n_ctiles, band = (blockIdx.x / n_ctiles) % n_bands, s = blockIdx.x / (n_ctiles * n_bands);
    const int64_t f0 = set_offsets[s], f1 = set_offsets[s + 1];
    const bool first = band == 0 && ct == 0 && tid == 0;   // the one thread that reports the set's K
    if (!(set_offsets[0] == 0 && set_offsets[n_sets] == n_frames && f0 >= 0 && f1 > f0 && f1 - f0 <= BSL_MAX_FRAMES && f1 <= n_frames)) {
        if (first) k_used[s] = PROBAV_BASELINE_BAD_SET;    // violated precondition: nothing read, the set's image not written
        return;
    }
    const int nf = (int)(f1 - f0);

    int cmax = 0, K = nf;
    if (MODE == PROBAV_BASELINE_ESA) {                     // the set's largest clear count, then how many frames attain it
        for (int i = tid; i < nf; i += BSL_THREADS) cmax = max(cmax, counts[f0 + i]);
        for (int o = 32; o > 0; o >>= 1) cmax = max(cmax, __shfl_xor(cmax, o, 64));
        if (lane == 0) red[wave] = cmax;
        __syncthreads();
        for (int k = 0; k < BSL_WAVES; ++k) cmax = max(cmax, red[k]);
        __syncthreads();
        if (wave == 0) {                                   // the chosen frames, in frame order, as a list: the loop below fetches several ahead
            int n = 0;
            for (int i0 = 0; i0 < nf; i0 += 64) {
                const int i = i0 + lane;
                const bool pick = i < nf && counts[f0 + i] == cmax;
                const unsigned long long m = __ballot(pick);
                if (pick) sel[n + __popcll(m & ((1ull << lane) - 1))] = (uint16_t)i;
                n += __popcll(m);
            }
            if (lane == 0) red[0] = n;
        }
        __syncthreads();
        K = red[0];
    }
    if (first) k_used[s] = K;

    const int r0 = band * BSL_BL, c0 = ct * BSL_TW;        // the band's first LR row / column
    const int lr = tid / BSL_TW, lc = tid % BSL_TW;        // this thread's LR pixel inside the band
    const int r = r0 + lr, c = c0 + lc;
    const bool live = r < H && c < W;
    const size_t HW = (size_t)H * W;

    // the window elements this thread fetches from every frame: e0 = tid and e1 = tid + 1024 (the first 560 threads)
    constexpr int E1 = BSL_WR * BSL_WC - BSL_THREADS;
    const int e1 = tid + BSL_THREADS;
    const bool has1 = tid < E1;
    const size_t off0 = (size_t)bsl_clamp(r0 - 2 + tid / BSL_WC, H) * W + bsl_clamp(c0 - 2 + tid % BSL_WC, W);
    const size_t off1 = has1 ? (size_t)bsl_clamp(r0 - 2 + e1 / BSL_WC, H) * W + bsl_clamp(c0 - 2 + e1 % BSL_WC, W) : off0;
    const size_t offc = live ? (size_t)r * W + c : 0;
    unsigned t0 = 0, t1 = 0;                               // totals of those two elements over the chosen frames (clear mode: all frames)
    unsigned S[25];                                        // clear mode: S[5 j + i] = sum of p[r - 2 + j][c - 2 + i] over the frames clear at (r, c)
#pragma unroll
    for (int k = 0; k < 25; ++k) S[k] = 0;
    unsigned kc = 0;                                       // clear mode: how many frames are clear at (r, c)

    // BSL_AHEAD frames are fetched before the first of them is used: one frame's work is far shorter than a trip to memory
    int buf = 0;
    constexpr int BSL_AHEAD = MODE == PROBAV_BASELINE_ESA ? 8 : 4;
    for (int base = 0; base < K; base += BSL_AHEAD) {      // K: the chosen frames (clear mode: all nf)
        unsigned v0[BSL_AHEAD], v1[BSL_AHEAD], cl[BSL_AHEAD];
#pragma unroll
        for (int g = 0; g < BSL_AHEAD; ++g) {
            v0[g] = v1[g] = cl[g] = 0;
            if (base + g < K) {                            // uniform over the workgroup
                const size_t f = (size_t)f0 + (MODE == PROBAV_BASELINE_ESA ? (int)sel[base + g] : base + g);
                const uint16_t* p = frames + f * HW;
                v0[g] = p[off0];
                v1[g] = p[off1];
                if (MODE == PROBAV_BASELINE_CLEAR && live) cl[g] = clear[f * HW + offc] != 0;
            }
        }
#pragma unroll
        for (int g = 0; g < BSL_AHEAD; ++g) {
            t0 += v0[g];
            t1 += v1[g];
            if (MODE == PROBAV_BASELINE_CLEAR && base + g < K) {
                unsigned* wl = win[buf];
                wl[tid] = v0[g];
                if (has1) wl[e1] = v1[g];
                __syncthreads();                           // (the other buffer is still being read by slower waves: two buffers, one barrier)
                const unsigned* row = wl + lr * BSL_WC + lc;
#pragma unroll
                for (int j = 0; j < 5; ++j)
#pragma unroll
                    for (int x = 0; x < 5; ++x) S[5 * j + x] += __umul24(row[j * BSL_WC + x], cl[g]);      // a sample below 2^16 times 0 / 1
                kc += cl[g];
                buf ^= 1;
            }
        }
    }

    tot[tid] = t0;
    if (has1) tot[e1] = t1;
    __syncthreads();
    if (live) {
        unsigned Kp = (unsigned)K;                         // this pixel's K
        if (MODE == PROBAV_BASELINE_CLEAR && kc > 0) Kp = kc;
        const bool from_totals = MODE == PROBAV_BASELINE_ESA || kc == 0;      // esa: every pixel; clear: the fallback to all frames
        long long h[5][3];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const unsigned* trow = tot + (lr + j) * BSL_WC + lc;
            long long q[5];
#pragma unroll
            for (int x = 0; x < 5; ++x) q[x] = from_totals ? trow[x] : S[5 * j + x];
            bsl_pass(q[0], q[1], q[2], q[3], q[4], h[j][0], h[j][1], h[j][2]);
        }
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            long long u[3];                                // u[y]: N at HR pixel (3 r + y, 3 c + x)
            bsl_pass(h[0][x], h[1][x], h[2][x], h[3][x], h[4][x], u[0], u[1], u[2]);
#pragma unroll
            for (int y = 0; y < 3; ++y) stage[(3 * lr + y) * (3 * BSL_TW) + 3 * lc + x] = bsl_mean(u[y], Kp);
        }
    }
    __syncthreads();
    const int H3 = 3 * H, W3 = 3 * W;
    float* o = out + (size_t)s * H3 * W3;
    for (int e = tid; e < 3 * BSL_BL * 3 * BSL_TW; e += BSL_THREADS) {
        const int y = e / (3 * BSL_TW), x = e % (3 * BSL_TW);
        const int Y = 3 * r0 + y, X = 3 * c0 + x;
        if (Y < H3 && X < W3) o[(size_t)Y * W3 + X] = stage[e];
    }
}

}  // namespace

}  // namespace probav

using namespace probav;

extern "C" int probav_baseline_upscale_mean(const uint16_t* frames, const uint8_t* clear, const int64_t* set_offsets, int n_sets, int64_t n_frames, int H,
                                            int W, int scale, int mode, int32_t* counts_scratch, float* out, int32_t* k_used, void* stream)
{
    if (!frames || !clear || !set_offsets || !counts_scratch || !out || !k_used || n_sets < 1 || n_frames < 1 || n_frames > 0x7fffffff) {
        set_error("probav_baseline_upscale_mean: null/invalid argument", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (scale != 3) {
        set_error("probav_baseline_upscale_mean: scale must be 3 (the integer weights over 27 are those of scale 3)", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (mode != PROBAV_BASELINE_ESA && mode != PROBAV_BASELINE_CLEAR) {
        set_error("probav_baseline_upscale_mean: mode must be PROBAV_BASELINE_ESA or PROBAV_BASELINE_CLEAR", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (H < 1 || W < 1 || 3 * (int64_t)H > BSL_MAX_HR || 3 * (int64_t)W > BSL_MAX_HR) {
        set_error("probav_baseline_upscale_mean: H, W must be at least 1 and 3 H, 3 W at most 2^20", hipSuccess);
        return PROBAV_EINVAL;
    }
    const int n_bands = (H + BSL_BL - 1) / BSL_BL, n_ctiles = (W + BSL_TW - 1) / BSL_TW;
    const int64_t blocks = (int64_t)n_sets * n_bands * n_ctiles;
    if (blocks > 0x7fffffff) {
        set_error("probav_baseline_upscale_mean: more than 2^31 - 1 bands in one call", hipSuccess);
        return PROBAV_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    if (mode == PROBAV_BASELINE_ESA) {
        const int rc = probav_prep_count_nonzero(clear, n_frames, (int64_t)H * W, counts_scratch, stream);
        if (rc != PROBAV_OK) return rc;
        hipLaunchKernelGGL(baseline_upscale_mean_kernel<PROBAV_BASELINE_ESA>, dim3((unsigned)blocks), dim3(BSL_THREADS), 0, s, frames, clear, set_offsets,
                           n_sets, n_frames, H, W, n_bands, n_ctiles, (const int32_t*)counts_scratch, out, k_used);
    } else {
        hipLaunchKernelGGL(baseline_upscale_mean_kernel<PROBAV_BASELINE_CLEAR>, dim3((unsigned)blocks), dim3(BSL_THREADS), 0, s, frames, clear, set_offsets,
                           n_sets, n_frames, H, W, n_bands, n_ctiles, (const int32_t*)counts_scratch, out, k_used);
    }
    return check_launch("baseline_upscale_mean_kernel");
}
