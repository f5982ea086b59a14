// Frame-window ensemble (gfx950): the device-side frame choice that writes the network inputs of all W windows of a tile, and the weighted
// integer mean of the W predictions.  proba-v_amd/frame_windows.py states both in numpy (frame_windows_select_numpy / _gather_numpy /
// _reduce_numpy) and testClass.resolve_windowed drives them; INTEGRATION.md, 'Frame windows', has the definition.
//
// Gather.  patches [N][T_pre][win][win] fp32 and counts [N][T_pre] int32 (masked pixels of every frame of the tile, 0 .. pixels = win^2)
// are the dataset builder's unfold (probav_prep_patches).  Per tile: frame t is eligible iff counts[t] < L (all T_pre frames when none is);
// the E eligible frames ordered by (count, index) are r[0 .. E); m = ceil(k / E); Q[i] = r[i / m], i < E m (the builder's tiled, sorted
// list); window j < W takes Q[(j step + i) % (E m)], i < k ((W - 1) step + k <= T_pre unless W = 1: a single window is the builder's own choice,
// which tiles a pool shorter than k).  x [N][W][win][win][k] receives the frames of every window with the frame index
// innermost (test.py's transpose), sel [N][W][k] the chosen frame indices, weight [N][W] the sum over the window's frames of
// (pixels - count) (mode 0, "clear") or 1 (mode 1, "uniform"); a tile whose weights are all 0 gets all 1.
//
// One workgroup of 256 threads per tile.  Wave 0 ranks: lane t < T_pre (T_pre <= 64) holds counts[t], one ballot gives the eligible set and
// a loop of T_pre shuffles counts the eligible u with (c_u, u) < (c_t, t); no sort network.  It leaves Q and the counts of Q in LDS, then
// writes `weight`.  Meanwhile all four waves stage the tile's T_pre win^2 floats in LDS, once, with 16-byte global loads where the tile
// base is 16-byte aligned (scalar loads for an unaligned view).  After one barrier every window is written from LDS: thread e of a window's
// win^2 k outputs reads plane Q[.] at pixel e / k, so a wave stores 64 consecutive floats and (e / k, e % k) advance by additions.
//
// LDS layout: float plane[T_pre][PS] and nothing else dynamic; static: int Qf[128], Qc[128] (E m < k + E <= 128: k <= 64) and E m.
// PS = fw_plane_stride(win^2): win^2 plus 0 .. 3 dwords of padding, the smallest stride whose residue mod 32 is not one of
// {0, 8, 16, 24, 1, 31, 11, 21}.  Dynamic LDS = 4 T_pre PS bytes exactly (22 x 22: PS = 484, 36 784 B at T_pre = 19; 44 x 44: PS = 1937,
// 162 708 B at T_pre = 21).  Why: the window reads are ds_read_b32 (32 banks, conflicts within 32-lane groups); a group covers 32 consecutive
// (pixel, i) pairs, ceil(31 / k) + 1 pixels at the most, and lane (p, i) reads dword f_i PS + p, bank (f_i r + p) mod 32 with r = PS mod 32.
// Two lanes meet on a bank iff r (f - f') == p' - p (mod 32) with |p' - p| <= 4.  r = 0 puts the k planes of one pixel on ONE bank (k-way),
// 16 / 8 / 24 every second / fourth plane; r = 1, 31 make neighbouring frames meet at neighbouring pixels, r = 11, 21 frames three apart
// (3 r == +-1).  Equal frames (a wrapped window) read one address, a broadcast.  Counted with that bank rule over random frame sets
// (k = 9, T_pre = 9 .. 19, the busiest bank of every group): 2.0 .. 2.5 distinct addresses on average at the admitted residues (the chosen
// frames are arbitrary, so no stride reaches 1), against 9 at r = 0, 5.4 at r = 16 (the unpadded 44 x 44 plane), 3.0 .. 4.2 at the other six.
// The staging writes are consecutive dwords within a plane (conflict-free).
//
// Reduce.  sr [N W][S][S] raw predictions or rounded members, weight [N][W] non-negative int32 with a positive sum per tile;
// p = rint(clip(sr, lo, hi)); out[n][px] = (sum_j w_j p_j) / (sum_j w_j) rounded half to even in 64-bit integers.  One thread per 4 pixels
// (16-byte loads and stores) when S^2 is a multiple of 4 and the arrays are 16-byte aligned, per pixel otherwise.  No atomics, no float after
// the rint.  w < 2^31, p <= 2^24 and W <= 64 keep the sums below 2^61 (what the gather writes: w <= k pixels, so below 2^46 at the shipped sizes).
#include "probav_common.h"
#include "image_math.h"
#include "../../include/probav_hip.h"

namespace probav {

namespace {

constexpr int FW_THREADS = 256;
constexpr int FW_MAX_T = 64;            // one lane per frame in the ranking wave
constexpr int FW_MAX_W = 64;
constexpr int FW_MAX_Q = 2 * FW_MAX_T;  // E m < k + E, k <= 64, E <= T_pre <= 64
constexpr size_t FW_STATIC_LDS = 2 * FW_MAX_Q * sizeof(int) + 16;   // Qf, Qc and E m (rounded up): the gather kernel's static LDS

struct FwGeom {
    int T, win, px, PS, k, L, W, step, mode;    // px = win^2, PS = the LDS plane stride in floats
    int vec;                                    // the tile bases are 16-byte aligned and a tile is a whole number of float4
};

// the LDS plane stride in floats (the header comment has the reasoning): the smallest PS >= px with PS mod 32 outside {0, 1, 8, 11, 16, 21, 24, 31}
inline int64_t fw_plane_stride(int64_t px)
{
    const uint32_t bad = (1u << 0) | (1u << 1) | (1u << 8) | (1u << 11) | (1u << 16) | (1u << 21) | (1u << 24) | (1u << 31);
    while ((bad >> (px & 31)) & 1u) ++px;
    return px;
}

__global__ __launch_bounds__(FW_THREADS) void frame_windows_gather_kernel(const float* __restrict__ patches, const int32_t* __restrict__ counts, FwGeom g,
                                                                          float* __restrict__ x, int32_t* __restrict__ weight, int32_t* __restrict__ sel)
{
    extern __shared__ float plane[];                                 // [T][PS]
    __shared__ int Qf[FW_MAX_Q], Qc[FW_MAX_Q], EmS;
    const size_t n = blockIdx.x;
    const int tid = threadIdx.x;

    if (tid < 64) {                                                  // wave 0: rank the frames, build Q
        const int t = tid;
        const int c = t < g.T ? counts[n * g.T + t] : 0;
        unsigned long long elig = __ballot(t < g.T && c < g.L);
        if (elig == 0ull) elig = g.T == 64 ? ~0ull : ((1ull << g.T) - 1ull);
        const int E = __popcll(elig);
        const int m = (g.k + E - 1) / E, Em = E * m;
        int rank = 0;
        for (int u = 0; u < g.T; ++u) {
            const int cu = __shfl(c, u, 64);
            if (((elig >> u) & 1ull) && (cu < c || (cu == c && u < t))) ++rank;
        }
        if ((elig >> t) & 1ull) {                                    // rank < E: the m copies of frame t sit at Q[rank m .. rank m + m)
            for (int q = 0; q < m; ++q) { Qf[rank * m + q] = t; Qc[rank * m + q] = c; }
        }
        if (t == 0) EmS = Em;
    }

    // stage the tile: T px contiguous floats -> plane[f][p]
    const float* src = patches + n * (size_t)g.T * g.px;
    const int total = g.T * g.px;
    if (g.vec) {
        for (int q = tid * 4; q < total; q += FW_THREADS * 4) {
            const Vec4f in = *reinterpret_cast<const Vec4f*>(src + q);
            int f = q / g.px, p = q - f * g.px;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                plane[f * g.PS + p] = in.v[j];
                if (++p == g.px) { p = 0; ++f; }
            }
        }
    } else {
        for (int q = tid; q < total; q += FW_THREADS) {
            const int f = q / g.px, p = q - f * g.px;
            plane[f * g.PS + p] = src[q];
        }
    }
    __syncthreads();
    const int Em = EmS;

    if (tid < 64) {                                                  // wave 0: the weights
        int w = 0;
        if (tid < g.W) {
            if (g.mode == 1) {
                w = 1;
            } else {
                int idx = (int)(((long long)tid * g.step) % Em);
                for (int i = 0; i < g.k; ++i) {
                    w += g.px - Qc[idx];
                    if (++idx == Em) idx = 0;
                }
            }
        }
        if (__ballot(tid < g.W && w != 0) == 0ull) w = 1;
        if (tid < g.W) weight[n * g.W + tid] = w;
    }
    for (int q = tid; q < g.W * g.k; q += FW_THREADS) {
        const int j = q / g.k, i = q - j * g.k;
        sel[n * (size_t)g.W * g.k + q] = Qf[(int)(((long long)j * g.step + i) % Em)];
    }

    // the windows: element e = pixel * k + i of window j reads plane Q[(j step + i) % Em] at `pixel`
    const int per = g.px * g.k;
    const int dp = FW_THREADS / g.k, di = FW_THREADS - dp * g.k;     // e += 256  ->  (pixel, i) += (dp, di) with one carry
    const int p0 = tid / g.k, i0 = tid - p0 * g.k;
    for (int j = 0; j < g.W; ++j) {
        const int base = (int)(((long long)j * g.step) % Em);
        float* dst = x + (n * g.W + j) * (size_t)per;
        int p = p0, i = i0;
        for (int e = tid; e < per; e += FW_THREADS) {
            int idx = base + i;                                      // i < k <= Em: one wrap at most
            if (idx >= Em) idx -= Em;
            dst[e] = plane[Qf[idx] * g.PS + p];
            p += dp; i += di;
            if (i >= g.k) { i -= g.k; ++p; }
        }
    }
}

// a precondition broken by the caller (weights with no positive sum) gives 0: no division by zero
__device__ __forceinline__ float fw_mean(long long N, long long D) { return D <= 0 ? 0.f : round_div_half_even(N, D); }

template <int Wd>
__global__ __launch_bounds__(FW_THREADS) void frame_windows_reduce_kernel(const float* __restrict__ sr, const int32_t* __restrict__ weight, int W, size_t SS,
                                                                          size_t groups, float lo, float hi, float* __restrict__ out)
{
    const size_t q = (size_t)blockIdx.x * FW_THREADS + threadIdx.x;
    if (q >= groups) return;
    const size_t e = q * Wd, n = e / SS, px = e - n * SS;          // Wd == 4 only when SS % 4 == 0: the group lies in one tile
    const float* src = sr + n * W * SS + px;
    const int32_t* w = weight + n * W;
    long long N[Wd], D = 0;
#pragma unroll
    for (int j = 0; j < Wd; ++j) N[j] = 0;
    for (int v = 0; v < W; ++v) {
        const long long wv = w[v];
        float mbr[Wd];
        if (Wd == 4) {
            const Vec4f in = *reinterpret_cast<const Vec4f*>(src + (size_t)v * SS);
#pragma unroll
            for (int j = 0; j < Wd; ++j) mbr[j] = in.v[j];
        } else {
            mbr[0] = src[(size_t)v * SS];
        }
#pragma unroll
        for (int j = 0; j < Wd; ++j) N[j] += wv * (long long)clip_rint(mbr[j], lo, hi);
        D += wv;
    }
    if (Wd == 4) {
        Vec4f o;
#pragma unroll
        for (int j = 0; j < Wd; ++j) o.v[j] = fw_mean(N[j], D);
        *reinterpret_cast<Vec4f*>(out + e) = o;
    } else {
        out[e] = fw_mean(N[0], D);
    }
}

}  // namespace

}  // namespace probav

using namespace probav;

extern "C" int probav_frame_windows_gather(const float* patches, const int32_t* counts, int64_t N, int T_pre, int win, int k, int L, int W, int step, int mode,
                                           float* x, int32_t* weight, int32_t* sel, void* stream)
{
    if (!patches || !counts || !x || !weight || !sel || N < 1 || N > 0x7fffffff || T_pre < 1 || T_pre > FW_MAX_T || win < 1 || win > 1024 || k < 1 || k > FW_MAX_T || W < 1 ||
        W > FW_MAX_W || step < 1 || step > 0x10000 || (mode != 0 && mode != 1)) {
        set_error("probav_frame_windows_gather: null/invalid argument (1 <= N < 2^31; 1 <= T_pre <= 64; 1 <= win <= 1024; 1 <= k <= 64; 1 <= W <= 64; "
                  "1 <= step <= 65536; mode 0 = clear, 1 = uniform)", hipSuccess);
        return PROBAV_EINVAL;
    }
    const int64_t px = (int64_t)win * win;
    if ((W > 1 && (int64_t)(W - 1) * step + k > T_pre) || L < 0 || L > px + 1) {
        set_error("probav_frame_windows_gather: W > 1 and (W - 1) step + k > T_pre (a tile whose frames are all eligible would wrap), or L outside 0 .. win^2 + 1",
                  hipSuccess);
        return PROBAV_EINVAL;
    }
    const int64_t PS = fw_plane_stride(px);
    if ((int64_t)T_pre * px > (int64_t)(LDS_LIMIT / 4) || (uint64_t)T_pre * PS * 4 + FW_STATIC_LDS > LDS_LIMIT) {
        char msg[256];
        snprintf(msg, sizeof(msg), "probav_frame_windows_gather: a tile of T_pre = %d frames of %d x %d does not fit the 160 KiB of LDS (at most %d floats "
                 "a tile, each frame padded by up to 3): fewer frames in the pool, or smaller tiles", T_pre, win, win, (int)(LDS_LIMIT / 4));
        set_error(msg, hipSuccess);
        return PROBAV_EINVAL;
    }
    FwGeom g;
    g.T = T_pre; g.win = win; g.px = (int)px; g.PS = (int)PS; g.k = k; g.L = L; g.W = W; g.step = step; g.mode = mode;
    g.vec = reinterpret_cast<uintptr_t>(patches) % 16 == 0 && ((int64_t)T_pre * px) % 4 == 0;
    return launch_lds<frame_windows_gather_kernel>("frame_windows_gather_kernel", dim3((unsigned)N), dim3(FW_THREADS), (size_t)T_pre * PS * 4, (hipStream_t)stream,
                                                   patches, counts, g, x, weight, sel);
}

extern "C" int probav_frame_windows_reduce(const float* sr, const int32_t* weight, int64_t N, int W, int S, float lo, float hi, float* out, void* stream)
{
    if (!sr || !weight || !out || N < 1 || W < 1 || W > FW_MAX_W || S < 1 || S > 0x7fff || !(lo <= hi)) {
        set_error("probav_frame_windows_reduce: null/invalid argument (N >= 1; 1 <= W <= 64; 1 <= S <= 32767; lo <= hi)", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (!(fabsf(lo) <= 16777216.f && fabsf(hi) <= 16777216.f)) {
        set_error("probav_frame_windows_reduce: clip bounds beyond +-2^24 (the result must be an integer that fp32 holds)", hipSuccess);
        return PROBAV_EINVAL;
    }
    const size_t SS = (size_t)S * S;
    if ((uint64_t)N > (uint64_t)0x7fffffffffffull / (SS * (size_t)W)) {
        set_error("probav_frame_windows_reduce: too many predictions for one launch", hipSuccess);
        return PROBAV_EINVAL;
    }
    return launch_pixel_groups<FW_THREADS>(SS % 4 == 0, sr, out, (size_t)N * SS,
                                           "probav_frame_windows_reduce: too many output pixels for one launch: reduce fewer tiles per call",
                                           "frame_windows_reduce_kernel", [&](auto Wd, unsigned blocks, size_t groups) {
        hipLaunchKernelGGL(frame_windows_reduce_kernel<decltype(Wd)::value>, dim3(blocks), dim3(FW_THREADS), 0, (hipStream_t)stream, sr, weight, W, SS, groups, lo,
                           hi, out);
    });
}
