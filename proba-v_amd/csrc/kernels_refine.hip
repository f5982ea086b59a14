// Dataset builder, refined quality masks (gfx950): after registration a set holds T co-registered looks at the same ground; a pixel that the
// quality mask calls clear but that lies far from the per-pixel temporal median of the set's clear looks, in units of their median absolute
// deviation, is taken out of the mask (thin cloud, shadow, saturation, haze, and the strip that the circular registration rolls in).  The
// counterpart of nothing in the reference: its README names the radiometric half of the problem ("I haven't clipped the LR images according
// to its bit depth which is 14-bit") and leaves it there.  The statement the kernels equal bit for bit is probav_amd.prep.refine_masks_numpy.
//
// The statement.  Per set, frames x[t] uint16 and clear flags c[t], t < T <= 64, per pixel p, everything an integer:
//     sat[t] = c[t] and saturation >= 0 and x[t] > saturation          c'[t] = c[t] and not sat[t]          n = #{t : c'[t]}
//     med = element (n - 1) / 2 of {x[t] : c'[t]} in ascending order   (the lower median)
//     d[t] = |x[t] - med|        mad = element (n - 1) / 2 of {d[t] : c'[t]} in ascending order        s = max(mad, floor)
//     o[t] = c'[t] and n >= min_clear and 16 d[t] > k16 s              (strict)
//     g[t][p] = any (sat | o)[t][q] over |q - p|_inf <= dilate, q inside the frame (nothing wraps or reflects)
//     clear_out[t] = c[t] and not g[t]      counts[t] = sum_p clear_out      flagged[t] = {sum_p sat, sum_p o}     (before the dilation)
//
// Exactness.  x, med, d, mad, floor <= 65535 and k16 <= 1024: 16 d < 2^20 and k16 s < 2^26, int32 with room.  Only VALUES are selected, so
// ties need no rule.  The element of rank r = (n - 1) / 2 of n values below 2^16 is the largest v with #{values < v} <= r (#{values < v} is
// non-decreasing in v, it is <= r at v = that element and > r one above it): 16 steps set the bits of v from the top, each one count over
// the values.  A slot holding 0xFFFF is never below any candidate (candidates are <= 0xFFFF), so slots past n are padded with it and the
// count runs over the set's length instead of the pixel's n: the loop is the same for every lane.  The counts per frame are integer
// atomicAdds: exact in any order.  No floating point anywhere in this unit.
//
// Shape, two launches, both one workgroup of 256 threads per (set, tile of RT_H x RT_W = 4 x 64 pixels), ONE THREAD PER PIXEL: a wave is 64
// consecutive pixels of one row (128 B of a frame, 64 B of a mask, 512 B of a plane of pixel_masks).  Between them a pixel's T flags travel
// as ONE 64-bit word per kind, bit t = frame t of the set: pixel_masks [set][3][pixel] = {clear, saturated, outlier}.
//   refine_stats_kernel.  A thread reads its pixel of every frame of the set (RT_SWEEP frames' loads in flight at a time) and keeps the
//   clear, unsaturated values COMPACTED in its own column of LDS, two uint16 to a dword, laid out [j / 2][pixel]: at every step the lanes
//   of a wave read consecutive dwords, one bank each.  Which t each j came from stays in a 64-bit register mask.  LDS is used because a
//   register array cannot be indexed by a run-time j; no thread reads another's column, so the kernel has no barrier.  256 x 4 x
//   ceil(max_set_len / 2) bytes (32 KiB at 64 frames, 5 KiB at 9: several workgroups per CU either way).  Median by bisection, the column
//   rewritten as d, the MAD by bisection, the test; three 8-byte stores per pixel, and the first tile zeroes the set's counters.  Work:
//   2 x 16 x T / 2 LDS reads and 2 x 16 x T compares per pixel against 3 bytes read per pixel and frame: the compares bound it (measured:
//   2 ms of vector work on the 32 447-frame corpus, where a copy of the statement's bytes takes 0.4 ms).
//   refine_dilate_kernel.  The flagged words (saturated | outlier) of the tile and a halo of `dilate` pixels go to LDS (at most 10 x 70 x 8
//   bytes, zeros outside the frame); one OR over the window dilates EVERY frame of the set at once, per pixel and not per pixel and frame.
//   The frame loop is then a bit test, a byte store and three ballots + popcounts whose results are parked in lane t; at the end the four
//   waves' sums meet in LDS and every frame's counters take one atomicAdd per workgroup.
//   (Measured on the way here, same corpus: one workgroup per (FRAME, tile) reading a byte of flags per frame took 7.6 ms, two million
//   workgroups that each walked set_offsets by bisection; per set with a T x halo byte array in LDS and the window read once per frame,
//   3.1 ms whatever was done to its loads and atomics: about 120 vector instructions per frame and wave.)
// A set that breaks the preconditions (include/probav_hip.h) is skipped by both kernels before any of its frames is touched; the second
// marks its frames' counters.
#include "probav_common.h"
#include "../../include/probav_hip.h"

namespace probav {

namespace {

constexpr int RT_H = 4, RT_W = 64, RT_THREADS = RT_H * RT_W, RT_MAX_T = 64, RT_MAX_DILATE = 3;
constexpr int RT_HALO_MAX = (RT_H + 2 * RT_MAX_DILATE) * (RT_W + 2 * RT_MAX_DILATE);      // 700 positions
constexpr int RT_HALO_PER_THREAD = (RT_HALO_MAX + RT_THREADS - 1) / RT_THREADS;            // 3
constexpr int RT_SWEEP = 8;                                                                // frames whose loads are issued together (statistics)

// set s keeps the preconditions: the whole array's ends, and its own bounds inside the frames and within the launch's LDS
__device__ __forceinline__ bool refine_set_ok(const int64_t* off, int n_sets, int64_t n_frames, int s, int max_set_len)
{
    if (off[0] != 0 || off[n_sets] != n_frames) return false;
    const int64_t a = off[s], b = off[s + 1];
    return a >= 0 && b <= n_frames && b > a && b - a <= (int64_t)max_set_len;
}

// element of rank r of the uint16 values packed two to a dword in col[0], col[RT_THREADS], ... (`words` dwords, unused slots 0xFFFF):
// the largest v with #{values < v} <= r
__device__ __forceinline__ int refine_select(const uint32_t* col, int words, int r)
{
    int v = 0;
    for (int bit = 15; bit >= 0; --bit) {
        const unsigned c = (unsigned)v | (1u << bit);
        int below = 0;
#pragma unroll 4
        for (int w = 0; w < words; ++w) {
            const uint32_t two = col[w * RT_THREADS];
            below += (two & 0xFFFFu) < c;
            below += (two >> 16) < c;
        }
        if (below <= r) v = (int)c;
    }
    return v;
}

__global__ __launch_bounds__(RT_THREADS) void refine_stats_kernel(const uint16_t* __restrict__ frames, const uint8_t* __restrict__ masks,
                                                                  const int64_t* __restrict__ set_offsets, int n_sets, int64_t n_frames, int H, int W,
                                                                  int tiles_x, int tiles, int max_set_len, int k16, int floor_dn, int min_clear,
                                                                  int saturation, uint64_t* __restrict__ pixel_masks, int32_t* __restrict__ out_counts,
                                                                  int32_t* __restrict__ flagged)
{
    extern __shared__ __align__(16) unsigned char refine_smem[];
    const int s = blockIdx.x / tiles, tile = blockIdx.x - s * tiles;
    if (!refine_set_ok(set_offsets, n_sets, n_frames, s, max_set_len)) return;       // uniform; nothing of the set is read or written
    const int64_t f0 = set_offsets[s];
    const int T = (int)(set_offsets[s + 1] - f0);
    if (tile == 0 && (int)threadIdx.x < T) {               // T <= 64 < RT_THREADS: the set's counters, before the second launch adds to them
        out_counts[f0 + threadIdx.x] = 0;
        flagged[2 * (f0 + threadIdx.x)] = 0;
        flagged[2 * (f0 + threadIdx.x) + 1] = 0;
    }
    const int y = (tile / tiles_x) * RT_H + (int)(threadIdx.x >> 6), x = (tile % tiles_x) * RT_W + (int)(threadIdx.x & 63);
    if (y >= H || x >= W) return;                          // no barrier below
    const size_t HW = (size_t)H * W, p = (size_t)f0 * HW + (size_t)y * W + x;
    uint32_t* col = reinterpret_cast<uint32_t*>(refine_smem) + threadIdx.x;          // value j: half j & 1 of dword (j >> 1) * RT_THREADS
    uint16_t* col16 = reinterpret_cast<uint16_t*>(col);
    const int words = (T + 1) >> 1;                        // <= (max_set_len + 1) / 2: inside the launch's LDS

    unsigned long long cm = 0, sm = 0, om = 0;             // bit t: clear and unsaturated / saturated / outlier
    int n = 0;
    for (int t0 = 0; t0 < T; t0 += RT_SWEEP) {             // RT_SWEEP frames at a time: 2 RT_SWEEP unconditional loads in flight, one wait
        int vs[RT_SWEEP];
        bool cs[RT_SWEEP];
#pragma unroll
        for (int u = 0; u < RT_SWEEP; ++u) {
            const size_t q = p + (size_t)min(t0 + u, T - 1) * HW;                    // past the set: its last frame again, not used
            vs[u] = frames[q];
            cs[u] = masks[q] != 0 && t0 + u < T;
        }
#pragma unroll
        for (int u = 0; u < RT_SWEEP; ++u) {
            const int t = t0 + u, v = vs[u];
            const bool c = cs[u], sat = c && v > saturation && saturation >= 0;
            if (sat) sm |= 1ull << t;                      // c: t < T <= 64
            if (c && !sat) {
                cm |= 1ull << t;
                col16[(n >> 1) * (2 * RT_THREADS) + (n & 1)] = (uint16_t)v;          // n <= t
                ++n;
            }
        }
    }
    if (n >= min_clear) {
        for (int j = n; j < 2 * words; ++j) col16[(j >> 1) * (2 * RT_THREADS) + (j & 1)] = 0xFFFFu;
        const int r = (n - 1) >> 1;
        const int med = refine_select(col, words, r);
        for (int w = 0; w < words; ++w) {                  // the column as distances; the padding stays
            const uint32_t two = col[w * RT_THREADS];
            const int a = (int)(two & 0xFFFFu) - med, b = (int)(two >> 16) - med;
            const uint32_t da = 2 * w < n ? (uint32_t)(a < 0 ? -a : a) : 0xFFFFu, db = 2 * w + 1 < n ? (uint32_t)(b < 0 ? -b : b) : 0xFFFFu;
            col[w * RT_THREADS] = da | db << 16;
        }
        const int mad = refine_select(col, words, r);
        const int thr = k16 * max(mad, floor_dn);
        int j = 0;
        for (int t = 0; t < T; ++t)
            if ((cm >> t) & 1) {
                if (16 * (int)col16[(j >> 1) * (2 * RT_THREADS) + (j & 1)] > thr) om |= 1ull << t;
                ++j;
            }
    }
    uint64_t* pm = pixel_masks + (size_t)s * 3 * HW + (size_t)y * W + x;             // [set][plane][pixel], bit t = frame t of the set
    pm[0] = cm | sm;                                       // clear, as the quality mask has it
    pm[HW] = sm;
    pm[2 * HW] = om;
}

__global__ __launch_bounds__(RT_THREADS) void refine_dilate_kernel(const uint64_t* __restrict__ pixel_masks,
                                                                   const int64_t* __restrict__ set_offsets, int n_sets, int64_t n_frames, int H, int W,
                                                                   int tiles_x, int tiles, int max_set_len, int dilate, uint8_t* __restrict__ out_masks,
                                                                   int32_t* __restrict__ out_counts, int32_t* __restrict__ flagged)
{
    extern __shared__ __align__(16) unsigned char refine_smem[];
    uint64_t* halo = reinterpret_cast<uint64_t*>(refine_smem);                        // [hs] flagged masks; later the waves' sums
    const int s = blockIdx.x / tiles, tile = blockIdx.x - s * tiles;
    if (!refine_set_ok(set_offsets, n_sets, n_frames, s, max_set_len)) {             // uniform: none of the set's frames is read or written, all are marked
        if (tile == 0) {
            const bool ends = set_offsets[0] != 0 || set_offsets[n_sets] != n_frames;        // then every set is refused: set 0 marks every frame
            int64_t a = ends ? 0 : set_offsets[s], b = ends ? (s == 0 ? n_frames : 0) : set_offsets[s + 1];
            a = a < 0 ? 0 : a;
            b = b > n_frames ? n_frames : b;
            for (int64_t f = a + threadIdx.x; f < b; f += RT_THREADS) out_counts[f] = flagged[2 * f] = flagged[2 * f + 1] = PROBAV_PREP_BAD_COUNT;
        }
        return;
    }
    const int64_t f0 = set_offsets[s];
    const int T = (int)(set_offsets[s + 1] - f0);
    const size_t HW = (size_t)H * W;
    const uint64_t* pm = pixel_masks + (size_t)s * 3 * HW;
    const int y0 = (tile / tiles_x) * RT_H, x0 = (tile % tiles_x) * RT_W;
    const int hw = RT_W + 2 * dilate, hh = RT_H + 2 * dilate, hs = hw * hh;          // hs <= RT_HALO_MAX: inside the launch's LDS

#pragma unroll
    for (int k = 0; k < RT_HALO_PER_THREAD; ++k) {         // flagged = saturated | outlier of the tile and its halo, zeros outside the frame
        const int i = threadIdx.x + k * RT_THREADS;
        if (i < hs) {
            const int yy = y0 - dilate + i / hw, xx = x0 - dilate + i % hw;
            uint64_t f = 0;
            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) f = pm[HW + (size_t)yy * W + xx] | pm[2 * HW + (size_t)yy * W + xx];
            halo[i] = f;
        }
    }
    const int ly = threadIdx.x >> 6, lx = threadIdx.x & 63, y = y0 + ly, x = x0 + lx;
    const bool inside = y < H && x < W;
    const size_t q = inside ? (size_t)y * W + x : 0;
    uint64_t keep = inside ? pm[q] : 0, sat = inside ? pm[HW + q] : 0, outl = inside ? pm[2 * HW + q] : 0;
    __syncthreads();

    uint64_t g = 0;                                        // every frame's dilation at once: one OR over the window per PIXEL, not per pixel and frame
    for (int dy = 0; dy <= 2 * dilate; ++dy)
        for (int dx = 0; dx <= 2 * dilate; ++dx) g |= halo[(ly + dy) * hw + lx + dx];
    keep &= ~g;                                            // bit t: clear_out of frame t
    const bool any_flag = __ballot((sat | outl) != 0) != 0;                           // uniform: most waves have none to count
    uint8_t* om = out_masks + (size_t)f0 * HW + q;
    int cnt = 0, nsat = 0, nout = 0;                       // lane t of a wave: the wave's three sums of frame t (T <= 64 lanes)
    for (int t = 0; t < T; ++t) {                          // uniform: every lane takes part in the ballots
        const bool clear = keep & 1;
        if (inside) om[(size_t)t * HW] = (uint8_t)clear;
        const int c0 = __popcll(__ballot(clear));
        int c1 = 0, c2 = 0;
        if (any_flag) {
            c1 = __popcll(__ballot((sat >> t) & 1));
            c2 = __popcll(__ballot((outl >> t) & 1));
        }
        if (lx == t) { cnt = c0; nsat = c1; nout = c2; }
        keep >>= 1;
    }
    __syncthreads();                                       // the halo has been read: the LDS now takes the waves' sums, [wave][T][3]
    int32_t* sums = reinterpret_cast<int32_t*>(refine_smem);
    if (lx < T) {
        sums[(ly * T + lx) * 3] = cnt;
        sums[(ly * T + lx) * 3 + 1] = nsat;
        sums[(ly * T + lx) * 3 + 2] = nout;
    }
    __syncthreads();
    if ((int)threadIdx.x < 3 * T) {                        // one atomicAdd per frame, counter and workgroup
        int v = 0;
        for (int wv = 0; wv < RT_H; ++wv) v += sums[wv * T * 3 + threadIdx.x];
        const int t = threadIdx.x / 3, k = threadIdx.x - 3 * t;
        if (v) atomicAdd(k == 0 ? out_counts + f0 + t : flagged + 2 * (f0 + t) + (k - 1), v);
    }
}

}  // namespace

}  // namespace probav

using namespace probav;

extern "C" int probav_prep_refine_masks(const uint16_t* frames, const uint8_t* masks, const int64_t* set_offsets, int n_sets, int64_t n_frames, int H, int W,
                                        int max_set_len, int k16, int floor_dn, int min_clear, int dilate, int saturation, uint64_t* pixel_masks,
                                        uint8_t* out_masks, int32_t* out_counts, int32_t* flagged, void* stream)
{
    if (!frames || !masks || !set_offsets || !pixel_masks || !out_masks || !out_counts || !flagged || n_sets < 1 || n_frames < 1 || n_frames > 0x7fffffff ||
        n_sets > n_frames || H < 1 || W < 1) {
        set_error("probav_prep_refine_masks: null/invalid argument", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (k16 < 0 || k16 > 1024 || floor_dn < 0 || floor_dn > 65535 || min_clear < 3 || min_clear > RT_MAX_T || dilate < 0 || dilate > RT_MAX_DILATE ||
        saturation < -1 || saturation > 65535 || max_set_len < 1 || max_set_len > RT_MAX_T) {
        set_error("probav_prep_refine_masks: k16 outside 0..1024, floor outside 0..65535, min_clear outside 3..64, dilate outside 0..3, saturation outside "
                  "-1..65535 or max_set_len outside 1..64", hipSuccess);
        return PROBAV_EINVAL;
    }
    const int64_t tiles_x = ((int64_t)W + RT_W - 1) / RT_W, tiles = tiles_x * (((int64_t)H + RT_H - 1) / RT_H);
    if (tiles > 0x7fffffff || tiles * n_sets > 0x7fffffff) {
        set_error("probav_prep_refine_masks: more than 2^31 - 1 workgroups in one launch", hipSuccess);
        return PROBAV_EINVAL;
    }
    const dim3 grid((unsigned)(tiles * n_sets)), block(RT_THREADS);
    const size_t lds_stats = (size_t)RT_THREADS * sizeof(uint32_t) * ((max_set_len + 1) / 2);
    const size_t lds_halo = std::max((size_t)(RT_H + 2 * dilate) * (RT_W + 2 * dilate) * sizeof(uint64_t),                          // <= 5600 bytes
                                     (size_t)RT_H * max_set_len * 3 * sizeof(int32_t));                                            // the waves' sums
    int rc = launch_lds<refine_stats_kernel>("refine_stats_kernel", grid, block, lds_stats, (hipStream_t)stream, frames, masks, set_offsets, n_sets, n_frames, H, W,
                                             (int)tiles_x, (int)tiles, max_set_len, k16, floor_dn, min_clear, saturation, pixel_masks, out_counts, flagged);
    if (rc) return rc;
    return launch_lds<refine_dilate_kernel>("refine_dilate_kernel", grid, block, lds_halo, (hipStream_t)stream, pixel_masks, set_offsets, n_sets, n_frames, H, W,
                                            (int)tiles_x, (int)tiles, max_set_len, dilate, out_masks, out_counts, flagged);
}
