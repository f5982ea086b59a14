// Random crops (gfx950): training samples cut at arbitrary origins out of registered scenes that stay resident on the device, replacing the
// fixed patch grid that stages 3 to 5 of the dataset builder cut and dumped.  proba-v_amd/crops.py states both kernels in numpy
// (window_counts_numpy, crop_batch_numpy), makes the recipes and drives them; INTEGRATION.md, 'Random crops', has the definition.
//
// 1. probav_window_counts.  masks uint8 [M][H][W] (nonzero = masked) -> counts int32 [M][ny][nx]: the masked pixels of every window of side
//    `win` at stride `stride` of the mask reflect-padded by `pad` (np.pad 'reflect': index -i for i < 0, 2 (n - 1) - i for i >= n).
//    ny = (H + 2 pad - win) / stride + 1, nx likewise.  The product use is the validity table of every crop origin: the HR masks with pad 0,
//    win = scale P, stride = scale.
//    Separable and sliding, never win^2 pixels per position.  A workgroup owns a band of WC_BAND output rows of one mask.  Pass 1, one
//    thread per padded column: the sum of the band's first `win` rows, then for every further output row `stride` rows leave and `stride`
//    rows enter (consecutive lanes read consecutive bytes of a mask row; only the <= pad reflected columns at either end break the order).
//    The WC_BAND x Wp column sums sit in LDS.  Pass 2, one thread per output: the sum of `win` consecutive column sums of its row; lane
//    ox reads dword ox stride + i, so for an odd stride (3, the product's) the 32 lanes of a group sit on 32 banks.  Exact integers (a count
//    is at most win^2 <= 2^20), no atomics, one writer per output.
//
// 2. probav_crop_batch.  One launch per batch.  positions int32 [V][3] = {scene, y, x}, the device-resident list of valid origins; recipe
//    int32 [B][3 + k] = {j, f, q, perm[0..k)}: position j, flip code f and q quarter turns in the convention of kernels_augment.hip, and the
//    frame order.  Scenes: lr fp32 and lr_mask uint8 [S][T_pre][H][H], hr fp32 and hr_clear (1 = clear; bool or uint8) [S][r H][r H].
//    Grid (B, 3), 256 threads: workgroup (b, 0) makes the LR sample, (b, 1) the HR sample, (b, 2) its clear-mask.
//    LR: (a) every wave counts the masked pixels of whole frames of the window (ballot + popcount per 64 pixels: wave-uniform, exact), frame
//    t by wave t mod 4; (b) wave 0 ranks the T_pre <= 64 frames, one lane per frame, by one ballot and T_pre shuffles exactly as
//    frame_windows_gather_kernel does (eligible iff count < L, all when none; order (count, index); tiled m = ceil(k / E) times), and
//    leaves the builder's choice Q[0 .. k) in LDS and in sel[b]; (c) ONLY the k chosen windows are staged, as tile [win][win][k] (17 424 B at
//    win 22, k 9), the reflect pad folded into the load index; (d) augment_emit (augment_part.h) writes out[y][x][i] = frame Q[perm[i]]
//    through the affine source map of the flip and the turns.
//    HR and clear-mask: the window rows r y .. r y + r P - 1 are staged and written the same way.
//
//    Loads.  On the output side every access is unit-stride and full-width (16 B per lane of fp32, 4 B of mask) as in kernels_augment.hip.
//    On the input side a window row is 22 floats (88 B) of an LR frame starting at column x - pad, 48 floats at column 3 x of an HR image:
//    4-byte aligned and no more, for arbitrary x.  They are read with SCALAR loads, one element per lane, consecutive lanes along the row.
//    Wider loads were not chosen: an 8-byte load is aligned only for even x (a second instance of the staging loop plus an odd head and
//    tail element per row), and at the scene's edges the reflect pad reverses up to `pad` elements of a row, which a vector load cannot
//    express.  With scalar loads the reflection is one index computation per element and there is one code path for every origin; a wave
//    still covers whole rows (64 lanes = 2.9 LR rows, 1.3 HR rows), so every fetched 128-byte line is used in full except at the two
//    ends of a row.  The launch moves about 5 MB at B = 128, beside a training step that moves gigabytes.
//    LDS.  Staging writes tile[(wy win + wx) k + i]: consecutive lanes are k dwords apart, conflict-free for odd k (9: the shipped cfg), and
//    2-way or worse for even k, which only costs the staging of a kernel that is not on the step's critical path.  Static LDS: counts
//    [64] and Q [128] ints = 768 B, a multiple of 16, so the dynamic base stays 16-byte aligned.
//
//    Safety.  A recipe row whose j is outside [0, V), whose f or q is outside 0..3 or whose perm holds an entry outside [0, k) is skipped by
//    all three of its workgroups before anything else is read; so is a row whose position {scene, y, x} lies outside the scenes (the list is
//    device data the library did not make).  The decision is uniform across the workgroup.  The host validates recipes before launching
//    (crops.validate_recipe); this is the second line.  No atomics, no hand-off between workgroups: every output byte has one writer,
//    so the result does not depend on the launch.
#include "probav_common.h"
#include "augment_part.h"
#include "../../include/probav_hip.h"

namespace probav {

namespace {

constexpr int WC_THREADS = 256, WC_BAND = 16;
constexpr int CROP_MAX_T = 64;                  // one lane of the ranking wave per frame of the pool
constexpr int CROP_MAX_Q = 2 * CROP_MAX_T;      // E m < k + E, k <= 64, E <= T_pre <= 64
constexpr size_t CROP_STATIC_LDS = (CROP_MAX_T + CROP_MAX_Q) * sizeof(int);

// np.pad(..., 'reflect'): padded index i in [-pad, n + pad), pad <= n - 1
__device__ __forceinline__ int reflect_index(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

struct WcGeom { int H, W, pad, win, stride, ny, nx, Wp, bands; };

__global__ __launch_bounds__(WC_THREADS) void window_counts_kernel(const uint8_t* __restrict__ masks, WcGeom g, int32_t* __restrict__ counts)
{
    extern __shared__ __align__(16) int wc_col[];                    // [WC_BAND][Wp]
    const int m = blockIdx.x / g.bands, band = blockIdx.x - m * g.bands;
    const int oy0 = band * WC_BAND;
    const int rows = min(WC_BAND, g.ny - oy0);
    const uint8_t* src = masks + (size_t)m * g.H * g.W;
    for (int px = threadIdx.x; px < g.Wp; px += WC_THREADS) {
        const uint8_t* col = src + reflect_index(px - g.pad, g.W);
        const int top = oy0 * g.stride - g.pad;                       // unpadded row of the band's first window row (may be negative)
        int s = 0;
        for (int i = 0; i < g.win; ++i) s += col[(size_t)reflect_index(top + i, g.H) * g.W] != 0;
        wc_col[px] = s;
        for (int rb = 1; rb < rows; ++rb) {
            const int out0 = top + (rb - 1) * g.stride;               // rows out0 .. out0 + stride - 1 leave, the same + win enter
            for (int i = 0; i < g.stride; ++i) {
                s -= col[(size_t)reflect_index(out0 + i, g.H) * g.W] != 0;
                s += col[(size_t)reflect_index(out0 + g.win + i, g.H) * g.W] != 0;
            }
            wc_col[rb * g.Wp + px] = s;
        }
    }
    __syncthreads();
    int32_t* dst = counts + ((size_t)m * g.ny + oy0) * g.nx;
    for (int o = threadIdx.x; o < rows * g.nx; o += WC_THREADS) {
        const int rb = o / g.nx, ox = o - rb * g.nx;
        const int* c = wc_col + rb * g.Wp + ox * g.stride;
        int s = 0;
        for (int i = 0; i < g.win; ++i) s += c[i];
        dst[o] = s;
    }
}

struct CropGeom {
    int64_t n_scenes, n_positions;
    int T, H, P, pad, win, r, S, k, L;      // S = r P, the HR window's side
    int lr_vec, hr_vec, mask_vec;           // 1: the output sample's byte size is a multiple of 16 and the output array is 16-byte aligned
};

template <int V>
__device__ __forceinline__ void crop_lr(const float* __restrict__ lr, const uint8_t* __restrict__ lr_mask, const CropGeom& g, int s, int y, int x,
                                        const int32_t* __restrict__ perm, int f, int q, float* __restrict__ dst, int32_t* __restrict__ sel,
                                        unsigned char* smem, int* cnt, int* Qf)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int px = g.win * g.win;
    const size_t frame = (size_t)g.H * g.H, scene = (size_t)s * g.T * frame;
    const int y0 = y - g.pad, x0 = x - g.pad;                        // the window's origin in the unpadded scene

    // (a) masked pixels of every frame of the window: frame t by wave t mod 4
    for (int t = wave; t < g.T; t += AUG_THREADS / 64) {
        const uint8_t* mk = lr_mask + scene + (size_t)t * frame;
        int c = 0;
        for (int p0 = 0; p0 < px; p0 += 64) {
            const int p = p0 + lane;
            bool masked = false;
            if (p < px) {
                const int wy = p / g.win, wx = p - wy * g.win;
                masked = mk[(size_t)reflect_index(y0 + wy, g.H) * g.H + reflect_index(x0 + wx, g.H)] != 0;
            }
            c += __popcll(__ballot(masked));
        }
        if (lane == 0) cnt[t] = c;
    }
    __syncthreads();

    // (b) wave 0 ranks the frames and leaves Q[0 .. E m) (frame_windows_gather_kernel's ranking; window 0, so only Q[0 .. k) is used)
    if (tid < 64) {
        const int t = tid;
        const int c = t < g.T ? cnt[t] : 0;
        unsigned long long elig = __ballot(t < g.T && c < g.L);
        if (elig == 0ull) elig = g.T == 64 ? ~0ull : ((1ull << g.T) - 1ull);
        const int E = __popcll(elig);
        const int m = (g.k + E - 1) / E;
        int rank = 0;
        for (int u = 0; u < g.T; ++u) {
            const int cu = __shfl(c, u, 64);
            if (((elig >> u) & 1ull) && (cu < c || (cu == c && u < t))) ++rank;
        }
        if ((elig >> t) & 1ull) {
            for (int i = 0; i < m; ++i) Qf[rank * m + i] = t;
        }
    }
    __syncthreads();
    if (tid < g.k) sel[tid] = Qf[tid];

    // (c) stage the k chosen windows: tile[(wy win + wx) k + i] = frame Q[i] at the window's pixel (wy, wx)
    float* tile = aug_tile<float>(smem);
    const int total = g.k * px;
    for (int e = tid; e < total; e += AUG_THREADS) {
        const int i = e / px, p = e - i * px;
        const int wy = p / g.win, wx = p - wy * g.win;
        tile[p * g.k + i] = lr[scene + (size_t)Qf[i] * frame + (size_t)reflect_index(y0 + wy, g.H) * g.H + reflect_index(x0 + wx, g.H)];
    }
    // (d) out[y][x][i] = frame Q[perm[i]] through the flip and the turns
    augment_emit<float, V>(dst, g.win, g.k, 1, perm, f, q, smem);
}

// the HR window (or its clear-mask): rows r y .. r y + S - 1, columns r x .. r x + S - 1 of image s [G][G], G = r H
template <typename E, int V>
__device__ __forceinline__ void crop_hr(const E* __restrict__ img, const CropGeom& g, int s, int y, int x, int f, int q, E* __restrict__ dst,
                                        unsigned char* smem)
{
    const size_t G = (size_t)g.r * g.H;
    const E* src = img + (size_t)s * G * G + (size_t)g.r * y * G + (size_t)g.r * x;
    E* tile = aug_tile<E>(smem);
    for (int e = threadIdx.x; e < g.S * g.S; e += AUG_THREADS) {
        const int wy = e / g.S, wx = e - wy * g.S;
        tile[e] = src[(size_t)wy * G + wx];
    }
    augment_emit<E, V>(dst, g.S, 1, 1, nullptr, f, q, smem);
}

__global__ __launch_bounds__(AUG_THREADS) void crop_batch_kernel(const float* __restrict__ lr, const uint8_t* __restrict__ lr_mask,
                                                                  const float* __restrict__ hr, const uint8_t* __restrict__ hr_clear,
                                                                  const int32_t* __restrict__ positions, const int32_t* __restrict__ recipe, CropGeom g,
                                                                  float* __restrict__ lr_b, float* __restrict__ hr_b, uint8_t* __restrict__ mask_b,
                                                                  int32_t* __restrict__ sel)
{
    extern __shared__ __align__(16) unsigned char crop_smem[];
    __shared__ int cnt[CROP_MAX_T], Qf[CROP_MAX_Q];
    const size_t b = blockIdx.x;
    const int32_t* r = recipe + b * (size_t)(3 + g.k);
    const int j = r[0], f = r[1], q = r[2];
    bool bad = j < 0 || (int64_t)j >= g.n_positions || (unsigned)f > 3u || (unsigned)q > 3u;
    for (int i = 0; i < g.k; ++i) bad |= (unsigned)r[3 + i] >= (unsigned)g.k;
    if (bad) return;                                        // the same answer in every thread of the sample's three workgroups
    const int32_t* pos = positions + (size_t)j * 3;
    const int s = pos[0], y = pos[1], x = pos[2];
    if (s < 0 || (int64_t)s >= g.n_scenes || y < 0 || y > g.H - g.P || x < 0 || x > g.H - g.P) return;     // uniform too
    if (blockIdx.y == 0) {
        const size_t n = (size_t)g.win * g.win * g.k;
        if (g.lr_vec) crop_lr<4>(lr, lr_mask, g, s, y, x, r + 3, f, q, lr_b + b * n, sel + b * g.k, crop_smem, cnt, Qf);
        else crop_lr<1>(lr, lr_mask, g, s, y, x, r + 3, f, q, lr_b + b * n, sel + b * g.k, crop_smem, cnt, Qf);
    } else if (blockIdx.y == 1) {
        const size_t n = (size_t)g.S * g.S;
        if (g.hr_vec) crop_hr<float, 4>(hr, g, s, y, x, f, q, hr_b + b * n, crop_smem);
        else crop_hr<float, 1>(hr, g, s, y, x, f, q, hr_b + b * n, crop_smem);
    } else {
        const size_t n = (size_t)g.S * g.S;
        if (g.mask_vec) crop_hr<uint8_t, 4>(hr_clear, g, s, y, x, f, q, mask_b + b * n, crop_smem);
        else crop_hr<uint8_t, 1>(hr_clear, g, s, y, x, f, q, mask_b + b * n, crop_smem);
    }
}

}  // namespace

}  // namespace probav

using namespace probav;

extern "C" int probav_window_counts(const uint8_t* masks, int64_t M, int H, int W, int pad, int win, int stride, int32_t* counts, void* stream)
{
    if (!masks || !counts || M < 1 || H < 1 || W < 1 || H > 0x7fff || W > 0x7fff || pad < 0 || pad >= H || pad >= W || win < 1 || win > 1024 ||
        win > H + 2 * pad || win > W + 2 * pad || stride < 1 || stride > 1024) {
        set_error("probav_window_counts: null/invalid argument (M >= 1; 1 <= H, W <= 32767; 0 <= pad < min(H, W); 1 <= win <= min(1024, H + 2 pad, W + 2 pad); "
                  "1 <= stride <= 1024)", hipSuccess);
        return PROBAV_EINVAL;
    }
    WcGeom g;
    g.H = H; g.W = W; g.pad = pad; g.win = win; g.stride = stride;
    g.ny = (H + 2 * pad - win) / stride + 1; g.nx = (W + 2 * pad - win) / stride + 1;
    g.Wp = W + 2 * pad; g.bands = (g.ny + WC_BAND - 1) / WC_BAND;
    const size_t lds = (size_t)WC_BAND * g.Wp * sizeof(int);
    if (lds > LDS_LIMIT || (uint64_t)M * g.bands > 0x7fffffffull) {
        set_error("probav_window_counts: 16 rows of column sums (64 (W + 2 pad) bytes) must fit the 160 KiB of LDS, and M x ceil(ny / 16) one launch (< 2^31)",
                  hipSuccess);
        return PROBAV_EINVAL;
    }
    return launch_lds<window_counts_kernel>("window_counts_kernel", dim3((unsigned)(M * g.bands)), dim3(WC_THREADS), lds, (hipStream_t)stream, masks, g, counts);
}

extern "C" int probav_crop_batch(const float* lr, const uint8_t* lr_mask, const float* hr, const uint8_t* hr_clear, int64_t n_scenes, int T_pre, int H,
                                 int P, int pad, int win, int scale, int k, int L, const int32_t* positions, int64_t n_positions, const int32_t* recipe,
                                 int64_t batch, float* lr_b, float* hr_b, uint8_t* mask_b, int32_t* sel, void* stream)
{
    if (!lr || !lr_mask || !hr || !hr_clear || !positions || !recipe || !lr_b || !hr_b || !mask_b || !sel || n_scenes < 1 || n_scenes > 0x7fffffff ||
        n_positions < 1 || n_positions > 0x7fffffff || batch < 1 || batch > 0x7fffffff || T_pre < 1 || T_pre > CROP_MAX_T || k < 1 || k > CROP_MAX_T ||
        H < 1 || H > 0x7fff || P < 1 || P > H || pad < 0 || pad >= H || win < P || win > P + 2 * pad || win > AUG_MAX_SIDE || scale < 1 || scale > 64 ||
        (int64_t)scale * P > AUG_MAX_SIDE || L < 0 || (int64_t)L > (int64_t)win * win + 1) {
        set_error("probav_crop_batch: null/invalid argument (1 <= n_scenes, n_positions, batch < 2^31; 1 <= T_pre, k <= 64; 1 <= P <= H <= 32767; "
                  "0 <= pad < H; P <= win <= min(P + 2 pad, 1024); 1 <= scale <= 64, scale P <= 1024; 0 <= L <= win^2 + 1)", hipSuccess);
        return PROBAV_EINVAL;
    }
    const int S = scale * P;
    const size_t lds_lr = aug_part_lds(win, k, sizeof(float)), lds_hr = aug_part_lds(S, 1, sizeof(float));       // (the mask's tile is the smaller HR one)
    const size_t lds = lds_lr > lds_hr ? lds_lr : lds_hr;
    if (lds + CROP_STATIC_LDS > LDS_LIMIT) {
        char msg[256];
        snprintf(msg, sizeof(msg), "probav_crop_batch: one sample (k = %d LR windows of %d x %d, or an HR window of %d x %d floats, plus a row table) does not fit "
                 "the 160 KiB of LDS", k, win, win, S, S);
        set_error(msg, hipSuccess);
        return PROBAV_EINVAL;
    }
    CropGeom g;
    g.n_scenes = n_scenes; g.n_positions = n_positions;
    g.T = T_pre; g.H = H; g.P = P; g.pad = pad; g.win = win; g.r = scale; g.S = S; g.k = k; g.L = L;
    g.lr_vec = ((size_t)win * win * k) % 4 == 0 && reinterpret_cast<uintptr_t>(lr_b) % 16 == 0;
    g.hr_vec = ((size_t)S * S) % 4 == 0 && reinterpret_cast<uintptr_t>(hr_b) % 16 == 0;
    g.mask_vec = ((size_t)S * S) % 16 == 0 && reinterpret_cast<uintptr_t>(mask_b) % 16 == 0;
    return launch_lds<crop_batch_kernel>("crop_batch_kernel", dim3((unsigned)batch, 3), dim3(AUG_THREADS), lds, (hipStream_t)stream, lr, lr_mask, hr,
                                         hr_clear, positions, recipe, g, lr_b, hr_b, mask_b, sel);
}
