// The general matrix route: a stride-1 convolution over (H, W, T) and its backward-filter as implicit GEMMs on the fp32-input MFMA of gfx950
// (v_mfma_f32_32x32x2_f32: fp32 operands, fp32 accumulation, an exact fma chain -- the arithmetic of the VALU kernels, on the matrix cores).
// For ANY Cin and Cout: this is what the engine launches, when probav_engine_set_gemm_route is on, wherever it would otherwise fall to the
// generic direct kernels (kernels_direct.hip).  Same ConvGeom, same operand layouts ([N][H][W][T][C], w [kh][kw][kt][Cin][Cout]), so the
// weight cache and the packing jobs know nothing of it.  DESIGN.md section 4, 'The general matrix route'.
//
// gemm_conv_fwd_kernel   M = output voxels, N = Cout, K = taps x Cin.  A workgroup of four waves owns 128 consecutive voxels x BN = 32 NT output
//   channels; wave w owns rows [32 w, 32 w + 32) and keeps NT accumulator tiles of 32 x 32.  K runs taps outer, 16-channel chunks inner: a chunk's
//   A tile [128][16] (x at the tap's offset, gated, zero on the pads) and B tile [16][BN] (the filter rows) are fetched into registers while the
//   MFMAs of the previous chunk run, then stored to LDS.  Every element outside the problem -- a channel past Cin, an output channel past Cout, a
//   voxel past the end, a tap on the zero padding -- is a ZERO IN BOTH tiles' terms it belongs to (never LDS garbage: 0 x garbage may be NaN).  A tap
//   on the padding is multiplied by its zero, not skipped, as in the direct kernel (0 x w is NaN for a non-finite w).
//   The order of additions of an output element is (tap, chunk, channel pair): it does not depend on the element's row in the tile, on the tile, or
//   on N, and row m of the product reads row m of A alone -- a sample's bits do not depend on its batch mates.
//
// gemm_conv_wgrad_kernel   per tap, M = Cin, N = Cout, K = voxels.  The voxels are cut into `slabs` contiguous ranges (a function of the voxel
//   count alone); workgroup (slab, tap, 64 x 64 tile of Cin x Cout) walks its range 32 voxels at a time: A [32][64] = x at the tap's offset,
//   B [32][64] = dY, gated by the layer's output.  A voxel whose tap falls on the zero padding is a zero row in BOTH tiles (the direct kernel skips
//   it), so a non-finite dY reaches exactly the filter taps whose windows read a real input.  The bias gradient is summed from the fetched dY rows
//   before that zeroing, by the workgroups of tap 0 / input tile 0, in a fixed order.  Each workgroup writes its tile of its slab; the slabs are
//   summed in a fixed order by slab_sum_later.  No atomics: bitwise reproducible on any device.
//
// The wide geometries (gemm_conv_supported_wide / gemm_wgrad_supported_wide: 5x5x5, pads up to k - 1, mirrored H/W pads of 2, a mirrored depth pad -- the 19-frame reducer's,
//   probav_engine_set_gemm_exotic) run on the same two kernels: nothing above is tied to three taps per axis, gemm_reflect folds any pad below the extent, and the mirrored depth
//   index is a branch on the uniform g.reflect_t.  A launch of the old predicates takes the arm it always took: the same bits.
#include "probav_common.h"
#include "kernels_gemm.h"
#include "x6_device.h"

namespace probav {

#define GEMM_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
typedef float gemm_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int gemm_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * n - 2 - i : i;
}

// ---------------------------------------------------------------------------------------------------
// forward / backward-data
// ---------------------------------------------------------------------------------------------------
constexpr int GF_BM = 128;                  // voxels per workgroup
constexpr int GF_KC = 16;                   // input channels per K chunk
constexpr int GF_AS = GF_KC + 1;            // A row stride in LDS (odd: the 32 rows a half-wave reads fall in 32 banks)

// TWO: the sum in two levels -- a tap's chunks into `acc`, the taps' sums into `tot` -- for the launches of more than 27 taps (5x5x5: K = 125 Cin, where one fp32 chain of
// 9 000 terms at 72 channels came to 3.6e-6 of max |ref|).  The order is still a function of (tap, chunk, channel pair) alone.  A template parameter: the instances the route
// launched before it (TWO = false) are the code they were
template <int NT, bool GATE, bool TWO>
__global__ __launch_bounds__(256) void gemm_conv_fwd_kernel(ConvGeom g, const float* __restrict__ x, const float* __restrict__ gate, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ skip, float* __restrict__ y)
{
    constexpr int BN = 32 * NT;
    constexpr int BS = BN + ((BN & 63) ? 0 : 32);      // B row stride: rows k and k + 1 (the two half-waves of an MFMA operand read) 32 banks apart
    constexpr int RB = GF_KC * BN / 256;               // B elements a thread fetches per chunk
    __shared__ float As[GF_BM * GF_AS];
    __shared__ float Bs[GF_KC * BS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long nvox = (long)g.N * g.Ho * g.Wo * g.To;
    const long m0 = (long)blockIdx.x * GF_BM;
    const int co0 = blockIdx.y * BN;
    const int taps = g.kh * g.kw * g.kt;
    const int nchunk = (g.Cin + GF_KC - 1) / GF_KC;
    const int niter = taps * nchunk;

    // the eight rows of the A tile this thread fetches (row i * 16 + tid / 16, channel tid % 16 of the chunk): their output coordinates, vn < 0 past the end
    int vn[8], vh[8], vw[8], vt[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        long r = m0 + i * 16 + (tid >> 4);
        if (r < nvox) {
            vt[i] = (int)(r % g.To); r /= g.To;
            vw[i] = (int)(r % g.Wo); r /= g.Wo;
            vh[i] = (int)(r % g.Ho);
            vn[i] = (int)(r / g.Ho);
        } else { vn[i] = -1; vh[i] = vw[i] = vt[i] = 0; }
    }

    float ra[8], rb[RB];
    auto fetch = [&](int it) {
        const int tap = it / nchunk, c0 = (it - tap * nchunk) * GF_KC;
        const int a = tap / (g.kw * g.kt), b = (tap / g.kt) % g.kw, c = tap % g.kt;
        const int ch = c0 + (tid & 15);
        const bool ch_ok = ch < g.Cin;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float v = 0.f;
            if (vn[i] >= 0 && ch_ok) {
                int ih = vh[i] + a - g.ph, iw = vw[i] + b - g.pw;
                int id = vt[i] + c - g.pt;
                bool pad = false;
                if (g.reflect_t) id = gemm_reflect(id, g.Ti);          // (uniform) the mirrored depth pad of the wide geometries: no tap of it is padding
                else pad = id < 0 || id >= g.Ti;
                if (g.reflect_hw) { ih = gemm_reflect(ih, g.Hi); iw = gemm_reflect(iw, g.Wi); }
                else pad = pad || ih < 0 || ih >= g.Hi || iw < 0 || iw >= g.Wi;
                if (!pad) {
                    const long off = ((((long)vn[i] * g.Hi + ih) * g.Wi + iw) * g.Ti + id) * g.Cin + ch;
                    v = x[off];
                    if (GATE) v = gate[off] > 0.f ? v : 0.f;
                }
            }
            ra[i] = v;
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            const int idx = j * 256 + tid;
            const int k = idx / BN, n = idx % BN;
            const int ci = c0 + k, co = co0 + n;
            rb[j] = (ci < g.Cin && co < g.Cout) ? w[((long)tap * g.Cin + ci) * g.Cout + co] : 0.f;
        }
    };

    gemm_f32x16 acc[NT], tot[TWO ? NT : 1];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
    if constexpr (TWO) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[nt][r] = 0.f;
    }
    [[maybe_unused]] int left = nchunk;             // (TWO) chunks left of the current tap

    fetch(0);
    for (int it = 0; it < niter; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) As[(i * 16 + (tid >> 4)) * GF_AS + (tid & 15)] = ra[i];
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            const int idx = j * 256 + tid;
            Bs[(idx / BN) * BS + idx % BN] = rb[j];
        }
        __syncthreads();
        if (it + 1 < niter) fetch(it + 1);              // the next chunk's loads fly under this chunk's MFMAs
#pragma unroll
        for (int s2 = 0; s2 < GF_KC / 2; ++s2) {
            const int k = 2 * s2 + (lane >> 5);
            const float av = As[(wave * 32 + (lane & 31)) * GF_AS + k];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = GEMM_MFMA(av, Bs[k * BS + nt * 32 + (lane & 31)], acc[nt]);
        }
        if constexpr (TWO) if (--left == 0) {       // (uniform) the tap is complete: its sum joins the total
            left = nchunk;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) { tot[TWO ? nt : 0][r] += acc[nt][r]; acc[nt][r] = 0.f; }
        }
        __syncthreads();
    }

    // C/D map of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = co0 + nt * 32 + (lane & 31);
        if (co >= g.Cout) continue;
        const float bv = bias ? bias[co] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long v = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (v >= nvox) continue;
            float o = (TWO ? tot[TWO ? nt : 0][r] : acc[nt][r]) + bv;
            if (g.relu) o = relu_keep_nan(o);
            if (skip) o += skip[v * g.Cout + co];
            y[v * g.Cout + co] = o;
        }
    }
}

static bool gemm_common_supported(const ConvGeom& g, int maxpad)
{
    if (g.N < 1 || g.Cin < 1 || g.Cout < 1 || g.Hi < 1 || g.Wi < 1 || g.Ti < 1 || g.Ho < 1 || g.Wo < 1 || g.To < 1) return false;
    if (g.reflect_t) return false;
    const bool pw = g.kh == 1 && g.kw == 1 && g.kt == 1;
    const bool k3 = g.kh == 3 && g.kw == 3 && (g.kt == 3 || g.kt == 1);
    if (!pw && !k3) return false;
    if (g.ph < 0 || g.pw < 0 || g.pt < 0 || g.ph > maxpad || g.pw > maxpad || g.pt > maxpad) return false;
    if (g.reflect_hw && (g.ph > 1 || g.pw > 1 || g.Hi < 2 || g.Wi < 2)) return false;
    // the output extents are the input's (a voxel's window then lies inside the padded input: the kernels' address arithmetic relies on it)
    if (g.Ho != g.Hi + 2 * g.ph - g.kh + 1 || g.Wo != g.Wi + 2 * g.pw - g.kw + 1 || g.To != g.Ti + 2 * g.pt - g.kt + 1) return false;
    // voxel indices and grid extents are ints
    const long lim = (long)1 << 30;
    if ((long)g.N * g.Hi * g.Wi * g.Ti >= lim || (long)g.N * g.Ho * g.Wo * g.To >= lim) return false;
    if ((long)g.kh * g.kw * g.kt * g.Cin * (long)g.Cout >= lim) return false;
    return true;
}

bool gemm_conv_supported(const ConvGeom& g) { return gemm_common_supported(g, 2); }

// The wide geometries (the 19-frame reducer's, which the engine calls exotic): k x k x k and k x k x 1 for k in {1, 3, 5}, zero pads up to `maxzero` and never above
// k - 1, mirrored H/W and depth pads up to 2 on an extent above the pad (gemm_reflect folds once).  The kernels are the ones above: they run taps = kh kw kt outer
// from the geometry, and the mirrored depth index is a branch on the uniform g.reflect_t
static bool gemm_wide_supported(const ConvGeom& g, int maxzero)
{
    if (g.N < 1 || g.Cin < 1 || g.Cout < 1 || g.Hi < 1 || g.Wi < 1 || g.Ti < 1 || g.Ho < 1 || g.Wo < 1 || g.To < 1) return false;
    if (g.kh != g.kw || (g.kh != 1 && g.kh != 3 && g.kh != 5) || (g.kt != g.kh && g.kt != 1)) return false;
    if (g.ph < 0 || g.pw < 0 || g.pt < 0 || g.ph > g.kh - 1 || g.pw > g.kw - 1 || g.pt > g.kt - 1) return false;
    const int mh = g.reflect_hw ? 2 : maxzero, mt = g.reflect_t ? 2 : maxzero;
    if (g.ph > mh || g.pw > mh || g.pt > mt) return false;
    if (g.reflect_hw && (g.Hi <= g.ph || g.Wi <= g.pw)) return false;
    if (g.reflect_t && g.Ti <= g.pt) return false;
    if (g.Ho != g.Hi + 2 * g.ph - g.kh + 1 || g.Wo != g.Wi + 2 * g.pw - g.kw + 1 || g.To != g.Ti + 2 * g.pt - g.kt + 1) return false;
    const long lim = (long)1 << 30;
    if ((long)g.N * g.Hi * g.Wi * g.Ti >= lim || (long)g.N * g.Ho * g.Wo * g.To >= lim) return false;
    if ((long)g.kh * g.kw * g.kt * g.Cin * (long)g.Cout >= lim) return false;
    return true;
}

bool gemm_conv_supported_wide(const ConvGeom& g) { return gemm_wide_supported(g, 4); }

int gemm_fwd_nt(const ConvGeom& g) { return g.Cout <= 32 ? 1 : (g.Cout <= 64 ? 2 : 4); }

static void gemm_conv_plan_fill(const ConvGeom& g, int v[6])
{
    const int bn = 32 * gemm_fwd_nt(g);
    const long nvox = (long)g.N * g.Ho * g.Wo * g.To;
    v[0] = GF_BM; v[1] = bn; v[2] = (int)((nvox + GF_BM - 1) / GF_BM); v[3] = (g.Cout + bn - 1) / bn; v[4] = GF_KC; v[5] = (g.Cin + GF_KC - 1) / GF_KC;
}

bool gemm_conv_plan_ints_wide(const ConvGeom& g, int v[6])
{
    if (!gemm_conv_supported_wide(g)) return false;
    gemm_conv_plan_fill(g, v);
    return true;
}

bool gemm_conv_plan_ints(const ConvGeom& g, int v[6])
{
    if (!gemm_conv_supported(g)) return false;
    gemm_conv_plan_fill(g, v);
    return true;
}

static int gemm_conv_launch(const ConvGeom& g, const int v[6], const float* x, const float* gate, const float* w, const float* bias, const float* skip, float* y, hipStream_t s, bool two = false);

int gemm_conv_forward(const ConvGeom& g, const float* x, const float* gate, const float* w, const float* bias, const float* skip, float* y, hipStream_t s)
{
    int v[6];
    if (!gemm_conv_plan_ints(g, v)) { set_error("gemm_conv_forward: geometry not supported", hipSuccess); return PROBAV_EINVAL; }
    return gemm_conv_launch(g, v, x, gate, w, bias, skip, y, s);
}

int gemm_conv_forward_wide(const ConvGeom& g, const float* x, const float* gate, const float* w, const float* bias, const float* skip, float* y, hipStream_t s)
{
    int v[6];
    if (!gemm_conv_plan_ints_wide(g, v)) { set_error("gemm_conv_forward_wide: geometry not supported", hipSuccess); return PROBAV_EINVAL; }
    return gemm_conv_launch(g, v, x, gate, w, bias, skip, y, s, g.kh * g.kw * g.kt > 27);     // more taps than any launch of the old predicate: the two-level sum
}

static int gemm_conv_launch(const ConvGeom& g, const int v[6], const float* x, const float* gate, const float* w, const float* bias, const float* skip, float* y, hipStream_t s, bool two)
{
    if (v[3] > 65535) { set_error("gemm_conv_forward: Cout too large", hipSuccess); return PROBAV_EINVAL; }
    const dim3 grid((unsigned)v[2], (unsigned)v[3]), block(256);
#define PROBAV_GF(NT) do { \
        if (two && gate) hipLaunchKernelGGL((gemm_conv_fwd_kernel<NT, true, true>), grid, block, 0, s, g, x, gate, w, bias, skip, y); \
        else if (two) hipLaunchKernelGGL((gemm_conv_fwd_kernel<NT, false, true>), grid, block, 0, s, g, x, gate, w, bias, skip, y); \
        else if (gate) hipLaunchKernelGGL((gemm_conv_fwd_kernel<NT, true, false>), grid, block, 0, s, g, x, gate, w, bias, skip, y); \
        else hipLaunchKernelGGL((gemm_conv_fwd_kernel<NT, false, false>), grid, block, 0, s, g, x, gate, w, bias, skip, y); } while (0)
    switch (gemm_fwd_nt(g)) {
    case 1: PROBAV_GF(1); break;
    case 2: PROBAV_GF(2); break;
    default: PROBAV_GF(4); break;
    }
#undef PROBAV_GF
    return check_launch("gemm_conv_fwd");
}

// ---------------------------------------------------------------------------------------------------
// backward-filter
// ---------------------------------------------------------------------------------------------------
constexpr int GW_T = 64;                    // tile: input channels x output channels per workgroup (2 x 2 waves of 32 x 32)
constexpr int GW_KV = 32;                   // voxels per K chunk
constexpr int GW_S = GW_T + 32;             // row stride of both tiles: rows k and k + 1 of an MFMA operand read 32 banks apart
constexpr int GW_MAX_SLABS = 32;            // bounds the scratch: slabs x (taps Cin Cout + Cout) floats per launch
constexpr long GW_MIN_VOX = 1024;           // a slab is worth a workgroup from here on

// slabs, voxels per slab (a multiple of the chunk): from the voxel count alone -- never from the device
static void gemm_wgrad_slabs(const ConvGeom& g, int& slabs, long& vps)
{
    const long nvox = (long)g.N * g.Ho * g.Wo * g.To;
    long want = (nvox + GW_MIN_VOX - 1) / GW_MIN_VOX;
    want = want < 1 ? 1 : (want > GW_MAX_SLABS ? GW_MAX_SLABS : want);
    vps = ((nvox + want - 1) / want + GW_KV - 1) / GW_KV * GW_KV;
    slabs = (int)((nvox + vps - 1) / vps);
}

template <bool GATE>
__global__ __launch_bounds__(256) void gemm_conv_wgrad_kernel(ConvGeom g, const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ gate,
                                                              float* __restrict__ partial, float* __restrict__ partial_b, long vps, int ncot)
{
    __shared__ float As[GW_KV * GW_S];
    __shared__ float Bs[GW_KV * GW_S];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tap = blockIdx.y;
    const int cit = blockIdx.z / ncot, cot = blockIdx.z - cit * ncot;
    const int ci0 = cit * GW_T, co0 = cot * GW_T;
    const int a = tap / (g.kw * g.kt), b = (tap / g.kt) % g.kw, c = tap % g.kt;
    const long nvox = (long)g.N * g.Ho * g.Wo * g.To;
    const long v0 = (long)blockIdx.x * vps;
    const long v1 = v0 + vps < nvox ? v0 + vps : nvox;
    const int niter = (int)((v1 - v0 + GW_KV - 1) / GW_KV);
    const bool want_db = tap == 0 && cit == 0;

    // this thread fetches rows kr and kr + 16 of a chunk (voxels), columns tid % 16 + 16 j of both tiles; their coordinates advance by a chunk at a time
    const int kr = tid >> 4, cl = tid & 15;
    int vn[2], vh[2], vw[2], vt[2];
    long pv[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        long r = v0 + kr + 16 * p;
        pv[p] = r;
        vt[p] = (int)(r % g.To); r /= g.To;
        vw[p] = (int)(r % g.Wo); r /= g.Wo;
        vh[p] = (int)(r % g.Ho);
        vn[p] = (int)(r / g.Ho);
    }
    // a chunk's step in the mixed radix (To, Wo, Ho)
    int sT, sW, sH, sN;
    { int r = GW_KV; sT = r % g.To; r /= g.To; sW = r % g.Wo; r /= g.Wo; sH = r % g.Ho; sN = r / g.Ho; }

    float ra[2][4], rb[2][4], accb[4] = {0.f, 0.f, 0.f, 0.f};
    auto fetch = [&]() {                        // the chunk at the current coordinates; then step them
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const bool live = pv[p] < v1;
            int ih = vh[p] + a - g.ph, iw = vw[p] + b - g.pw;
            int id = vt[p] + c - g.pt;
            bool pad = false;
            if (g.reflect_t) id = gemm_reflect(id, g.Ti);              // (uniform) the mirrored depth pad of the wide geometries
            else pad = id < 0 || id >= g.Ti;
            if (g.reflect_hw) { ih = gemm_reflect(ih, g.Hi); iw = gemm_reflect(iw, g.Wi); }
            else pad = pad || ih < 0 || ih >= g.Hi || iw < 0 || iw >= g.Wi;
            const long xoff = ((((long)vn[p] * g.Hi + ih) * g.Wi + iw) * g.Ti + id) * g.Cin;
            const long yoff = pv[p] * g.Cout;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ci = ci0 + cl + 16 * j, co = co0 + cl + 16 * j;
                float d = 0.f;
                if (live && co < g.Cout) {
                    d = dy[yoff + co];
                    if (GATE) d = gate[yoff + co] > 0.f ? d : 0.f;
                }
                accb[j] += d;                   // the bias gradient sums every voxel, padded taps or not (used by tap 0 / input tile 0 only)
                rb[p][j] = (live && !pad) ? d : 0.f;
                ra[p][j] = (live && !pad && ci < g.Cin) ? x[xoff + ci] : 0.f;
            }
            // step: each digit is below its radix, so is each step digit: one carry per digit
            pv[p] += GW_KV;
            int t2 = vt[p] + sT; int cy = t2 >= g.To; vt[p] = t2 - (cy ? g.To : 0);
            int w2 = vw[p] + sW + cy; cy = w2 >= g.Wo; vw[p] = w2 - (cy ? g.Wo : 0);
            int h2 = vh[p] + sH + cy; cy = h2 >= g.Ho; vh[p] = h2 - (cy ? g.Ho : 0);
            vn[p] += sN + cy;
        }
    };

    gemm_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int wm = wave >> 1, wn = wave & 1;                                   // the wave's 32 x 32 part of the 64 x 64 tile
    const bool wave_live = ci0 + wm * 32 < g.Cin && co0 + wn * 32 < g.Cout;      // (wave-uniform) nothing of its part is inside the problem: no MFMAs

    fetch();
    for (int it = 0; it < niter; ++it) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                As[(kr + 16 * p) * GW_S + cl + 16 * j] = ra[p][j];
                Bs[(kr + 16 * p) * GW_S + cl + 16 * j] = rb[p][j];
            }
        __syncthreads();
        if (it + 1 < niter) fetch();
        if (wave_live) {
#pragma unroll
            for (int s2 = 0; s2 < GW_KV / 2; ++s2) {
                const int k = 2 * s2 + (lane >> 5);
                acc = GEMM_MFMA(As[k * GW_S + wm * 32 + (lane & 31)], Bs[k * GW_S + wn * 32 + (lane & 31)], acc);
            }
        }
        __syncthreads();
    }

    if (wave_live) {
        float* pp = partial + (long)blockIdx.x * ((long)gridDim.y * g.Cin * g.Cout) + (long)tap * g.Cin * g.Cout;
        const int co = co0 + wn * 32 + (lane & 31);
        if (co < g.Cout) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = ci0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (ci < g.Cin) pp[(long)ci * g.Cout + co] = acc[r];
            }
        }
    }
    if (want_db) {                              // (workgroup-uniform) the 16 row groups' sums of each column, added in a fixed order
#pragma unroll
        for (int j = 0; j < 4; ++j) As[kr * GW_S + cl + 16 * j] = accb[j];
        __syncthreads();
        if (tid < GW_T && co0 + tid < g.Cout) {
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) sum += As[k * GW_S + tid];
            partial_b[(long)blockIdx.x * g.Cout + co0 + tid] = sum;
        }
    }
}

bool gemm_wgrad_supported(const ConvGeom& g)
{
    if (!gemm_common_supported(g, 1)) return false;
    const long ncit = (g.Cin + GW_T - 1) / GW_T, ncot = (g.Cout + GW_T - 1) / GW_T;
    return ncit * ncot <= 65535;
}

bool gemm_wgrad_supported_wide(const ConvGeom& g)
{
    if (!gemm_wide_supported(g, 2)) return false;
    const long ncit = (g.Cin + GW_T - 1) / GW_T, ncot = (g.Cout + GW_T - 1) / GW_T;
    return ncit * ncot <= 65535;
}

static void gemm_wgrad_plan_fill(const ConvGeom& g, int v[5]);
bool gemm_wgrad_plan_ints_wide(const ConvGeom& g, int v[5])
{
    if (!gemm_wgrad_supported_wide(g)) return false;
    gemm_wgrad_plan_fill(g, v);
    return true;
}

bool gemm_wgrad_plan_ints(const ConvGeom& g, int v[5])
{
    if (!gemm_wgrad_supported(g)) return false;
    gemm_wgrad_plan_fill(g, v);
    return true;
}

static void gemm_wgrad_plan_fill(const ConvGeom& g, int v[5])
{
    int slabs; long vps;
    gemm_wgrad_slabs(g, slabs, vps);
    const int ncit = (g.Cin + GW_T - 1) / GW_T, ncot = (g.Cout + GW_T - 1) / GW_T;
    v[0] = slabs; v[1] = (int)vps; v[2] = GW_T; v[3] = GW_T; v[4] = slabs * g.kh * g.kw * g.kt * ncit * ncot;
}

size_t gemm_wgrad_partial_floats(const ConvGeom& g)
{
    int slabs; long vps;
    gemm_wgrad_slabs(g, slabs, vps);
    return (size_t)slabs * ((size_t)g.kh * g.kw * g.kt * g.Cin * g.Cout + g.Cout);
}

static int gemm_wgrad_launch(const ConvGeom& g, const float* x, const float* dy, const float* gate, float* dw, float* db, float* partial, hipStream_t s);

int gemm_conv_wgrad(const ConvGeom& g, const float* x, const float* dy, const float* gate, float* dw, float* db, float* partial, hipStream_t s)
{
    if (!gemm_wgrad_supported(g)) { set_error("gemm_conv_wgrad: geometry not supported", hipSuccess); return PROBAV_EINVAL; }
    return gemm_wgrad_launch(g, x, dy, gate, dw, db, partial, s);
}

int gemm_conv_wgrad_wide(const ConvGeom& g, const float* x, const float* dy, const float* gate, float* dw, float* db, float* partial, hipStream_t s)
{
    if (!gemm_wgrad_supported_wide(g)) { set_error("gemm_conv_wgrad_wide: geometry not supported", hipSuccess); return PROBAV_EINVAL; }
    return gemm_wgrad_launch(g, x, dy, gate, dw, db, partial, s);
}

static int gemm_wgrad_launch(const ConvGeom& g, const float* x, const float* dy, const float* gate, float* dw, float* db, float* partial, hipStream_t s)
{
    int slabs; long vps;
    gemm_wgrad_slabs(g, slabs, vps);
    const int taps = g.kh * g.kw * g.kt;
    const int ncit = (g.Cin + GW_T - 1) / GW_T, ncot = (g.Cout + GW_T - 1) / GW_T;
    const long nw = (long)taps * g.Cin * g.Cout;
    float* partial_b = partial + (size_t)slabs * nw;
    const dim3 grid((unsigned)slabs, (unsigned)taps, (unsigned)(ncit * ncot)), block(256);
    if (gate) hipLaunchKernelGGL(gemm_conv_wgrad_kernel<true>, grid, block, 0, s, g, x, dy, gate, partial, partial_b, vps, ncot);
    else hipLaunchKernelGGL(gemm_conv_wgrad_kernel<false>, grid, block, 0, s, g, x, dy, gate, partial, partial_b, vps, ncot);
    const int rc = check_launch("gemm_conv_wgrad");
    if (rc) return rc;
    // a filter gradient and its bias gradient are two jobs of one slab sum: fp64 across the slabs in a fixed order (kernels_small.hip)
    SlabSumJob jobs[2] = {{partial, dw, nw, (int)nw, slabs}, {partial_b, db, (long)g.Cout, g.Cout, slabs}};
    return slab_sum_later(s, jobs, db ? 2 : 1);
}

}  // namespace probav
