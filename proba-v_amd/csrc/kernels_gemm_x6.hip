// The general matrix route on the 16-bit matrix pipe: the convolution kernel of kernels_gemm.hip (forward and backward-data) in x6 arithmetic.  An fp32 operand is cut into three bf16
// truncation pieces (pieces / cut8<X6> of x6_device.h) ONCE, as it is stored to LDS; a 16-deep K step of a 32 x 32 accumulator tile is then the six
// largest piece products on v_mfma_f32_32x32x16_bf16, smallest terms first (mac<X6>'s order, on two accumulators: gx_mac below), against eight v_mfma_f32_32x32x2_f32 of the fp32 route: 6 x 32
// matrix cycles instead of 8 x 64, and 3 + 3 NT sixteen-byte LDS reads instead of 8 + 8 NT four-byte ones.  No operand scaling, so no amax slots.
// Geometries, operand layouts, tiles, grids, tails, pad handling and epilogue are those of
// kernels_gemm.hip (its header comment states them); what differs is the staging.  DESIGN.md section 4.2.
//
// The operand lane map of the 32x32x16 bf16 MFMA: A[row l & 31][k = 8 (l >> 5) + j], B[k = 8 (l >> 5) + j][col l & 31], j = 0 .. 7 -- a lane's eight
// consecutive k of its row / column.  Both operands therefore lie in LDS as piece planes of [row or column][k] bf16, so that a lane's fragment is 16
// contiguous, 16-byte-aligned bytes: one ds_read_b128 per piece.
//
// gemm_conv_fwd_x6_kernel   A [128 voxels][16 channels]: memory has the channels innermost, a thread fetches the eight consecutive channels of half a
//   row (two 16-byte loads where Cin % 4 == 0) and stores its three fragments whole.  B [BN output channels][16 input channels]: memory has Cout
//   innermost, so B is TRANSPOSED on its way into LDS -- a thread fetches 2 NT consecutive input channels of one output channel (the loads of a wave
//   coalesce along Cout) and stores them as 4 NT contiguous bytes per plane.
//   Banks.  A plane row is 32 bytes = two 16-byte slots; ds_read_b128 is served in four groups of 16 lanes ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and
//   the same + 32: one half-wave h = l >> 5 each, rows that are all different modulo 16), each group reading one 256-byte bank row = 16 slots.  Slot of
//   (row r, half h) is 2 r + (h ^ (r >> 3 & 1)) modulo 16: rows r and r + 8 of a group share 2 r mod 16 and differ in bit 3, so the XOR sends them to the
//   two slots of the pair -- 16 lanes, 16 slots, no conflict, and no padding (two buffers of the NT = 4 instance are 48 KiB).
//   Two LDS buffers: chunk it + 1 is fetched into registers under the MFMAs of chunk it and stored to the other buffer behind them, ONE barrier per chunk.
//   Everything outside the problem -- a channel past Cin, an output channel past Cout, a voxel past the end, a tap on the zero padding -- is fetched as
//   0.f, whose three pieces are zero: a zero in both operands' pieces, never LDS garbage.  A padded tap is multiplied, not skipped.  The order of
//   additions of an output element is (tap, chunk, piece pair) and the MFMA's own order over the 16 channels: nothing of its row, tile or batch.
//
// The wide geometries (gemm_conv_supported_wide of kernels_gemm.h: the 19-frame reducer's 5x5x5 and mirrored layers, probav_engine_set_gemm_exotic) run on this kernel too:
//   the mirrored depth index is a branch on the uniform g.reflect_t, everything else follows from the geometry.
//
// The backward-filter stays on the fp32 route (gemm_conv_wgrad_kernel): an x6 form of it -- both operands cut per tap, 27 times per voxel -- was measured
// slower than the fp32 kernel and is not part of this unit ('The general matrix route').
#include "probav_common.h"
#include "kernels_gemm.h"
#include "kernels_gemm_x6.h"
#include "x6_device.h"

namespace probav {

__device__ __forceinline__ int gx_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * n - 2 - i : i;
}

// One K step of 16 in mac<X6>'s order, smallest terms first, on TWO accumulators: `hi` takes the leading product a0 b0, `lo` the five terms below it (2^-8
// and 2^-16 of it).  Every MFMA rounds its sum to the accumulator's magnitude; a general K runs to hundreds of steps (27 taps x Cin / 16), and six roundings
// per step at the full sum's magnitude add up to the fp32 kernels' error several times over.  Apart, the five small terms round at 2^-8 of that magnitude
// and only the leading one at the sum's: one rounding per step instead of six.  hi + lo is formed once, in the epilogue.
__device__ __forceinline__ void gx_mac(const Frag (&a)[3], const Frag (&b)[3], f32x16& hi, f32x16& lo)
{
    lo = MFMA16(a[2], b[0], lo);
    lo = MFMA16(a[1], b[1], lo);
    lo = MFMA16(a[0], b[2], lo);
    lo = MFMA16(a[1], b[0], lo);
    lo = MFMA16(a[0], b[1], lo);
    hi = MFMA16(a[0], b[0], hi);
}

// ---------------------------------------------------------------------------------------------------
// forward / backward-data
// ---------------------------------------------------------------------------------------------------
constexpr int GX_BM = 128;                  // voxels per workgroup          (= GF_BM of kernels_gemm.hip: the plan report is shared)
constexpr int GX_KC = 16;                   // input channels per K chunk    (= GF_KC)
constexpr int GX_ROW = 2 * GX_KC;           // bytes of a plane row

__device__ __forceinline__ int gx_slot(int row, int h) { return row * GX_ROW + 16 * (h ^ ((row >> 3) & 1)); }

template <int NT, bool GATE>
__global__ __launch_bounds__(256) void gemm_conv_fwd_x6_kernel(ConvGeom g, const float* __restrict__ x, const float* __restrict__ gate, const float* __restrict__ w,
                                                               const float* __restrict__ bias, const float* __restrict__ skip, float* __restrict__ y)
{
    constexpr int BN = 32 * NT;
    constexpr int KPT = 2 * NT;                        // consecutive input channels of one output channel a thread fetches per chunk (256 KPT = 16 BN)
    constexpr int A_PL = GX_BM * GX_ROW, B_PL = BN * GX_ROW;      // bytes of a piece plane
    constexpr int BUF = 3 * (A_PL + B_PL);
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long nvox = (long)g.N * g.Ho * g.Wo * g.To;
    const long m0 = (long)blockIdx.x * GX_BM;
    const int co0 = blockIdx.y * BN;
    const int taps = g.kh * g.kw * g.kt;
    const int nchunk = (g.Cin + GX_KC - 1) / GX_KC;
    const int niter = taps * nchunk;
    // (uniform) a row's channels in 16-byte loads: every offset below is then a multiple of four floats, on bases that are 16-byte aligned themselves
    const bool vec = (g.Cin & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | (GATE ? reinterpret_cast<uintptr_t>(gate) : (uintptr_t)0)) & 15) == 0;

    // A: this thread fetches channels [8 ah, 8 ah + 8) of the chunk at row arow; vn < 0 past the end
    const int arow = tid >> 1, ah = tid & 1;
    int vn = -1, vh = 0, vw = 0, vt = 0;
    {
        long r = m0 + arow;
        if (r < nvox) {
            vt = (int)(r % g.To); r /= g.To;
            vw = (int)(r % g.Wo); r /= g.Wo;
            vh = (int)(r % g.Ho);
            vn = (int)(r / g.Ho);
        }
    }
    // B: input channels [bk, bk + KPT) of the chunk at output channel co0 + bn
    const int bn = tid % BN, bk = (tid / BN) * KPT;

    float ra[8], rg[8], rb[KPT];
    auto fetch = [&](int it) {
        const int tap = it / nchunk, c0 = (it - tap * nchunk) * GX_KC;
        const int a = tap / (g.kw * g.kt), b = (tap / g.kt) % g.kw, c = tap % g.kt;
        const int ch = c0 + 8 * ah;
#pragma unroll
        for (int j = 0; j < 8; ++j) { ra[j] = 0.f; rg[j] = 1.f; }
        if (vn >= 0 && ch < g.Cin) {
            int ih = vh + a - g.ph, iw = vw + b - g.pw;
            int id = vt + c - g.pt;
            bool pad = false;
            if (g.reflect_t) id = gx_reflect(id, g.Ti);                // (uniform) the mirrored depth pad of the wide geometries: no tap of it is padding
            else pad = id < 0 || id >= g.Ti;
            if (g.reflect_hw) { ih = gx_reflect(ih, g.Hi); iw = gx_reflect(iw, g.Wi); }
            else pad = pad || ih < 0 || ih >= g.Hi || iw < 0 || iw >= g.Wi;
            if (!pad) {
                const long off = ((((long)vn * g.Hi + ih) * g.Wi + iw) * g.Ti + id) * g.Cin + ch;
                if (vec) {
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        if (ch + 4 * q < g.Cin) {       // (Cin % 4 == 0: the four are inside together)
                            const float4 v = *reinterpret_cast<const float4*>(x + off + 4 * q);
                            ra[4 * q] = v.x; ra[4 * q + 1] = v.y; ra[4 * q + 2] = v.z; ra[4 * q + 3] = v.w;
                            if (GATE) {
                                const float4 t = *reinterpret_cast<const float4*>(gate + off + 4 * q);
                                rg[4 * q] = t.x; rg[4 * q + 1] = t.y; rg[4 * q + 2] = t.z; rg[4 * q + 3] = t.w;
                            }
                        }
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if (ch + j < g.Cin) {
                            ra[j] = x[off + j];
                            if (GATE) rg[j] = gate[off + j];
                        }
                    }
                }
            }
        }
        const int co = co0 + bn;
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const int ci = c0 + bk + i;
            rb[i] = (ci < g.Cin && co < g.Cout) ? w[((long)tap * g.Cin + ci) * g.Cout + co] : 0.f;
        }
    };
    // the fetched chunk, cut into its pieces, into buffer `buf`
    auto store = [&](unsigned char* buf) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = GATE ? (rg[j] > 0.f ? ra[j] : 0.f) : ra[j];      // the gate as a select: a gated non-finite x is a zero
        Frag f[3];
        cut8<X6>(v, 1.f, f);
#pragma unroll
        for (int p = 0; p < 3; ++p) *reinterpret_cast<uint4*>(buf + p * A_PL + gx_slot(arow, ah)) = f[p].u;
        unsigned q[KPT / 2][3];
#pragma unroll
        for (int i = 0; i < KPT / 2; ++i) split_pair(rb[2 * i], rb[2 * i + 1], q[i][0], q[i][1], q[i][2]);
        unsigned char* bp = buf + 3 * A_PL + gx_slot(bn, bk >> 3) + (bk & 7) * 2;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            if constexpr (NT == 1) *reinterpret_cast<unsigned*>(bp + p * B_PL) = q[0][p];
            else if constexpr (NT == 2) *reinterpret_cast<uint2*>(bp + p * B_PL) = make_uint2(q[0][p], q[1][p]);
            else *reinterpret_cast<uint4*>(bp + p * B_PL) = make_uint4(q[0][p], q[1][p], q[2][p], q[3][p]);
        }
    };

    f32x16 acc[NT], accl[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[nt][r] = 0.f; accl[nt][r] = 0.f; }

    const int mrow = wave * 32 + (lane & 31), mh = lane >> 5;
    fetch(0);
    store(lds);
    __syncthreads();
    for (int it = 0; it < niter; ++it) {
        const unsigned char* cur = lds + (it & 1) * BUF;
        const bool more = it + 1 < niter;
        if (more) fetch(it + 1);                        // the next chunk's loads fly under this chunk's MFMAs
        Frag fa[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) fa[p].u = *reinterpret_cast<const uint4*>(cur + p * A_PL + gx_slot(mrow, mh));
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            Frag fb[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) fb[p].u = *reinterpret_cast<const uint4*>(cur + 3 * A_PL + p * B_PL + gx_slot(nt * 32 + (lane & 31), mh));
            gx_mac(fa, fb, acc[nt], accl[nt]);
        }
        if (more) store(lds + ((it + 1) & 1) * BUF);    // the other buffer: every wave left it at the barrier that ended chunk it - 1
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
            const long v = m0 + wave * 32 + rowmap(r, lane >> 5);
            if (v >= nvox) continue;
            float o = (acc[nt][r] + accl[nt][r]) + bv;
            if (g.relu) o = relu_keep_nan(o);
            if (skip) o += skip[v * g.Cout + co];
            y[v * g.Cout + co] = o;
        }
    }
}

bool gemm_x6_conv_plan_ints(const ConvGeom& g, int v[6])
{
    if (!gemm_conv_plan_ints(g, v)) return false;
    return v[0] == GX_BM && v[4] == GX_KC;              // the fp32 route's tiles: one report for both arithmetics
}

bool gemm_x6_conv_plan_ints_wide(const ConvGeom& g, int v[6])
{
    if (!gemm_conv_plan_ints_wide(g, v)) return false;
    return v[0] == GX_BM && v[4] == GX_KC;
}

static int gemm_x6_conv_launch(const ConvGeom& g, const int v[6], const float* x, const float* gate, const float* w, const float* bias, const float* skip, float* y, hipStream_t s);

int gemm_x6_conv_forward(const ConvGeom& g, const float* x, const float* gate, const float* w, const float* bias, const float* skip, float* y, hipStream_t s)
{
    int v[6];
    if (!gemm_x6_conv_plan_ints(g, v)) { set_error("gemm_x6_conv_forward: geometry not supported", hipSuccess); return PROBAV_EINVAL; }
    return gemm_x6_conv_launch(g, v, x, gate, w, bias, skip, y, s);
}

int gemm_x6_conv_forward_wide(const ConvGeom& g, const float* x, const float* gate, const float* w, const float* bias, const float* skip, float* y, hipStream_t s)
{
    int v[6];
    if (!gemm_x6_conv_plan_ints_wide(g, v)) { set_error("gemm_x6_conv_forward_wide: geometry not supported", hipSuccess); return PROBAV_EINVAL; }
    return gemm_x6_conv_launch(g, v, x, gate, w, bias, skip, y, s);
}

static int gemm_x6_conv_launch(const ConvGeom& g, const int v[6], const float* x, const float* gate, const float* w, const float* bias, const float* skip, float* y, hipStream_t s)
{
    if (v[3] > 65535) { set_error("gemm_x6_conv_forward: Cout too large", hipSuccess); return PROBAV_EINVAL; }
    const dim3 grid((unsigned)v[2], (unsigned)v[3]), block(256);
#define PROBAV_GX(NT) do { \
        if (gate) hipLaunchKernelGGL((gemm_conv_fwd_x6_kernel<NT, true>), grid, block, 0, s, g, x, gate, w, bias, skip, y); \
        else hipLaunchKernelGGL((gemm_conv_fwd_x6_kernel<NT, false>), grid, block, 0, s, g, x, gate, w, bias, skip, y); } while (0)
    switch (gemm_fwd_nt(g)) {
    case 1: PROBAV_GX(1); break;
    case 2: PROBAV_GX(2); break;
    default: PROBAV_GX(4); break;
    }
#undef PROBAV_GX
    return check_launch("gemm_conv_fwd_x6");
}

}  // namespace probav
