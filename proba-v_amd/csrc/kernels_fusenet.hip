// FuseNet (gfx950): the reference's learned stitching network (models/modelsTF.py:391-474, FuseNetv3) -- one 48 x 48 convolution of the
// stitched image with 64 filters, an instance normalisation, LeakyReLU(0.3), the channel mean, added to the image.  proba-v_amd/fusenet_numpy.py
// states the forward and the backward in fp64; INTEGRATION.md, 'FuseNet', has the definition.
//
//   y[b,r,s,c]   = sum_{i,j < 48} x[b, r+i-23, s+j-23] K[i,j,0,c]     zero outside the image (TF 'SAME': 23 before, 24 after).  NO bias: it cancels
//                                                                     in y - mu, so the kernels never read it and its gradient is exact zeros
//   mu, var      = mean and biased variance of y[b,:,:,c];  rstd = 1 / sqrt(var + 1e-3)
//   m[b,r,s]     = (1/64) sum_c leaky(gamma[c] (y - mu) rstd + beta[c]);   out = x + m  (residual) or m
// y is kept channel-innermost, [B][H][W][64] (the library's activation layout); stats [B][64][2] = (mu, rstd).
//
// Arithmetic: the fp32-input MFMA (v_mfma_f32_32x32x2_f32 forward, v_mfma_f32_16x16x4_f32 filter gradient), an exact fp32 fma chain.  No operand
// scaling, so a sample's bits cannot depend on its batch.  The forward sums the 48 products of one filter row in an accumulator of their own and
// adds the 48 row sums: two chains of 48 instead of one of 2304.  Every reduction across threads, waves or workgroups (the statistics, the
// gradient slabs) is fp64 in a fixed order, no floating-point atomics: the bits do not depend on the launch order.
//
// Forward convolution, an implicit GEMM (M = 32 pixels of an image row, N = 64, K = 2304).  A workgroup of 4 waves owns a 16 x 32 pixel tile: the
// image tile with its 47-pixel halo is staged in LDS once (63 x 79 floats), the filter is streamed one row (48 taps x 64 channels, 12 KiB) at a
// time through two LDS buffers.  Wave w owns rows 4w .. 4w+3 of the tile (four M tiles) and both N tiles.  Operand reads (ds_read_b32):
//   A[m = lane & 31][k = lane >> 5] = X[row + i][m + j + k]        consecutive lanes, consecutive words; the two halves overlap in 31 words (broadcast)
//   B[k][n = lane & 31]             = F[(j + k) * 96 + n]          row pitch 96 words: the two k rows of one read fall in different bank halves
// 6 reads feed 8 MFMAs of 64 cycles each.
//
// Filter gradient, a GEMM with M = 48 taps j of one filter row, N = 64 channels, K = pixels, on 16x16x4 tiles (48 = 3 x 16).  A workgroup owns 16
// filter rows (grid.x = 3) and one slab of pixel tiles (grid.y); wave w owns filter rows 4w .. 4w+3 of the group: 4 x 3 x 4 accumulator tiles of 4
// registers.  Per pixel tile (2 rows x 64 columns) the workgroup stages the image rows its filter rows reach (17 x 111 floats) and dy, FORMED HERE
// from y, g and the statistics (never written to memory), as [pixel][64] with pitch 80.  Reads:
//   A[j = lane & 15][k = lane >> 4] = X[row][s + k + 16 jt + j]      at most 19 distinct consecutive words
//   B[k][c = lane & 15]             = DY[(s + k) * 80 + 16 ct + c]   pitch 80: the four k rows fall in four different bank quarters
// A slab is written as [2304][64] floats; fusenet_reduce sums the slabs in fp64 in slab order.
#include "probav_common.h"
#include "../../include/probav_hip.h"

namespace probav {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int FK = 48, FC = 64, FPAD = 23;                    // filter side, filters, pad before
constexpr int FTAPS = FK * FK;
constexpr long FN_KERNEL = (long)FTAPS * FC;                // 147 456
constexpr long FN_FLAT = FN_KERNEL + 3 * FC;                // + bias, gamma, beta = 147 648
constexpr long OFF_BIAS = FN_KERNEL, OFF_GAMMA = FN_KERNEL + FC, OFF_BETA = FN_KERNEL + 2 * FC;
constexpr float IN_EPS = 1e-3f, LEAK = 0.3f;

// ---- forward convolution --------------------------------------------------------------------------------------------------------
constexpr int CT_R = 16, CT_C = 32;                           // pixel tile of a workgroup
constexpr int CX_R = CT_R + FK - 1, CX_C = CT_C + FK - 1;     // 63 x 79 with the halo
constexpr int CX_P = 80;                                      // row pitch of the image tile (floats)
constexpr int CF_P = 96;                                      // row pitch of a filter row's [48][64] (floats)
constexpr int CF_BUF = FK * CF_P;
constexpr size_t CONV_LDS = (size_t)(CX_R * CX_P + 2 * CF_BUF) * sizeof(float);      // 57 024 bytes

__global__ __launch_bounds__(256) void fusenet_conv_fwd(const float* __restrict__ x, const float* __restrict__ filt, float* __restrict__ y,
                                                        double* __restrict__ part, int H, int W)
{
    extern __shared__ float lds[];
    float* X = lds;
    float* F = lds + CX_R * CX_P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, r0 = blockIdx.y * CT_R, s0 = blockIdx.x * CT_C;
    const float* xb = x + (size_t)b * H * W;
    for (int e = tid; e < CX_R * CX_P; e += 256) {
        const int rr = e / CX_P, cc = e - rr * CX_P;
        const int gr = r0 + rr - FPAD, gc = s0 + cc - FPAD;
        float v = 0.f;
        if (cc < CX_C && gr >= 0 && gr < H && gc >= 0 && gc < W) v = xb[(size_t)gr * W + gc];
        X[e] = v;
    }
    // one filter row = 768 float4, three per thread; float4 q -> tap q >> 4, channels 4 (q & 15)
    float4 nxt[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) nxt[u] = reinterpret_cast<const float4*>(filt)[tid + 256 * u];
#pragma unroll
    for (int u = 0; u < 3; ++u) { const int q = tid + 256 * u; *reinterpret_cast<float4*>(F + (q >> 4) * CF_P + 4 * (q & 15)) = nxt[u]; }
    __syncthreads();

    f32x16 tot[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[mt][nt][r] = 0.f;
    const int m = lane & 31, h = lane >> 5;
    for (int i = 0; i < FK; ++i) {
        if (i + 1 < FK) {
#pragma unroll
            for (int u = 0; u < 3; ++u) nxt[u] = reinterpret_cast<const float4*>(filt + (size_t)(i + 1) * FK * FC)[tid + 256 * u];
        }
        const float* Fi = F + (i & 1) * CF_BUF + h * CF_P + m;
        const float* Xi = X + (4 * wave + i) * CX_P + m + h;
        f32x16 acc[4][2];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
#pragma unroll 4
        for (int j = 0; j < FK; j += 2) {
            const float b0 = Fi[j * CF_P], b1 = Fi[j * CF_P + 32];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const float a = Xi[mt * CX_P + j];
                acc[mt][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[mt][0], 0, 0, 0);
                acc[mt][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[mt][1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) tot[mt][nt] += acc[mt][nt];
        if (i + 1 < FK) {
            float* Fn = F + ((i + 1) & 1) * CF_BUF;             // last read as row i - 1, before the barrier that ended that iteration
#pragma unroll
            for (int u = 0; u < 3; ++u) { const int q = tid + 256 * u; *reinterpret_cast<float4*>(Fn + (q >> 4) * CF_P + 4 * (q & 15)) = nxt[u]; }
        }
        __syncthreads();
    }

    // D[m][n]: n = lane & 31 (channel), m = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (pixel column)
    double s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0};
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int r = r0 + 4 * wave + mt;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int s = s0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            if (r < H && s < W) {
                float* dst = y + (((size_t)b * H + r) * W + s) * FC + m;
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const float v = tot[mt][nt][reg];
                    dst[32 * nt] = v;
                    s1[nt] += (double)v;
                    s2[nt] += (double)v * (double)v;
                }
            }
        }
    }
    // per (tile, channel) partial sums: lane halves, then the four waves, in that order
    double* R = reinterpret_cast<double*>(F);                    // the filter buffers are free: the loop ended on a barrier
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const double o1 = __shfl_xor(s1[nt], 32, 64), o2 = __shfl_xor(s2[nt], 32, 64);
        if (h == 0) {
            R[(wave * FC + 32 * nt + m) * 2 + 0] = s1[nt] + o1;
            R[(wave * FC + 32 * nt + m) * 2 + 1] = s2[nt] + o2;
        }
    }
    __syncthreads();
    if (tid < 2 * FC) {
        const double v = ((R[tid] + R[2 * FC + tid]) + R[4 * FC + tid]) + R[6 * FC + tid];
        const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x, ntile = (size_t)gridDim.x * gridDim.y;
        part[((size_t)b * ntile + tile) * 2 * FC + tid] = v;
    }
}

// partials [B][n][64][2] (sum, sum of squares) -> stats [B][64][2] = (mu, 1 / sqrt(var + eps)); one workgroup per sample, thread = channel
__global__ __launch_bounds__(64) void fusenet_stats_finish(const double* __restrict__ part, int n, double npix, float* __restrict__ stats)
{
    const int b = blockIdx.x, c = threadIdx.x;
    const double* p = part + (size_t)b * n * 2 * FC + 2 * c;
    double s1 = 0.0, s2 = 0.0;
    for (int t = 0; t < n; ++t) { s1 += p[(size_t)t * 2 * FC]; s2 += p[(size_t)t * 2 * FC + 1]; }
    const double mu = s1 / npix;
    double var = s2 / npix - mu * mu;
    var = var < 0.0 ? 0.0 : var;                                  // (NaN stays NaN)
    stats[((size_t)b * FC + c) * 2 + 0] = (float)mu;
    stats[((size_t)b * FC + c) * 2 + 1] = (float)(1.0 / sqrt(var + (double)IN_EPS));
}

__device__ __forceinline__ float leaky(float a) { return a >= 0.f ? a : LEAK * a; }         // NaN goes through (0.3 NaN)

// ---- forward epilogue: normalise, scale, LeakyReLU, channel mean, optional + x.  16 lanes per pixel, 4 channels per lane ----
__global__ __launch_bounds__(256) void fusenet_epilogue(const float* __restrict__ y, const float* __restrict__ stats, const float* __restrict__ flat,
                                                        const float* __restrict__ x, float* __restrict__ out, size_t npix_sample, size_t npix, int residual)
{
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t p = gid >> 4;
    const int cg = (int)(gid & 15);
    const bool live = p < npix;
    float part = 0.f;
    if (live) {
        const size_t b = p / npix_sample;
        const float4 v = reinterpret_cast<const float4*>(y)[p * 16 + cg];
        const float4 st0 = reinterpret_cast<const float4*>(stats)[(b * FC + 4 * cg) / 2], st1 = reinterpret_cast<const float4*>(stats)[(b * FC + 4 * cg) / 2 + 1];
        const float4 ga = reinterpret_cast<const float4*>(flat + OFF_GAMMA)[cg], be = reinterpret_cast<const float4*>(flat + OFF_BETA)[cg];
        const float l0 = leaky(ga.x * ((v.x - st0.x) * st0.y) + be.x);
        const float l1 = leaky(ga.y * ((v.y - st0.z) * st0.w) + be.y);
        const float l2 = leaky(ga.z * ((v.z - st1.x) * st1.y) + be.z);
        const float l3 = leaky(ga.w * ((v.w - st1.z) * st1.w) + be.w);
        part = (l0 + l1) + (l2 + l3);
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) part += __shfl_xor(part, o, 64);          // the same butterfly on every lane: one order, whatever the batch
    if (live && cg == 0) {
        const float mval = part * (1.f / FC);
        out[p] = residual ? x[p] + mval : mval;
    }
}

// ---- backward statistics: per (sample, chunk of pixels, channel) sum of da and of da * xhat, fp64 ----
constexpr int BS_CHUNK = 4096;                                // pixels per workgroup
__global__ __launch_bounds__(256) void fusenet_bwd_stats(const float* __restrict__ y, const float* __restrict__ g, const float* __restrict__ stats,
                                                         const float* __restrict__ flat, double* __restrict__ part, int npix_sample)
{
    __shared__ double R[16 * 2 * FC];
    const int tid = threadIdx.x, cg = tid & 15, pl = tid >> 4;
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int p0 = chunk * BS_CHUNK, p1 = min(p0 + BS_CHUNK, npix_sample);
    const float4 st0 = reinterpret_cast<const float4*>(stats)[((size_t)b * FC + 4 * cg) / 2], st1 = reinterpret_cast<const float4*>(stats)[((size_t)b * FC + 4 * cg) / 2 + 1];
    const float4 ga = reinterpret_cast<const float4*>(flat + OFF_GAMMA)[cg], be = reinterpret_cast<const float4*>(flat + OFF_BETA)[cg];
    const float mu[4] = {st0.x, st0.z, st1.x, st1.z}, rs[4] = {st0.y, st0.w, st1.y, st1.w};
    const float gam[4] = {ga.x, ga.y, ga.z, ga.w}, bet[4] = {be.x, be.y, be.z, be.w};
    double a1[4] = {0.0, 0.0, 0.0, 0.0}, a2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = p0 + pl; p < p1; p += 16) {
        const size_t gp = (size_t)b * npix_sample + p;
        const float4 v4 = reinterpret_cast<const float4*>(y)[gp * 16 + cg];
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
        const float dl = g[gp] * (1.f / FC);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float xh = (v[k] - mu[k]) * rs[k];
            const float a = gam[k] * xh + bet[k];
            const float da = a >= 0.f ? dl : LEAK * dl;
            a1[k] += (double)da;
            a2[k] += (double)da * (double)xh;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { R[(pl * FC + 4 * cg + k) * 2 + 0] = a1[k]; R[(pl * FC + 4 * cg + k) * 2 + 1] = a2[k]; }
    __syncthreads();
    if (tid < 2 * FC) {
        double v = 0.0;
        for (int q = 0; q < 16; ++q) v += R[q * 2 * FC + tid];
        part[(((size_t)b * gridDim.x + chunk) * FC) * 2 + tid] = v;
    }
}

// partials [B][n][64][2] -> sums [B][64][2] fp64 (sum da, sum da xhat) and bst [B][64][2] fp32 = (S1 / N, S2 / N) with S = gamma * sum
__global__ __launch_bounds__(64) void fusenet_bwd_finish(const double* __restrict__ part, int n, double npix, const float* __restrict__ flat,
                                                         double* __restrict__ sums, float* __restrict__ bst)
{
    const int b = blockIdx.x, c = threadIdx.x;
    const double* p = part + (size_t)b * n * 2 * FC + 2 * c;
    double a1 = 0.0, a2 = 0.0;
    for (int t = 0; t < n; ++t) { a1 += p[(size_t)t * 2 * FC]; a2 += p[(size_t)t * 2 * FC + 1]; }
    sums[((size_t)b * FC + c) * 2 + 0] = a1;
    sums[((size_t)b * FC + c) * 2 + 1] = a2;
    const double gm = (double)flat[OFF_GAMMA + c];
    bst[((size_t)b * FC + c) * 2 + 0] = (float)(gm * a1 / npix);
    bst[((size_t)b * FC + c) * 2 + 1] = (float)(gm * a2 / npix);
}

// ---- filter gradient ------------------------------------------------------------------------------------------------------------
constexpr int WT_R = 2, WT_C = 64;                            // pixel tile
constexpr int WG_ROWS = 16;                                   // filter rows of a workgroup (4 per wave)
constexpr int WX_R = WT_R + WG_ROWS - 1;                      // 17 image rows
constexpr int WX_C = WT_C + FK - 1, WX_P = 112;               // 111 columns
constexpr int WD_P = 80;                                      // pitch of a pixel's 64 dy values
constexpr size_t WGRAD_LDS = (size_t)(WX_R * WX_P + WT_R * WT_C * WD_P) * sizeof(float);      // 48 576 bytes

__global__ __launch_bounds__(256) void fusenet_wgrad(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g,
                                                     const float* __restrict__ stats, const float* __restrict__ bst, const float* __restrict__ flat,
                                                     float* __restrict__ slabs, int B, int H, int W, int tiles_x, int tiles_y)
{
    extern __shared__ float lds[];
    float* X = lds;
    float* DY = lds + WX_R * WX_P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ig = blockIdx.x * WG_ROWS;                          // first filter row of this workgroup
    const long tps = (long)tiles_x * tiles_y, ntiles = tps * B;
    const long t0 = ntiles * blockIdx.y / gridDim.y, t1 = ntiles * (blockIdx.y + 1) / gridDim.y;
    const float4 ga = reinterpret_cast<const float4*>(flat + OFF_GAMMA)[tid & 15], be = reinterpret_cast<const float4*>(flat + OFF_BETA)[tid & 15];
    const float gam[4] = {ga.x, ga.y, ga.z, ga.w}, bet[4] = {be.x, be.y, be.z, be.w};

    f32x4 acc[4][3][4];
#pragma unroll
    for (int il = 0; il < 4; ++il)
#pragma unroll
        for (int jt = 0; jt < 3; ++jt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[il][jt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int l15 = lane & 15, k4 = lane >> 4;

    for (long t = t0; t < t1; ++t) {
        const int b = (int)(t / tps);
        const int rem = (int)(t - (long)b * tps), ty = rem / tiles_x, tx = rem - ty * tiles_x;
        const int r0 = ty * WT_R, s0 = tx * WT_C;
        __syncthreads();                                           // the previous tile's reads are done
        const float* xb = x + (size_t)b * H * W;
        for (int e = tid; e < WX_R * WX_P; e += 256) {
            const int rr = e / WX_P, cc = e - rr * WX_P;
            const int gr = r0 + ig + rr - FPAD, gc = s0 + cc - FPAD;
            float v = 0.f;
            if (cc < WX_C && gr >= 0 && gr < H && gc >= 0 && gc < W) v = xb[(size_t)gr * W + gc];
            X[e] = v;
        }
        {
            const int cg = tid & 15;
            const float4 st0 = reinterpret_cast<const float4*>(stats)[((size_t)b * FC + 4 * cg) / 2], st1 = reinterpret_cast<const float4*>(stats)[((size_t)b * FC + 4 * cg) / 2 + 1];
            const float4 bs0 = reinterpret_cast<const float4*>(bst)[((size_t)b * FC + 4 * cg) / 2], bs1 = reinterpret_cast<const float4*>(bst)[((size_t)b * FC + 4 * cg) / 2 + 1];
            const float mu[4] = {st0.x, st0.z, st1.x, st1.z}, rs[4] = {st0.y, st0.w, st1.y, st1.w};
            const float m1[4] = {bs0.x, bs0.z, bs1.x, bs1.z}, m2[4] = {bs0.y, bs0.w, bs1.y, bs1.w};
#pragma unroll
            for (int u = 0; u < WT_R * WT_C * 16 / 256; ++u) {
                const int px = (tid >> 4) + 16 * u;               // 0 .. 127
                const int r = r0 + (px >> 6), s = s0 + (px & 63);
                float d[4] = {0.f, 0.f, 0.f, 0.f};
                if (r < H && s < W) {
                    const size_t gp = ((size_t)b * H + r) * W + s;
                    const float4 v4 = reinterpret_cast<const float4*>(y)[gp * 16 + cg];
                    const float v[4] = {v4.x, v4.y, v4.z, v4.w};
                    const float dl = g[gp] * (1.f / FC);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float xh = (v[k] - mu[k]) * rs[k];
                        const float a = gam[k] * xh + bet[k];
                        const float da = a >= 0.f ? dl : LEAK * dl;
                        d[k] = (da * gam[k] - m1[k] - xh * m2[k]) * rs[k];
                    }
                }
                *reinterpret_cast<float4*>(DY + px * WD_P + 4 * cg) = make_float4(d[0], d[1], d[2], d[3]);
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int rr = 0; rr < WT_R; ++rr) {
            const float* Xr = X + (rr + 4 * wave) * WX_P + k4 + l15;
            const float* Dr = DY + (rr * WT_C + k4) * WD_P + l15;
#pragma unroll 2
            for (int s = 0; s < WT_C; s += 4) {
                float bf[4];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) bf[ct] = Dr[s * WD_P + 16 * ct];
#pragma unroll
                for (int il = 0; il < 4; ++il)
#pragma unroll
                    for (int jt = 0; jt < 3; ++jt) {
                        const float a = Xr[il * WX_P + s + 16 * jt];
#pragma unroll
                        for (int ct = 0; ct < 4; ++ct) acc[il][jt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bf[ct], acc[il][jt][ct], 0, 0, 0);
                    }
            }
        }
    }
    // D[j][c]: c = lane & 15, j = 4 (lane >> 4) + reg
    float* slab = slabs + (size_t)blockIdx.y * FN_KERNEL;
#pragma unroll
    for (int il = 0; il < 4; ++il) {
        const int i = ig + 4 * wave + il;
#pragma unroll
        for (int jt = 0; jt < 3; ++jt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int j = 16 * jt + 4 * k4 + reg;
                    slab[((size_t)i * FK + j) * FC + 16 * ct + l15] = acc[il][jt][ct][reg];
                }
    }
}

// dflat: the kernel = the slabs summed in fp64 in slab order; bias = exact zeros; gamma, beta = the per-sample sums over the batch, in order
__global__ __launch_bounds__(256) void fusenet_reduce(const float* __restrict__ slabs, int nslab, const double* __restrict__ sums, int B, float* __restrict__ dflat)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= FN_FLAT) return;
    if (e < FN_KERNEL) {
        double v = 0.0;
        for (int q = 0; q < nslab; ++q) v += (double)slabs[(size_t)q * FN_KERNEL + e];
        dflat[e] = (float)v;
    } else if (e < OFF_GAMMA) {
        dflat[e] = 0.f;
    } else {
        const int c = (int)((e - OFF_GAMMA) & (FC - 1)), which = e < OFF_BETA ? 1 : 0;      // dgamma = sum da xhat, dbeta = sum da
        double v = 0.0;
        for (int b = 0; b < B; ++b) v += sums[((size_t)b * FC + c) * 2 + which];
        dflat[e] = (float)v;
    }
}

// ---- host-side geometry ----
struct FuseGeom {
    int B, H, W;
    int ctx, cty;               // forward tiles
    int chunks;                 // backward-statistics chunks per sample
    int wtx, wty, nslab;        // filter-gradient tiles per sample, slabs
    size_t off_part, off_sums, off_bst, off_slabs, bytes_fwd, bytes_bwd;
};
constexpr int MAX_SLABS = 84;                                 // x 3 filter-row groups = 252 workgroups: one round of a 256-CU device

bool fuse_geom(int B, int H, int W, FuseGeom& q)
{
    if (B < 1 || H < 1 || W < 1 || B > 65535 || H > 32768 || W > 32768 || (int64_t)B * H * W > 0x7fffffffLL / 64) return false;
    q.B = B; q.H = H; q.W = W;
    q.ctx = (W + CT_C - 1) / CT_C; q.cty = (H + CT_R - 1) / CT_R;
    q.chunks = (int)(((int64_t)H * W + BS_CHUNK - 1) / BS_CHUNK);
    q.wtx = (W + WT_C - 1) / WT_C; q.wty = (H + WT_R - 1) / WT_R;
    const int64_t ntiles = (int64_t)q.wtx * q.wty * B;
    q.nslab = (int)(ntiles < MAX_SLABS ? ntiles : MAX_SLABS);
    const size_t nfwd = (size_t)B * q.ctx * q.cty * 2 * FC * sizeof(double), nbwd = (size_t)B * q.chunks * 2 * FC * sizeof(double);
    q.off_part = 0;
    q.bytes_fwd = nfwd;
    q.off_sums = nbwd;
    q.off_bst = q.off_sums + (size_t)B * 2 * FC * sizeof(double);
    q.off_slabs = q.off_bst + (size_t)B * 2 * FC * sizeof(float);                  // (a multiple of 16 bytes)
    q.bytes_bwd = q.off_slabs + (size_t)q.nslab * FN_KERNEL * sizeof(float);
    return true;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

}  // namespace probav

using namespace probav;

extern "C" size_t probav_fusenet_workspace_bytes(int batch, int H, int W, int backward)
{
    FuseGeom q;
    if (!fuse_geom(batch, H, W, q)) return 0;
    return backward ? q.bytes_bwd : q.bytes_fwd;
}

extern "C" int probav_fusenet_forward(const float* x, const float* flat, int64_t flat_count, int batch, int H, int W, int residual, float* out, float* y,
                                      float* stats, void* workspace, size_t workspace_bytes, void* stream)
{
    FuseGeom q;
    if (!x || !flat || !out || !y || !stats || !workspace || flat_count != FN_FLAT || !fuse_geom(batch, H, W, q) || !aligned16(flat) || !aligned16(y) ||
        !aligned16(stats) || !aligned16(workspace)) {
        set_error("probav_fusenet_forward: null/invalid argument (batch, H, W >= 1; batch <= 65535; H, W <= 32768; batch H W 64 < 2^31; flat_count == 147648; "
                  "flat, y, stats and workspace 16-byte aligned)", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (workspace_bytes < q.bytes_fwd) {
        set_error("probav_fusenet_forward: workspace smaller than probav_fusenet_workspace_bytes(batch, H, W, 0)", hipSuccess);
        return PROBAV_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(workspace);
    int rc = launch_lds<fusenet_conv_fwd>("fusenet_conv_fwd", dim3(q.ctx, q.cty, batch), dim3(256), CONV_LDS, s, x, flat, y, part, H, W);
    if (rc) return rc;
    hipLaunchKernelGGL(fusenet_stats_finish, dim3(batch), dim3(64), 0, s, (const double*)part, q.ctx * q.cty, (double)H * (double)W, stats);
    rc = check_launch("fusenet_stats_finish");
    if (rc) return rc;
    const size_t npix = (size_t)batch * H * W;
    hipLaunchKernelGGL(fusenet_epilogue, dim3((unsigned)((npix * 16 + 255) / 256)), dim3(256), 0, s, (const float*)y, (const float*)stats, flat, x, out,
                       (size_t)H * W, npix, residual ? 1 : 0);
    return check_launch("fusenet_epilogue");
}

extern "C" int probav_fusenet_backward(const float* g, const float* x, const float* y, const float* stats, const float* flat, int64_t flat_count, int batch,
                                       int H, int W, float* dflat, void* workspace, size_t workspace_bytes, void* stream)
{
    FuseGeom q;
    if (!g || !x || !y || !stats || !flat || !dflat || !workspace || flat_count != FN_FLAT || !fuse_geom(batch, H, W, q) || !aligned16(flat) || !aligned16(y) ||
        !aligned16(stats) || !aligned16(workspace)) {
        set_error("probav_fusenet_backward: null/invalid argument (batch, H, W >= 1; batch <= 65535; H, W <= 32768; batch H W 64 < 2^31; flat_count == 147648; "
                  "flat, y, stats and workspace 16-byte aligned)", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (workspace_bytes < q.bytes_bwd) {
        set_error("probav_fusenet_backward: workspace smaller than probav_fusenet_workspace_bytes(batch, H, W, 1)", hipSuccess);
        return PROBAV_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(workspace);
    double* part = reinterpret_cast<double*>(ws + q.off_part);
    double* sums = reinterpret_cast<double*>(ws + q.off_sums);
    float* bst = reinterpret_cast<float*>(ws + q.off_bst);
    float* slabs = reinterpret_cast<float*>(ws + q.off_slabs);
    hipLaunchKernelGGL(fusenet_bwd_stats, dim3(q.chunks, batch), dim3(256), 0, s, y, g, stats, flat, part, H * W);
    int rc = check_launch("fusenet_bwd_stats");
    if (rc) return rc;
    hipLaunchKernelGGL(fusenet_bwd_finish, dim3(batch), dim3(64), 0, s, (const double*)part, q.chunks, (double)H * (double)W, flat, sums, bst);
    rc = check_launch("fusenet_bwd_finish");
    if (rc) return rc;
    rc = launch_lds<fusenet_wgrad>("fusenet_wgrad", dim3(FK / WG_ROWS, q.nslab), dim3(256), WGRAD_LDS, s, x, y, g, stats, (const float*)bst, flat, slabs, batch, H, W,
                                   q.wtx, q.wty);
    if (rc) return rc;
    hipLaunchKernelGGL(fusenet_reduce, dim3((unsigned)((FN_FLAT + 255) / 256)), dim3(256), 0, s, (const float*)slabs, q.nslab, (const double*)sums, batch, dflat);
    return check_launch("fusenet_reduce");
}
