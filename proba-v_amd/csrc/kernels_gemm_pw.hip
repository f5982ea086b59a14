// The general matrix route's fused pointwise pair: expConv (F -> H) + ReLU + decConv (H -> D) of a residual block in one launch, and its reverse, on the
// fp32-input MFMA (v_mfma_f32_32x32x2_f32) for F <= 64, D <= 64 and ANY hidden count H.  The hidden tensor lives in accumulator registers only.
// Operands as the route reads them (kernels_gemm.hip): x [nvox][F], W1 [F][H], W2 [H][D] -- no packed fragments.  DESIGN.md section 4.2.
//
// The rule of kernels_gemm.hip holds here: every element outside the problem that a product SUMS over -- a channel past F, D or H, a voxel past the end
// of a slab -- is a ZERO IN BOTH operands (never LDS or register garbage: 0 x garbage may be NaN).
//
// Hidden channels go 32 at a time (a chunk).  A product's 32 x 32 result has its column on the lane and its rows in the 16 accumulator registers: register r
// of lane half h is row pw_row(r, h).  As the operand of the next MFMA, register r is k-step r, and the two lane halves are its k = 0, 1.  So the first
// product is laid out with the hidden channel on its ROWS, row pw_row(r, h) carrying channel 2 r + h of the chunk (pw_perm): the second product then sums
// the hidden channels in ASCENDING order straight from the registers.
//
// gemm_pw_fwd_kernel   eight waves, each owning 64 voxels (two tiles); the workgroup walks the chunks with W1's and W2's chunk in LDS (double buffered).
//   hidden^T [h][vox] = W1^T x^T, k = input channels ascending, padded to a multiple of 16 as gemm_conv_fwd_kernel pads them; + b1, relu_keep_nan;
//   dec^T [d][vox] += W2^T hidden^T, k = hidden channels ascending over all chunks, padded to a multiple of 16.  Each element is the fma chain of the
//   un-fused route, bit for bit.
// gemm_pw_bwd_data_kernel   the same walk, one tile per wave: hidden^T recomputed (the forward's chain: the forward's gates), dH^T [h][vox] = W2 dT^T,
//   gated, dX^T [k][vox] += W1 dHg^T over all chunks ascending; + dOut.  A voxel's dX reads that voxel's rows only.
// gemm_pw_wgrad_kernel   workgroup (slab, group of eight chunks), wave = chunk, W1's and W2's chunk in registers; the workgroup walks its slab 32 voxels at
//   a time with x's and dT's tile in LDS (double buffered).  hidden [vox][h] and dH [vox][h] (column = hidden channel) are the operands of
//   dW2 [h][d] += hidden^T dT and dW1 [k][h] += x^T dHg as they stand.  db1 from dHg, db2 from dT's tile (last wave of group 0).  One slab per
//   workgroup row; a workgroup without voxels writes zeros.  No atomics.
#include "probav_common.h"
#include "kernels_gemm_pw.h"
#include "x6_device.h"

namespace probav {

#define PW_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
typedef float pw_f32x16 __attribute__((ext_vector_type(16)));

constexpr int PW_NW = 8;                    // waves per workgroup
constexpr int PW_FWD_VT = 2;                // forward: 32-voxel tiles per wave
constexpr int PW_MAX_SLABS = 128;           // bounds the scratch: slabs x (F H + H D + H + D) floats per launch
constexpr long PW_MIN_VOX = 1024;           // a slab is worth a workgroup from here on

// C/D map of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
__device__ __forceinline__ int pw_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }
// the chunk's hidden channel that row i of a [h][vox] product carries: pw_perm(pw_row(r, half)) = 2 r + half
__device__ __forceinline__ int pw_perm(int i) { return 2 * ((i & 3) + 4 * (i >> 3)) + ((i >> 2) & 1); }
__device__ __forceinline__ pw_f32x16 pw_zero()
{
    pw_f32x16 v;
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = 0.f;
    return v;
}

// ---------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------
template <int KT, int ND, bool DUMP>
__global__ __launch_bounds__(512) void gemm_pw_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W1, const float* __restrict__ b1,
                                                          const float* __restrict__ W2, const float* __restrict__ b2, float* __restrict__ dec,
                                                          float* __restrict__ hidden, long nvox, int F, int H, int D)
{
    constexpr int VT = PW_FWD_VT;
    constexpr int DS = 32 * ND + (ND == 2 ? 32 : 0);       // W2 chunk row stride: rows k and k + 1 (the two lane halves of an operand read) 32 banks apart
    constexpr int OFF_W2 = 32 * KT * 32, OFF_B = OFF_W2 + 32 * DS, BUF = OFF_B + 32;
    extern __shared__ float lds[];                          // [2][BUF]: W1 chunk [32 KT][32] | W2 chunk [32][DS] | b1 chunk [32]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, half = lane >> 5;
    const int pi = pw_perm(i);
    const long vw = (long)blockIdx.x * (PW_NW * 32 * VT) + wave * (32 * VT);
    const int Kp = (F + 15) / 16 * 16, Hp = (H + 15) / 16 * 16, nchunk = (H + 31) / 32;

    float xr[VT][16 * KT];                                  // x as the first product's B operand: [k][vox]
#pragma unroll
    for (int t = 0; t < VT; ++t) {
        const long v = vw + t * 32 + i;
#pragma unroll
        for (int s = 0; s < 16 * KT; ++s) {
            const int k = 2 * s + half;
            xr[t][s] = (v < nvox && k < F) ? x[v * F + k] : 0.f;
        }
    }

    float rw1[2 * KT], rw2[2 * ND], rb = 0.f;
    auto fetch = [&](int c) {
        const int h0 = c * 32;
#pragma unroll
        for (int q = 0; q < 2 * KT; ++q) {
            const int e = tid + 512 * q, k = e >> 5, j = e & 31;
            rw1[q] = (k < F && h0 + j < H) ? W1[(long)k * H + h0 + j] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 2 * ND; ++q) {
            const int e = tid + 512 * q, j = e / (32 * ND), d = e % (32 * ND);
            rw2[q] = (d < D && h0 + j < H) ? W2[(long)(h0 + j) * D + d] : 0.f;
        }
        if (tid < 32) rb = h0 + tid < H ? b1[h0 + tid] : 0.f;
    };
    auto stash = [&](int b) {
        float* base = lds + b * BUF;
#pragma unroll
        for (int q = 0; q < 2 * KT; ++q) base[tid + 512 * q] = rw1[q];
#pragma unroll
        for (int q = 0; q < 2 * ND; ++q) {
            const int e = tid + 512 * q, j = e / (32 * ND), d = e % (32 * ND);
            base[OFF_W2 + j * DS + d] = rw2[q];
        }
        if (tid < 32) base[OFF_B + tid] = rb;
    };

    pw_f32x16 accD[VT][ND];
#pragma unroll
    for (int t = 0; t < VT; ++t)
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) accD[t][dt] = pw_zero();

    fetch(0);
    for (int c = 0; c < nchunk; ++c) {
        // (one barrier per chunk: the buffer written here was last read two chunks ago, and every wave has passed the previous chunk's barrier since)
        stash(c & 1);
        __syncthreads();
        if (c + 1 < nchunk) fetch(c + 1);                   // the next chunk's loads fly under this chunk's MFMAs
        const float* Wk = lds + (c & 1) * BUF;
        const float* Wh = Wk + OFF_W2;
        const float* bs = Wk + OFF_B;
        const int h0 = c * 32;

        pw_f32x16 acc1[VT];
#pragma unroll
        for (int t = 0; t < VT; ++t) acc1[t] = pw_zero();
#pragma unroll
        for (int s = 0; s < 16 * KT; ++s) {
            if (2 * s < Kp) {
                const float a = Wk[(2 * s + half) * 32 + pi];
#pragma unroll
                for (int t = 0; t < VT; ++t) acc1[t] = PW_MFMA(a, xr[t][s], acc1[t]);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (h0 + 2 * r < Hp) {                          // (the un-fused route pads the hidden channels to a multiple of 16: the same chain)
                const int hh = h0 + 2 * r + half;
                const float bv = bs[2 * r + half];
                float hc[VT];
#pragma unroll
                for (int t = 0; t < VT; ++t) {
                    hc[t] = relu_keep_nan(acc1[t][r] + bv);
                    if (hh >= H) hc[t] = 0.f;
                    const long v = vw + t * 32 + i;
                    if (DUMP && hh < H && v < nvox) hidden[v * H + hh] = hc[t];
                }
#pragma unroll
                for (int dt = 0; dt < ND; ++dt) {
                    const float a = Wh[(2 * r + half) * DS + dt * 32 + i];
#pragma unroll
                    for (int t = 0; t < VT; ++t) accD[t][dt] = PW_MFMA(a, hc[t], accD[t][dt]);
                }
            }
        }
    }

#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = dt * 32 + pw_row(r, half);
            if (d >= D) continue;
            const float bv = b2[d];
#pragma unroll
            for (int t = 0; t < VT; ++t) {
                const long v = vw + t * 32 + i;
                if (v < nvox) dec[v * D + d] = accD[t][dt][r] + bv;
            }
        }
}

// ---------------------------------------------------------------------------------------------------
// reverse: the input gradient
// ---------------------------------------------------------------------------------------------------
template <int KT, int ND>
__global__ __launch_bounds__(512) void gemm_pw_bwd_data_kernel(const float* __restrict__ x, const float* __restrict__ dT, const float* __restrict__ dOut,
                                                               const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2,
                                                               float* __restrict__ dX, long nvox, int F, int H, int D)
{
    constexpr int JS = 32 * KT + 1;                         // W1 chunk, hidden-channel-major: odd stride (written down its columns, read along its rows)
    constexpr int OFF_WJ = 32 * KT * 32, OFF_W2 = OFF_WJ + 32 * JS, OFF_B = OFF_W2 + 32 * ND * 33, BUF = OFF_B + 32;
    extern __shared__ float lds[];                          // [2][BUF]: W1 chunk [32 KT][32] | W1 chunk [32][JS] | W2 chunk transposed [32 ND][33] | b1 chunk [32]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, half = lane >> 5;
    const int pi = pw_perm(i);
    const long v = (long)blockIdx.x * (PW_NW * 32) + wave * 32 + i;
    const int Kp = (F + 15) / 16 * 16, nchunk = (H + 31) / 32;

    float xr[16 * KT], tr[16 * ND];                         // x and dT as B operands: [k][vox], [d][vox]
#pragma unroll
    for (int s = 0; s < 16 * KT; ++s) {
        const int k = 2 * s + half;
        xr[s] = (v < nvox && k < F) ? x[v * F + k] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < 16 * ND; ++s) {
        const int d = 2 * s + half;
        tr[s] = (v < nvox && d < D) ? dT[v * D + d] : 0.f;
    }

    float rw1[2 * KT], rw2[2 * ND], rb = 0.f;
    auto fetch = [&](int c) {
        const int h0 = c * 32;
#pragma unroll
        for (int q = 0; q < 2 * KT; ++q) {
            const int e = tid + 512 * q, k = e >> 5, j = e & 31;
            rw1[q] = (k < F && h0 + j < H) ? W1[(long)k * H + h0 + j] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 2 * ND; ++q) {
            const int e = tid + 512 * q, j = e / (32 * ND), d = e % (32 * ND);
            rw2[q] = (d < D && h0 + j < H) ? W2[(long)(h0 + j) * D + d] : 0.f;
        }
        if (tid < 32) rb = h0 + tid < H ? b1[h0 + tid] : 0.f;
    };
    auto stash = [&](int b) {
        float* base = lds + b * BUF;
#pragma unroll
        for (int q = 0; q < 2 * KT; ++q) {
            const int e = tid + 512 * q, k = e >> 5, j = e & 31;
            base[e] = rw1[q];
            base[OFF_WJ + j * JS + k] = rw1[q];
        }
#pragma unroll
        for (int q = 0; q < 2 * ND; ++q) {
            const int e = tid + 512 * q, j = e / (32 * ND), d = e % (32 * ND);
            base[OFF_W2 + d * 33 + j] = rw2[q];
        }
        if (tid < 32) base[OFF_B + tid] = rb;
    };

    pw_f32x16 accX[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) accX[kt] = pw_zero();

    fetch(0);
    for (int c = 0; c < nchunk; ++c) {
        stash(c & 1);
        __syncthreads();
        if (c + 1 < nchunk) fetch(c + 1);
        const float* Wk = lds + (c & 1) * BUF;
        const float* Wj = Wk + OFF_WJ;
        const float* Wt = Wk + OFF_W2;
        const float* bs = Wk + OFF_B;
        const int h0 = c * 32;

        // two independent chains: the hidden tile (the forward's chain) and dH
        pw_f32x16 acc1 = pw_zero(), accH = pw_zero();
#pragma unroll
        for (int s = 0; s < 16 * (KT > ND ? KT : ND); ++s) {
            if (s < 16 * KT && 2 * s < Kp) acc1 = PW_MFMA(Wk[(2 * s + half) * 32 + pi], xr[s < 16 * KT ? s : 0], acc1);
            if (s < 16 * ND && 2 * s < D) accH = PW_MFMA(Wt[(2 * s + half) * 33 + pi], tr[s < 16 * ND ? s : 0], accH);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (h0 + 2 * r < H) {
                const int hh = h0 + 2 * r + half;
                float hc = relu_keep_nan(acc1[r] + bs[2 * r + half]);
                if (hh >= H) hc = 0.f;
                const float dh = hc > 0.f ? accH[r] : 0.f;
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) accX[kt] = PW_MFMA(Wj[(2 * r + half) * JS + kt * 32 + i], dh, accX[kt]);
            }
        }
    }

    if (v < nvox) {
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = kt * 32 + pw_row(r, half);
                if (k < F) dX[v * F + k] = accX[kt][r] + dOut[v * F + k];
            }
    }
}

// ---------------------------------------------------------------------------------------------------
// reverse: the weight and bias gradients
// ---------------------------------------------------------------------------------------------------
// slabs, voxels per slab (a multiple of the tile): from the voxel count alone -- never from the device
static void gemm_pw_slabs(long nvox, int& slabs, long& vps)
{
    long want = (nvox + PW_MIN_VOX - 1) / PW_MIN_VOX;
    want = want < 1 ? 1 : (want > PW_MAX_SLABS ? PW_MAX_SLABS : want);
    vps = ((nvox + want - 1) / want + 31) / 32 * 32;
    slabs = (int)((nvox + vps - 1) / vps);
}

template <int KT, int ND>
__global__ __launch_bounds__(512) void gemm_pw_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dT, const float* __restrict__ W1,
                                                            const float* __restrict__ b1, const float* __restrict__ W2, float* __restrict__ slabs,
                                                            long nvox, long vps, int F, int H, int D)
{
    constexpr int XS = 32 * KT + 1, TS = 32 * ND + 1;       // odd strides: a column of 32 voxels falls in 32 banks, a row is read along the lanes
    constexpr int OFF_T = 32 * XS, BUF = OFF_T + 32 * TS;
    extern __shared__ float lds[];                          // [2][BUF]: x tile [32][XS] | dT tile [32][TS], zero past F / D and past the slab's end

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, half = lane >> 5;
    const int h0 = (blockIdx.y * PW_NW + wave) * 32, h = h0 + i;
    const bool live = h0 < H, hok = h < H;                  // live: wave-uniform
    const long v0 = (long)blockIdx.x * vps;
    const long v1 = v0 + vps < nvox ? v0 + vps : nvox;
    const int ntile = v1 > v0 ? (int)((v1 - v0 + 31) / 32) : 0;
    const int Kp = (F + 15) / 16 * 16;
    const bool want_db2 = blockIdx.y == 0 && wave == PW_NW - 1;

    // this wave's chunk of W1 ([k][h]) and W2 ([d][h]) as B operands, column = hidden channel
    float w1r[16 * KT], w2r[16 * ND];
#pragma unroll
    for (int s = 0; s < 16 * KT; ++s) {
        const int k = 2 * s + half;
        w1r[s] = (hok && k < F) ? W1[(long)k * H + h] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < 16 * ND; ++s) {
        const int d = 2 * s + half;
        w2r[s] = (hok && d < D) ? W2[(long)h * D + d] : 0.f;
    }
    const float b1v = hok ? b1[h] : 0.f;

    float rx[2 * KT], rt[2 * ND];
    auto fetch = [&](int it) {
        const long t0 = v0 + (long)it * 32;
#pragma unroll
        for (int q = 0; q < 2 * KT; ++q) {
            const int e = tid + 512 * q, row = e / (32 * KT), col = e % (32 * KT);
            rx[q] = (t0 + row < v1 && col < F) ? x[(t0 + row) * F + col] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 2 * ND; ++q) {
            const int e = tid + 512 * q, row = e / (32 * ND), col = e % (32 * ND);
            rt[q] = (t0 + row < v1 && col < D) ? dT[(t0 + row) * D + col] : 0.f;
        }
    };
    auto stash = [&](int b) {
        float* base = lds + b * BUF;
#pragma unroll
        for (int q = 0; q < 2 * KT; ++q) {
            const int e = tid + 512 * q;
            base[(e / (32 * KT)) * XS + e % (32 * KT)] = rx[q];
        }
#pragma unroll
        for (int q = 0; q < 2 * ND; ++q) {
            const int e = tid + 512 * q;
            base[OFF_T + (e / (32 * ND)) * TS + e % (32 * ND)] = rt[q];
        }
    };

    pw_f32x16 accW1[KT], accW2[ND];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) accW1[kt] = pw_zero();
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) accW2[dt] = pw_zero();
    float db1 = 0.f, db2 = 0.f;

    if (ntile > 0) fetch(0);
    for (int it = 0; it < ntile; ++it) {
        stash(it & 1);
        __syncthreads();
        if (it + 1 < ntile) fetch(it + 1);
        const float* Xb = lds + (it & 1) * BUF;
        const float* Tb = Xb + OFF_T;
        const long t0 = v0 + (long)it * 32;

        if (want_db2 && lane < 32 * ND) {                   // column `lane` of dT's tile, rows in order
#pragma unroll 8
            for (int row = 0; row < 32; ++row) db2 += Tb[row * TS + lane];
        }
        if (!live) continue;                                // (wave-uniform; the barrier above is the iteration's only one)

        // hidden [vox][h] (the forward's chain) and dH [vox][h]: two independent chains
        pw_f32x16 acc1 = pw_zero(), accH = pw_zero();
#pragma unroll
        for (int s = 0; s < 16 * (KT > ND ? KT : ND); ++s) {
            if (s < 16 * KT && 2 * s < Kp) acc1 = PW_MFMA(Xb[i * XS + 2 * s + half], w1r[s < 16 * KT ? s : 0], acc1);
            if (s < 16 * ND && 2 * s < D) accH = PW_MFMA(Tb[i * TS + 2 * s + half], w2r[s < 16 * ND ? s : 0], accH);
        }
        // register r: voxel pw_row(r, half) of the tile.  Both as operands of products that sum over the voxels: zero past the slab's end and past H
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = pw_row(r, half);
            float hc = relu_keep_nan(acc1[r] + b1v);
            if (!hok || t0 + row >= v1) hc = 0.f;
            const float dh = hc > 0.f ? accH[r] : 0.f;
            db1 += dh;
#pragma unroll
            for (int dt = 0; dt < ND; ++dt) accW2[dt] = PW_MFMA(hc, Tb[row * TS + dt * 32 + i], accW2[dt]);          // dW2 [h][d] += hidden^T dT
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) accW1[kt] = PW_MFMA(Xb[row * XS + kt * 32 + i], dh, accW1[kt]);          // dW1 [k][h] += x^T dHg
        }
    }

    // the slab: dW1 [F][H] | dW2 [H][D] | db1 [H] | db2 [D]
    float* slab = slabs + (long)blockIdx.x * ((long)F * H + (long)H * D + H + D);
    if (live) {
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = kt * 32 + pw_row(r, half);
                if (k < F && hok) slab[(long)k * H + h] = accW1[kt][r];
            }
        float* s2 = slab + (long)F * H;
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int hr = h0 + pw_row(r, half), d = dt * 32 + i;
                if (hr < H && d < D) s2[(long)hr * D + d] = accW2[dt][r];
            }
        const float other = __shfl_xor(db1, 32, 64);        // the two lane halves hold the two halves of the tile's voxels: a fixed order
        if (half == 0 && hok) slab[(long)F * H + (long)H * D + h] = db1 + other;
    }
    if (want_db2 && lane < D) slab[(long)F * H + (long)H * D + H + lane] = db2;
}

// ---------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------
bool gemm_pw_supported(int F, int H, int D, long nvox)
{
    if (F < 1 || F > 64 || D < 1 || D > 64 || H < 1 || nvox < 1) return false;
    // voxel indices, chunk counts and grid extents are ints
    const long lim = (long)1 << 30;
    if (nvox >= lim || (long)F * H >= lim || (long)H * D >= lim) return false;
    if (((long)H + 31) / 32 / PW_NW >= 65535) return false;
    return true;
}

bool gemm_pw_plan_ints(int F, int H, int D, long nvox, bool backward, int v[8])
{
    if (!gemm_pw_supported(F, H, D, nvox)) return false;
    const int chunks = (H + 31) / 32;
    const int tile = backward ? PW_NW * 32 : PW_NW * 32 * PW_FWD_VT;
    const int tiles = (int)((nvox + tile - 1) / tile);
    int slabs = 0; long vps = 0;
    if (backward) gemm_pw_slabs(nvox, slabs, vps);
    const int groups = (chunks + PW_NW - 1) / PW_NW;
    v[0] = tile; v[1] = tiles; v[2] = 32; v[3] = chunks; v[4] = tiles + slabs * groups; v[5] = slabs; v[6] = (int)vps; v[7] = 0;
    return true;
}

size_t gemm_pw_backward_slab_floats(int F, int H, int D, long nvox)
{
    int slabs; long vps;
    gemm_pw_slabs(nvox, slabs, vps);
    return (size_t)slabs * ((size_t)F * H + (size_t)H * D + H + D);
}

#define PROBAV_PW_DISPATCH(F, D, CALL) do { \
        if ((F) <= 32) { if ((D) <= 32) { CALL(1, 1); } else { CALL(1, 2); } } \
        else { if ((D) <= 32) { CALL(2, 1); } else { CALL(2, 2); } } } while (0)

int gemm_pw_forward(const float* x, const float* W1, const float* b1, const float* W2, const float* b2, float* dec, float* hidden,
                    long nvox, int F, int H, int D, hipStream_t s)
{
    int v[8];
    if (!gemm_pw_plan_ints(F, H, D, nvox, false, v)) { set_error("gemm_pw_forward: shape not supported", hipSuccess); return PROBAV_EINVAL; }
    const dim3 grid((unsigned)v[1]), block(512);
    int rc = PROBAV_OK;
#define PROBAV_PW_FWD(KT, ND) do { \
        constexpr int ds = 32 * ND + (ND == 2 ? 32 : 0); \
        const size_t bytes = 2 * (size_t)(32 * KT * 32 + 32 * ds + 32) * sizeof(float); \
        if (hidden) rc = launch_lds<gemm_pw_fwd_kernel<KT, ND, true>>("gemm_pw_fwd", grid, block, bytes, s, x, W1, b1, W2, b2, dec, hidden, nvox, F, H, D); \
        else rc = launch_lds<gemm_pw_fwd_kernel<KT, ND, false>>("gemm_pw_fwd", grid, block, bytes, s, x, W1, b1, W2, b2, dec, hidden, nvox, F, H, D); } while (0)
    PROBAV_PW_DISPATCH(F, D, PROBAV_PW_FWD);
#undef PROBAV_PW_FWD
    return rc;
}

int gemm_pw_backward(const float* x, const float* dT, const float* dOut, const float* W1, const float* b1, const float* W2, float* dX,
                     float* dW1, float* dW2, float* db1, float* db2, float* slabs, long nvox, int F, int H, int D, hipStream_t s)
{
    int v[8];
    if (!gemm_pw_plan_ints(F, H, D, nvox, true, v)) { set_error("gemm_pw_backward: shape not supported", hipSuccess); return PROBAV_EINVAL; }
    int nslab; long vps;
    gemm_pw_slabs(nvox, nslab, vps);
    const dim3 gridd((unsigned)v[1]), gridw((unsigned)nslab, (unsigned)((v[3] + PW_NW - 1) / PW_NW)), block(512);
    int rc = PROBAV_OK;
#define PROBAV_PW_BWD(KT, ND) do { \
        const size_t bd = 2 * (size_t)(32 * KT * 32 + 32 * (32 * KT + 1) + 32 * ND * 33 + 32) * sizeof(float); \
        const size_t bw = 2 * (size_t)(32 * (32 * KT + 1) + 32 * (32 * ND + 1)) * sizeof(float); \
        rc = launch_lds<gemm_pw_bwd_data_kernel<KT, ND>>("gemm_pw_bwd_data", gridd, block, bd, s, x, dT, dOut, W1, b1, W2, dX, nvox, F, H, D); \
        if (!rc) rc = launch_lds<gemm_pw_wgrad_kernel<KT, ND>>("gemm_pw_wgrad", gridw, block, bw, s, x, dT, W1, b1, W2, slabs, nvox, vps, F, H, D); } while (0)
    PROBAV_PW_DISPATCH(F, D, PROBAV_PW_BWD);
#undef PROBAV_PW_BWD
    if (rc) return rc;
    // the four gradients are four jobs of one slab sum: fp64 across the slabs in a fixed order (kernels_small.hip)
    const long stride = (long)F * H + (long)H * D + H + D;
    const SlabSumJob jobs[4] = {{slabs, dW1, stride, F * H, nslab}, {slabs + (long)F * H, dW2, stride, H * D, nslab},
                                {slabs + (long)F * H + (long)H * D, db1, stride, H, nslab}, {slabs + (long)F * H + (long)H * D + H, db2, stride, D, nslab}};
    return slab_sum_later(s, jobs, 4);
}

}  // namespace probav
