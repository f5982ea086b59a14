// Small fused kernels around the convolution stack (gfx950):
//   weight-norm reparameterisation fwd/bwd   (tensorflow_addons WeightNormalization; models/modelsTF.py:191-197)
//   head  : mean over T + instance normalisation        (models/modelsTF.py:23-27, 199-200)
//   tail  : depth_to_space x2 + Add + denormalise       (models/modelsTF.py:38-41, 52, 71-73, 202-203)
//   reflect-pad gradient fold                           (tf.pad 'reflect', models/modelsTF.py:157-158)
//   clip + round-half-even                              (test.py:117-119, models/testClass.py:27-28)
//   Nadam, the gradient guard and the slab sums beside the main chain
// The library's error text lives here too.  The shift-compensated losses are a unit of their own: kernels_loss.hip.
#include "probav_common.h"
#include "image_math.h"
#include "reduce_device.h"
#include "../../include/probav_hip.h"
#include <cstdlib>
#include <vector>
#include <functional>
#include <stdio.h>
#include <string.h>

namespace probav {

static thread_local char g_err[512] = "";
void set_error(const char* what, hipError_t e)
{
    if (e != hipSuccess) snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    else snprintf(g_err, sizeof(g_err), "%s", what);
}
const char* last_error() { return g_err; }
int check_launch(const char* what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(what, e); return PROBAV_EHIP; }
    return PROBAV_OK;
}

// ---------------------------------------------------------------------------------------------------
// Weight normalisation.  One 64-lane wave per (layer, output channel): the ||v||^2 reduction over
// taps*Cin is a strided read folded with a wavefront shuffle reduction; the same wave then writes the
// effective kernel in both layouts the convolutions consume:
//   weff  [tap][ci][co]                      forward / backward-filter
//   weffT [taps-1-tap][co][ci]               backward-data (flipped taps, channels swapped)
// ---------------------------------------------------------------------------------------------------
// the layer whose channel range [n_off, next n_off) holds `chan` (offsets ascending).  One wave, up to 64 layers: lane i looks at layer i, a ballot
// counts the layers that start at or before the channel -- one round trip instead of a chain of up to nl dependent loads (which was most of
// these kernels' 40 us).  More layers than lanes: the chain, from layer 63 on.
__device__ __forceinline__ int find_by_offset(const WnLayer* L, int nl, int chan, bool rows)
{
    const int lane = threadIdx.x & 63;
    const int mine = lane < nl ? (rows ? L[lane].r_off : L[lane].n_off) : 0x7fffffff;
    int i = __popcll(__ballot(mine <= chan)) - 1;                    // (layer 0 starts at 0: at least one)
    if (nl > 64) while (i + 1 < nl && chan >= (rows ? L[i + 1].r_off : L[i + 1].n_off)) ++i;
    return __builtin_amdgcn_readfirstlane(i);
}
__device__ __forceinline__ int find_layer(const WnLayer* L, int nl, int chan, int& co)
{
    const int i = find_by_offset(L, nl, chan, false);
    co = chan - L[i].n_off;
    return i;
}

// Optimizer coefficients of the fused update (the rule of nadam_kernel below; Keras Nadam / Adam / SGD by coefficients)
struct OptCoef { float lr, b1, b2, eps, c_g, c_m, c_v; };
__device__ __forceinline__ float opt_update(float theta, float g, float& m, float& v, const OptCoef& c)
{
    m = c.b1 * m + (1.f - c.b1) * g;
    v = c.b2 * v + (1.f - c.b2) * g * g;
    return theta - c.lr * (c.c_g * g + c.c_m * m) / (sqrtf(v * c.c_v) + c.eps);
}

// opt_update with every rounding written out, for the GUARD kernels.  The guarded step with scale == 1, no skip and no EMA must leave the plain
// step's bits, and which of opt_update's multiply-adds the compiler fuses in the plain kernel is decided per inlined copy (the vectoriser pairs
// the products of the column loop before fusion sees them): two differently shaped kernels do not get the same choices by themselves.  These are
// the two forms wn_forward_kernel<true> is compiled to -- COLUMN = false: the gain / bias copy (m, v and the numerator each one fused
// multiply-add); COLUMN = true: the column loop (m fused, v and the numerator two rounded products and a sum).  Contraction is off in here, so
// the form does not depend on the caller.  tests/test_gpu_optim_guard.py compares the two kernels bit for bit: a compiler that chooses
// otherwise for the plain kernel shows there.
template <bool COLUMN>
__device__ __forceinline__ float opt_update_exact(float theta, float g, float& m, float& v, const OptCoef& c)
{
#pragma clang fp contract(off)
    const float gm = (1.f - c.b1) * g;
    m = __builtin_fmaf(c.b1, m, gm);
    const float gv = ((1.f - c.b2) * g) * g;
    float num;
    if constexpr (COLUMN) {
        const float bv = c.b2 * v;
        v = bv + gv;
        const float ng = c.c_g * g, nm = c.c_m * m;
        num = ng + nm;
    } else {
        v = __builtin_fmaf(c.b2, v, gv);
        const float nm = c.c_m * m;
        num = __builtin_fmaf(c.c_g, g, nm);
    }
    const float up = c.lr * num;
    const float den = sqrtf(v * c.c_v) + c.eps;
    return theta - up / den;
}

// UPDATE: the optimizer step of this column's parameters (g[co], bias[co], v[:, co]) runs first, in the same wave, and the
// reparameterisation that follows is that of the UPDATED parameters: the next forward pass finds its effective weights ready
// (reference: optimizer.apply_gradients, then WeightNormalization's kernel recomputed at the next call --
// models/trainClass.py:132, models/modelsTF.py:191-197).  The arithmetic of every element is the one of nadam_kernel.
// GUARD (include/probav_hip.h, 'optimizer options on the device'): the update reads the step's control block -- every gradient element is
// multiplied by ctl->scale before opt_update, and with ctl->skip set the whole update half is left out (params, m, v, ema untouched; the
// reparameterisation below then runs on the unchanged parameters) -- and, with an EMA buffer, follows every updated parameter with
// ema = mom * ema + (1 - mom) * theta_new.  ctl and ema are wave-uniform (scalar loads, uniform branches).  The two kernels below share this
// body: with GUARD = false the guard arguments are compile-time dead and the plain kernel is the code it always was.
template <bool UPDATE, bool GUARD>
__device__ __forceinline__ void wn_forward_body(const WnLayer* __restrict__ layers, int nl,
                                                float* __restrict__ params, float* __restrict__ weff,
                                                float* __restrict__ weffT, float* __restrict__ inv_norm,
                                                unsigned* __restrict__ amax, const float* __restrict__ grad,
                                                float* __restrict__ om, float* __restrict__ ov, const OptCoef& oc,
                                                const probav_guard_ctl* __restrict__ ctl, float* __restrict__ ema, float ema_mom)
{
    int co;
    const int li = find_layer(layers, nl, blockIdx.x, co);
    const WnLayer L = layers[li];
    float* v = params + L.v_off;
    const int lane = threadIdx.x;
    float gain = params[L.g_off + co];
    if constexpr (UPDATE && GUARD) {
        const float gs = ctl ? ctl->scale : 1.f;
        const bool skip = ctl && ctl->skip != 0u;
        if (!skip) {
            {   // as below: every lane computes the gain and the bias, lanes 0 and 1 store them (and their averages)
                const int ig = L.g_off + co, ib = L.b_off + co;
                float mg = om[ig], vg = ov[ig], mb = om[ib], vb = ov[ib];
                gain = opt_update_exact<false>(gain, grad[ig] * gs, mg, vg, oc);
                const float bnew = opt_update_exact<false>(params[ib], grad[ib] * gs, mb, vb, oc);
                if (lane == 0) { params[ig] = gain; om[ig] = mg; ov[ig] = vg; if (ema) ema[ig] = ema_mom * ema[ig] + (1.f - ema_mom) * gain; }
                if (lane == 1) { params[ib] = bnew; om[ib] = mb; ov[ib] = vb; if (ema) ema[ib] = ema_mom * ema[ib] + (1.f - ema_mom) * bnew; }
            }
            if (ema) {
                for (int k = lane; k < L.K; k += 64) {
                    const int i = L.v_off + k * L.Cout + co;
                    float mi = om[i], vi = ov[i];
                    const float e = ema[i];
                    const float t = opt_update_exact<true>(params[i], grad[i] * gs, mi, vi, oc);
                    params[i] = t; om[i] = mi; ov[i] = vi;
                    ema[i] = ema_mom * e + (1.f - ema_mom) * t;
                }
            } else {
                for (int k = lane; k < L.K; k += 64) {
                    const int i = L.v_off + k * L.Cout + co;
                    float mi = om[i], vi = ov[i];
                    params[i] = opt_update_exact<true>(params[i], grad[i] * gs, mi, vi, oc);
                    om[i] = mi; ov[i] = vi;
                }
            }
        }
    } else if constexpr (UPDATE) {
        {   // the gain g[co] and the bias[co]: every lane computes both (the values are needed below), lanes 0 and 1 store them
            const int ig = L.g_off + co, ib = L.b_off + co;
            float mg = om[ig], vg = ov[ig], mb = om[ib], vb = ov[ib];
            gain = opt_update(gain, grad[ig], mg, vg, oc);
            const float bnew = opt_update(params[ib], grad[ib], mb, vb, oc);
            if (lane == 0) { params[ig] = gain; om[ig] = mg; ov[ig] = vg; }
            if (lane == 1) { params[ib] = bnew; om[ib] = mb; ov[ib] = vb; }
        }
        for (int k = lane; k < L.K; k += 64) {                      // the filter column; each lane re-reads only what it wrote itself
            const int i = L.v_off + k * L.Cout + co;
            float mi = om[i], vi = ov[i];
            params[i] = opt_update(params[i], grad[i], mi, vi, oc);
            om[i] = mi; ov[i] = vi;
        }
    }
    // The column lives in registers between the norm and the scaled stores: all of its loads are in flight together (a loop over a runtime K
    // waited for each in turn -- 14 round trips for a 3x3x3x32 column, twice).  Columns longer than WN_Q * 64 (none in this network) take the loop.
    constexpr int WN_Q = 14;
    float ss = 0.f, wmax = 0.f;
    if (L.K <= WN_Q * 64) {
        float q[WN_Q];
#pragma unroll
        for (int j = 0; j < WN_Q; ++j) { const int k = lane + 64 * j; q[j] = k < L.K ? v[(long)k * L.Cout + co] : 0.f; }
#pragma unroll
        for (int j = 0; j < WN_Q; ++j) ss = fmaf(q[j], q[j], ss);              // (the same order as the loop: zeros beyond the column add nothing)
        ss = wave_sum(ss);
        const float inv = 1.0f / sqrtf(ss < 1e-12f ? 1e-12f : ss);   // tf.nn.l2_normalize epsilon (written so that a NaN sum stays NaN: fmaxf would clamp it)
        const float scale = gain * inv;
        if (lane == 0) inv_norm[L.n_off + co] = inv;
#pragma unroll
        for (int j = 0; j < WN_Q; ++j) {
            const int k = lane + 64 * j;
            if (k < L.K) {
                const float w = q[j] * scale;
                weff[L.w_off + (long)k * L.Cout + co] = w;
                const int tap = k / L.Cin, ci = k - tap * L.Cin;
                weffT[L.w_off + ((long)(L.taps - 1 - tap) * L.Cout + co) * L.Cin + ci] = w;
                wmax = fmaxf(wmax, fabsf(w));
            }
        }
    } else {
        for (int k = lane; k < L.K; k += 64) { const float q = v[(long)k * L.Cout + co]; ss = fmaf(q, q, ss); }
        ss = wave_sum(ss);
        const float inv = 1.0f / sqrtf(ss < 1e-12f ? 1e-12f : ss);
        const float scale = gain * inv;
        if (lane == 0) inv_norm[L.n_off + co] = inv;
        for (int k = lane; k < L.K; k += 64) {
            const float q = v[(long)k * L.Cout + co] * scale;
            weff[L.w_off + (long)k * L.Cout + co] = q;
            const int tap = k / L.Cin, ci = k - tap * L.Cin;
            weffT[L.w_off + ((long)(L.taps - 1 - tap) * L.Cout + co) * L.Cin + ci] = q;
            wmax = fmaxf(wmax, fabsf(q));
        }
    }
    if (amax) {     // largest |effective weight| and |bias| of the layer (slots li and nl + li) and of this output column: operand scales of the H3 kernels
#pragma unroll
        for (int o = 32; o; o >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, o, 64));
        // (the layer's own two slots, li and nl + li, are filled by wn_rowmax_kernel from the per-column slots and the biases: 2 x 3 920 atomicMax calls on
        // three cache lines queued for 24 us -- tools/atomic_probe.hip: 3 ns apiece, one after the other)
        if (lane == 0) amax[2 * nl + L.n_off + co] = __float_as_uint(wmax);
    }
}
template <bool UPDATE>
__global__ __launch_bounds__(64) void wn_forward_kernel(const WnLayer* __restrict__ layers, int nl,
                                                       float* __restrict__ params, float* __restrict__ weff,
                                                       float* __restrict__ weffT, float* __restrict__ inv_norm,
                                                       unsigned* __restrict__ amax, const float* __restrict__ grad,
                                                       float* __restrict__ om, float* __restrict__ ov, OptCoef oc)
{
    wn_forward_body<UPDATE, false>(layers, nl, params, weff, weffT, inv_norm, amax, grad, om, ov, oc, nullptr, nullptr, 0.f);
}
// wn_forward_kernel<true> with GUARD: the guarded fused step (probav_optimizer_step_fused_guarded)
__global__ __launch_bounds__(64) void wn_forward_guard_kernel(const WnLayer* __restrict__ layers, int nl,
                                                             float* __restrict__ params, float* __restrict__ weff,
                                                             float* __restrict__ weffT, float* __restrict__ inv_norm,
                                                             unsigned* __restrict__ amax, const float* __restrict__ grad,
                                                             float* __restrict__ om, float* __restrict__ ov, OptCoef oc,
                                                             const probav_guard_ctl* __restrict__ ctl, float* __restrict__ ema, float ema_mom)
{
    wn_forward_body<true, true>(layers, nl, params, weff, weffT, inv_norm, amax, grad, om, ov, oc, ctl, ema, ema_mom);
}

// largest |effective weight| per INPUT channel (the output columns of the backward-data matrices weffT, and the rows of W1 the fused
// pointwise backward scales its dX by): one wave per (layer, input channel), after wn_forward_kernel on the same stream
__global__ __launch_bounds__(64) void wn_rowmax_kernel(const WnLayer* __restrict__ layers, int nl, const float* __restrict__ weff,
                                                      unsigned* __restrict__ arow, unsigned* __restrict__ amax, const float* __restrict__ params)
{
    const int i = find_by_offset(layers, nl, (int)blockIdx.x, true);
    const WnLayer L = layers[i];
    const int ci = blockIdx.x - L.r_off, lane = threadIdx.x;
    float m = 0.f;
    const int ne = L.taps * L.Cout;
    for (int e0 = 0; e0 < ne; e0 += 64 * 8) {                         // eight independent loads per round trip
        float q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = e0 + 64 * j + lane;
            const int ec = e < ne ? e : 0;
            const int tap = ec / L.Cout, co = ec - tap * L.Cout;
            q[j] = weff[L.w_off + ((long)tap * L.Cin + ci) * L.Cout + co];
            q[j] = e < ne ? fabsf(q[j]) : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) m = fmaxf(m, q[j]);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) arow[blockIdx.x] = __float_as_uint(m);
    if (ci == 0) {      // the layer's first wave also fills the layer's own slots: largest |effective weight| (= the largest of its per-column slots, written by
                        // wn_forward_kernel before this launch) and largest |bias| (the parameters hold the updated biases by now)
        unsigned wm = 0u; float bm = 0.f;
        for (int c = lane; c < L.Cout; c += 64) { const unsigned q = amax[2 * nl + L.n_off + c]; wm = q > wm ? q : wm; bm = fmaxf(bm, fabsf(params[L.b_off + c])); }
#pragma unroll
        for (int o = 32; o; o >>= 1) { const unsigned q = (unsigned)__shfl_xor((int)wm, o, 64); wm = q > wm ? q : wm; bm = fmaxf(bm, __shfl_xor(bm, o, 64)); }
        if (lane == 0) { amax[i] = wm; amax[nl + i] = __float_as_uint(bm); }
    }
}

__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ xall, size_t n, unsigned* __restrict__ slots)
{
    const float* x = xall + (size_t)blockIdx.y * n;                 // sample blockIdx.y: n values (n % 4 == 0 or the base stays 16-byte aligned only for sample 0: see the scalar path)
    unsigned* slot = slots + blockIdx.y;
    float m = 0.f;
    const size_t stride = (size_t)gridDim.x * 256;
    if ((n & 3) == 0) {
        const size_t n4 = n >> 2;
        size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
        for (; i + 3 * stride < n4; i += 4 * stride) {                  // four independent loads in flight
            const float4 a = reinterpret_cast<const float4*>(x)[i], b = reinterpret_cast<const float4*>(x)[i + stride];
            const float4 c = reinterpret_cast<const float4*>(x)[i + 2 * stride], d = reinterpret_cast<const float4*>(x)[i + 3 * stride];
            m = fmaxf(m, fmaxf(fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))), fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fmaxf(fabsf(b.z), fabsf(b.w)))));
            m = fmaxf(m, fmaxf(fmaxf(fmaxf(fabsf(c.x), fabsf(c.y)), fmaxf(fabsf(c.z), fabsf(c.w))), fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fmaxf(fabsf(d.z), fabsf(d.w)))));
        }
        for (; i < n4; i += stride) {
            const float4 v = reinterpret_cast<const float4*>(x)[i];
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) m = fmaxf(m, fabsf(x[i]));
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __shared__ float wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {                                          // one atomic per workgroup, skipped when the slot already holds more
        m = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
        atomicMax(slot, __float_as_uint(m));
    }
}
int amax_tensor(const float* x, size_t per_sample, int N, unsigned* slots, hipStream_t s)
{
    if (N < 1) return PROBAV_OK;
    size_t blocks = (per_sample / 4 + 255) / 256;
    if (blocks < 1) blocks = 1;
    const size_t cap = N >= 2048 ? 1 : 2048 / (size_t)N;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(amax_kernel, dim3((unsigned)blocks, (unsigned)N), dim3(256), 0, s, x, per_sample, slots);
    return check_launch("amax");
}

// largest |w[r][c]| over the rows r of a row-major [rows][cols] matrix -> slots[c] (plain store; cols <= 256): the per-column filter
// scales of the H3 kernels for the single-operator entry points (the engine gets them from wn_forward)
__global__ __launch_bounds__(256) void amax_columns_kernel(const float* __restrict__ w, long rows, int cols, unsigned* __restrict__ slots)
{
    __shared__ float part[256];
    const int per = 256 / cols, c = threadIdx.x % cols, r0 = threadIdx.x / cols;      // `per` row streams per column
    float m = 0.f;
    if (r0 < per) for (long r = r0; r < rows; r += per) m = fmaxf(m, fabsf(w[r * cols + c]));
    part[threadIdx.x] = m;
    __syncthreads();
    if (threadIdx.x < cols) {
        for (int k = 1; k < per; ++k) m = fmaxf(m, part[k * cols + threadIdx.x]);
        slots[threadIdx.x] = __float_as_uint(m);
    }
}
int amax_columns(const float* w, long rows, int cols, unsigned* slots, hipStream_t s)
{
    if (cols < 1 || cols > 256) { set_error("amax_columns: 1 <= cols <= 256", hipSuccess); return PROBAV_EINVAL; }
    hipLaunchKernelGGL(amax_columns_kernel, dim3(1), dim3(256), 0, s, w, rows, cols, slots);
    return check_launch("amax_columns");
}

// d loss/d g = sum(dw * v) / ||v|| ;  d loss/d v = g/||v|| * (dw - v * sum(dw * v) / ||v||^2)
__global__ __launch_bounds__(64) void wn_backward_kernel(const WnLayer* __restrict__ layers, int nl,
                                                        const float* __restrict__ params, const float* __restrict__ dweff,
                                                        const float* __restrict__ inv_norm, float* __restrict__ grads)
{
    int co;
    const WnLayer L = layers[find_layer(layers, nl, blockIdx.x, co)];
    const float* v = params + L.v_off;
    const float* dw = dweff + L.w_off;
    const int lane = threadIdx.x;
    float dot = 0.f;
    for (int k = lane; k < L.K; k += 64) dot = fmaf(dw[(long)k * L.Cout + co], v[(long)k * L.Cout + co], dot);
    dot = wave_sum(dot);
    const float inv = inv_norm[L.n_off + co];
    const float gg = params[L.g_off + co];
    const bool clamped = inv >= 1e6f;                               // ||v||^2 < 1e-12: norm is the constant 1e-6
    const float proj = clamped ? 0.f : dot * inv * inv;
    if (lane == 0) grads[L.g_off + co] = dot * inv;
    for (int k = lane; k < L.K; k += 64) {
        const long i = (long)k * L.Cout + co;
        grads[L.v_off + i] = gg * inv * (dw[i] - v[i] * proj);
    }
}

int wn_forward(const WnLayer* d_layers, int nlayers, int cout_total, int cin_total, const float* params,
               float* weff, float* weffT, float* inv_norm, unsigned* amax, hipStream_t s)
{
    hipLaunchKernelGGL(wn_forward_kernel<false>, dim3(cout_total), dim3(64), 0, s, d_layers, nlayers, const_cast<float*>(params), weff, weffT, inv_norm, amax,
                       (const float*)nullptr, (float*)nullptr, (float*)nullptr, OptCoef());
    int rc = check_launch("wn_forward");
    if (rc || !amax) return rc;
    hipLaunchKernelGGL(wn_rowmax_kernel, dim3(cin_total), dim3(64), 0, s, d_layers, nlayers, weff, amax + 2 * nlayers + cout_total, amax, params);
    return check_launch("wn_rowmax");
}
int optimizer_wn_step(const WnLayer* d_layers, int nlayers, int cout_total, int cin_total, float* params, const float* grad, float* m, float* v,
                      float lr, float b1, float b2, float eps, float c_g, float c_m, float c_v,
                      float* weff, float* weffT, float* inv_norm, unsigned* amax, hipStream_t s)
{
    OptCoef oc = {lr, b1, b2, eps, c_g, c_m, c_v};
    hipLaunchKernelGGL(wn_forward_kernel<true>, dim3(cout_total), dim3(64), 0, s, d_layers, nlayers, params, weff, weffT, inv_norm, amax, grad, m, v, oc);
    int rc = check_launch("optimizer_wn_step");
    if (rc || !amax) return rc;
    hipLaunchKernelGGL(wn_rowmax_kernel, dim3(cin_total), dim3(64), 0, s, d_layers, nlayers, weff, amax + 2 * nlayers + cout_total, amax, params);
    return check_launch("wn_rowmax");
}
int optimizer_wn_step_guarded(const WnLayer* d_layers, int nlayers, int cout_total, int cin_total, float* params, const float* grad, float* m, float* v,
                              float lr, float b1, float b2, float eps, float c_g, float c_m, float c_v,
                              float* weff, float* weffT, float* inv_norm, unsigned* amax, float* ema, float ema_mom, const probav_guard_ctl* ctl, hipStream_t s)
{
    OptCoef oc = {lr, b1, b2, eps, c_g, c_m, c_v};
    hipLaunchKernelGGL(wn_forward_guard_kernel, dim3(cout_total), dim3(64), 0, s, d_layers, nlayers, params, weff, weffT, inv_norm, amax, grad, m, v, oc, ctl, ema, ema_mom);
    int rc = check_launch("optimizer_wn_step_guarded");
    if (rc || !amax) return rc;
    hipLaunchKernelGGL(wn_rowmax_kernel, dim3(cin_total), dim3(64), 0, s, d_layers, nlayers, weff, amax + 2 * nlayers + cout_total, amax, params);
    return check_launch("wn_rowmax");
}
int wn_backward(const WnLayer* d_layers, int nlayers, int cout_total, const float* params,
                const float* dweff, const float* inv_norm, float* grads, hipStream_t s)
{
    hipLaunchKernelGGL(wn_backward_kernel, dim3(cout_total), dim3(64), 0, s, d_layers, nlayers, params, dweff, inv_norm, grads);
    return check_launch("wn_backward");
}

// ---------------------------------------------------------------------------------------------------
// head: x [N,H,W,T,C] -> xn = (x - mean)/std  [N,H,W,T,C] ,  mn = (mean_T(x) - mean)/std  [N,H,W,C]     (C = 1, or 3 for isGrayScale=False)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_kernel(const float* __restrict__ x, float* __restrict__ xn,
                                                  float* __restrict__ mn, int nhw, int T, int C, float mean, float stdv, unsigned* __restrict__ zero, int nzero)
{
    const int i = blockIdx.x * 256 + threadIdx.x;          // (pixel, channel)
    for (int z = i; z < nzero; z += gridDim.x * 256) zero[z] = 0u;      // the forward pass's per-sample amax slots (a 6-us memset launch of their own before)
    if (i >= nhw * C) return;
    const int px = i / C, c = i - px * C;
    float s = 0.f;
    for (int t = 0; t < T; ++t) {
        const long o = ((long)px * T + t) * C + c;
        const float q = x[o];
        s += q;
        xn[o] = (q - mean) / stdv;
    }
    mn[i] = (s / (float)T - mean) / stdv;
}
int head_forward(const float* x, float* xn, float* mn, int nhw, int T, int C, float mean, float stdv, hipStream_t s, unsigned* zero, int nzero)
{
    hipLaunchKernelGGL(head_kernel, dim3((nhw * C + 255) / 256), dim3(256), 0, s, x, xn, mn, nhw, T, C, mean, stdv, zero, nzero);
    return check_launch("head");
}

// tail: y[n, s*h+i, s*w+j] = (up[n,h,w,i*s+j] + r3[n,h,w,i*s+j]) * std + mean
__global__ __launch_bounds__(256) void tail_fwd_kernel(const float* __restrict__ up, const float* __restrict__ r3,
                                                      float* __restrict__ y, int N, int P, int sc, float mean, float stdv)
{
    const int S = P * sc;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)N * S * S) return;
    const int X = (int)(i % S), Y = (int)((i / S) % S), n = (int)(i / ((long)S * S));
    const long src = (((long)n * P + Y / sc) * P + X / sc) * (sc * sc) + (Y % sc) * sc + (X % sc);
    y[i] = (up[src] + r3[src]) * stdv + mean;
}
__global__ __launch_bounds__(256) void tail_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dtail,
                                                      int N, int P, int sc, float stdv, unsigned* __restrict__ zero, int nzero)
{
    const int S = P * sc, C = sc * sc;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    for (long z = i; z < nzero; z += (long)gridDim.x * 256) zero[z] = 0u;      // the backward pass's per-sample amax slots
    if (i >= (long)N * P * P * C) return;
    const int c = (int)(i % C);
    long r = i / C;
    const int w = (int)(r % P); r /= P;
    const int h = (int)(r % P);
    const int n = (int)(r / P);
    dtail[i] = dy[((long)n * S + h * sc + c / sc) * S + w * sc + c % sc] * stdv;
}
int tail_forward(const float* up, const float* r3, float* y, int N, int P, int sc, float mean, float stdv, hipStream_t s)
{
    const long n = (long)N * P * sc * P * sc;
    hipLaunchKernelGGL(tail_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, up, r3, y, N, P, sc, mean, stdv);
    return check_launch("tail_fwd");
}
int tail_backward(const float* dy, float* dtail, int N, int P, int sc, float stdv, hipStream_t s, unsigned* zero, int nzero)
{
    const long n = (long)N * P * P * sc * sc;
    hipLaunchKernelGGL(tail_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dy, dtail, N, P, sc, stdv, zero, nzero);
    return check_launch("tail_bwd");
}

// Gradient of tf.pad(x, 1 on H and W, 'reflect'): padded row 0 mirrors row 1, padded row H+1 mirrors row H-2.
template <int VEC>
__global__ __launch_bounds__(256) void reflect_fold_kernel(const float* __restrict__ dpad, float* __restrict__ dx,
                                                          int N, int H, int W, int TC, unsigned* __restrict__ amax)
{
    // VEC = 4: TC % 4 == 0 and 16-byte aligned tensors; indices stay in 32 bits inside a sample (64-bit divisions cost more than the traffic)
    typedef float vec_t __attribute__((ext_vector_type(VEC)));
    const int n = blockIdx.y;                                       // one sample per grid row: its largest |dx| goes to amax[n]
    const int TCv = TC / VEC, per = H * W * TCv;
    const float* src = dpad + (long)n * (H + 2) * (W + 2) * TC;
    float* dst = dx + (long)n * H * W * TC;
    float m = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < per; i += gridDim.x * 256) {
        const int r = i / TCv, e = i - r * TCv;
        const int h = r / W, w = r - h * W;
        int hs[2], ws[2], nh = 1, nw = 1;
        hs[0] = h + 1; ws[0] = w + 1;
        if (h == 1) hs[nh++] = 0;
        if (h == H - 2) hs[nh++] = H + 1;          // H >= 4, so h == 1 and h == H-2 never coincide
        if (w == 1) ws[nw++] = 0;
        if (w == W - 2) ws[nw++] = W + 1;
        vec_t s = 0.f;
        for (int a = 0; a < nh; ++a)
            for (int b = 0; b < nw; ++b)
                s += *reinterpret_cast<const vec_t*>(src + ((long)(hs[a] * (W + 2) + ws[b]) * TCv + e) * VEC);
        *reinterpret_cast<vec_t*>(dst + (long)i * VEC) = s;
#pragma unroll
        for (int c = 0; c < VEC; ++c) m = fmaxf(m, fabsf(s[c]));
    }
    if (amax) {                                 // largest |dx| of the sample (H3 operand scale of the next layer's kernels): one guarded atomic per workgroup
#pragma unroll
        for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        __shared__ float wm[4];
        if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            m = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
            atomicMax(amax + n, __float_as_uint(m));
        }
    }
}
// nothing but a dependent chain of 32x32x16 fp16 MFMAs: what the matrix pipe of THIS device sustains (probav_mfma_probe)
typedef _Float16 probe_f16x8 __attribute__((ext_vector_type(8)));
typedef float probe_f32x16 __attribute__((ext_vector_type(16)));
__global__ __launch_bounds__(256) void mfma_probe_kernel(const probe_f16x8* __restrict__ seed, float* __restrict__ sink, int iters)
{
    probe_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const probe_f16x8 a = seed[threadIdx.x & 63], b = seed[64 + (threadIdx.x & 63)];
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
    }
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += acc[i];
    sink[blockIdx.x * 256 + threadIdx.x] = t;
}
typedef float probe_f32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void mfma_probe16_kernel(const probe_f16x8* __restrict__ seed, float* __restrict__ sink, int iters)
{
    probe_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const probe_f16x8 a = seed[threadIdx.x & 63], b = seed[64 + (threadIdx.x & 63)];
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 32; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
    }
    sink[blockIdx.x * 256 + threadIdx.x] = acc[0] + acc[1] + acc[2] + acc[3];
}
int mfma_probe(const void* seed, float* sink, int iters, int launches, hipStream_t s, int shape)
{
    for (int l = 0; l < launches; ++l) {
        if (shape == 1) hipLaunchKernelGGL(mfma_probe16_kernel, dim3(256), dim3(256), 0, s, (const probe_f16x8*)seed, sink, iters);
        else hipLaunchKernelGGL(mfma_probe_kernel, dim3(256), dim3(256), 0, s, (const probe_f16x8*)seed, sink, iters);
    }
    return check_launch("mfma_probe");
}

static thread_local ReduceSide* g_reduce_side = nullptr;
void reduce_side_activate(ReduceSide* ctx) { g_reduce_side = ctx; }
hipStream_t reduce_fork(hipStream_t s)
{
    ReduceSide* c = g_reduce_side;
    if (!c || !c->side || s == c->side) return s;
    hipEvent_t ev = c->ev[c->k++ & 7];
    if (hipEventRecord(ev, s) != hipSuccess || hipStreamWaitEvent(c->side, ev, 0) != hipSuccess) { (void)hipGetLastError(); c->last = nullptr; return s; }
    c->last = s;
    return c->side;
}
// The caller guarantees that nothing has been enqueued on s since its last reduce_fork(s): the side stream, being in order, already waits for
// that point -- no second event (an event record between two kernels of the launch stream costs it about 6 us of bubble).
hipStream_t reduce_fork_adjacent(hipStream_t s)
{
    ReduceSide* c = g_reduce_side;
    if (!c || !c->side || s == c->side) return s;
    if (c->k == 0 || c->last != s || c->defer) return reduce_fork(s);   // (deferred launches: the previous fork point is no longer adjacent)   // (nothing forked yet in this pass, or the last fork did not take: there is no earlier point)
    return c->side;
}
struct PendingList { std::vector<std::function<int(hipStream_t)>> fns; std::vector<SlabSumJob> jobs; };
int reduce_later(hipStream_t s, std::function<int(hipStream_t)> fn)
{
    ReduceSide* c = g_reduce_side;
    if (!c || !c->side || !c->defer || s == c->side) return fn(reduce_fork(s));
    if (!c->pending) c->pending = new PendingList();
    static_cast<PendingList*>(c->pending)->fns.push_back(std::move(fn));
    return PROBAV_OK;
}

// ---- batched slab sums: one launch for a list of (source slabs -> destination) jobs.  A block = 64 consecutive elements of one job x 4 interleaved slab groups (a wave's
// load is 256 consecutive bytes of one slab); a thread sums its group's slabs in two fp64 accumulators (16 independent requests in flight), the groups meet in LDS:
// ((g0 + g1) + g2) + g3.  The order is a function of (element, slabs) only: the same bits whatever else shares the launch. ----
constexpr int SLAB_SUM_MAXJ = 40;
struct SlabSumBatch { SlabSumJob job[SLAB_SUM_MAXJ]; int first[SLAB_SUM_MAXJ + 1]; int njobs; };
__global__ __launch_bounds__(256) void slab_sum_batch_kernel(SlabSumBatch b)
{
    __shared__ double red[4][64];
    int j = 0;
    while (j + 1 < b.njobs && (int)blockIdx.x >= b.first[j + 1]) ++j;
    const SlabSumJob& J = b.job[j];
    const int e = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int i = ((int)blockIdx.x - b.first[j]) * 64 + e;
    double a0 = 0.0, a1 = 0.0;
    if (i < J.count) {
        const float* p = J.src + i;
        int c = g;
#pragma unroll 8
        for (; c + 4 < J.slabs; c += 8) { a0 += (double)p[(long)c * J.stride]; a1 += (double)p[(long)(c + 4) * J.stride]; }
        if (c < J.slabs) a0 += (double)p[(long)c * J.stride];
    }
    red[g][e] = a0 + a1;
    __syncthreads();
    if (g == 0 && i < J.count) J.dst[i] = (float)(((red[0][e] + red[1][e]) + red[2][e]) + red[3][e]);
}
static int slab_sum_launch(const SlabSumJob* jobs, int njobs, hipStream_t s)
{
    for (int j0 = 0; j0 < njobs; j0 += SLAB_SUM_MAXJ) {
        SlabSumBatch b;
        b.njobs = njobs - j0 < SLAB_SUM_MAXJ ? njobs - j0 : SLAB_SUM_MAXJ;
        int blocks = 0;
        for (int j = 0; j < b.njobs; ++j) { b.job[j] = jobs[j0 + j]; b.first[j] = blocks; blocks += (jobs[j0 + j].count + 63) / 64; }
        b.first[b.njobs] = blocks;
        if (blocks == 0) continue;
        hipLaunchKernelGGL(slab_sum_batch_kernel, dim3((unsigned)blocks), dim3(256), 0, s, b);
        const int rc = check_launch("slab_sum_batch");
        if (rc) return rc;
    }
    return PROBAV_OK;
}
int slab_sum_later(hipStream_t s, const SlabSumJob* jobs, int njobs)
{
    ReduceSide* c = g_reduce_side;
    if (!c || !c->side || !c->defer || s == c->side) return slab_sum_launch(jobs, njobs, reduce_fork(s));
    if (!c->pending) c->pending = new PendingList();
    PendingList* q = static_cast<PendingList*>(c->pending);
    q->jobs.insert(q->jobs.end(), jobs, jobs + njobs);
    return PROBAV_OK;
}
int reduce_flush(hipStream_t s)
{
    ReduceSide* c = g_reduce_side;
    if (!c || !c->pending) return PROBAV_OK;
    PendingList* q = static_cast<PendingList*>(c->pending);
    if (q->fns.empty() && q->jobs.empty()) return PROBAV_OK;
    // The small launches fork to the side stream (one event for all of them).  The slab sums do NOT: a flush's worth of them is one kernel that streams 150 MB at the memory's
    // rate (40 us) and goes to the launch stream itself -- measured against the same kernel on the side stream: -0.8 % of the step (a fork is an event record between two
    // chip-filling kernels, and what the low-priority stream has not finished is waited for at the join); flushes that only carry slab sums record no event at all.
    int rc = PROBAV_OK;
    if (!q->fns.empty()) {
        hipStream_t rs = reduce_fork(s);
        for (auto& fn : q->fns) { rc = fn(rs); if (rc) break; }      // (a failed launch ends the flush: the launches behind it belong to a pass that is being abandoned)
    }
    if (!rc && !q->jobs.empty()) rc = slab_sum_launch(q->jobs.data(), (int)q->jobs.size(), s);
    q->fns.clear(); q->jobs.clear();
    return rc;
}
void reduce_free_pending(ReduceSide* ctx)
{
    if (ctx && ctx->pending) { delete static_cast<PendingList*>(ctx->pending); ctx->pending = nullptr; }
}
void reduce_drop_pending()
{
    ReduceSide* c = g_reduce_side;
    if (c && c->pending) { static_cast<PendingList*>(c->pending)->fns.clear(); static_cast<PendingList*>(c->pending)->jobs.clear(); }
}
int reduce_join(hipStream_t s)
{
    ReduceSide* c = g_reduce_side;
    { const int rc = reduce_flush(s); if (rc) return rc; }
    if (!c || !c->side || c->k == 0) return PROBAV_OK;
    if (hipEventRecord(c->joined, c->side) != hipSuccess || hipStreamWaitEvent(s, c->joined, 0) != hipSuccess) {
        set_error("reduce_join: event record / wait", hipGetLastError());
        return PROBAV_EHIP;
    }
    c->k = 0;
    c->last = nullptr;
    return PROBAV_OK;
}

// The same fold, one workgroup per output row (n, h): which padded rows fold onto it is a property of the workgroup (row h + 1, and row 0 / H + 1 behind
// rows 1 / H - 2), the row's 16-byte elements are walked in order (every request of a wave is one contiguous run), one multiply-high finds the column.
__global__ __launch_bounds__(256) void reflect_fold_rows_kernel(const float4* __restrict__ dpad, float4* __restrict__ dx, int H, int W, int TCv, unsigned mTCv,
                                                               unsigned* __restrict__ amax)
{
    const int h = blockIdx.x, n = blockIdx.y;
    const int rowv = (W + 2) * TCv;                                 // 16-byte elements of a padded row
    const float4* r0 = dpad + ((long)n * (H + 2) + h + 1) * rowv;
    const int extra = h == 1 ? -(h + 1) : (h == H - 2 ? 2 : 0);     // the second padded row that folds onto this one, relative to r0 (0: none)
    const float4* r1 = r0 + (long)extra * rowv;
    float4* dst = dx + ((long)n * H + h) * W * TCv;
    float m = 0.f;
    const int nel = W * TCv;
    for (int i0 = threadIdx.x; i0 < nel; i0 += 256 * 4) {           // four elements per thread and round: their requests go out together
        float4 a[4], b[4];
        int c1[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + 256 * k < nel ? i0 + 256 * k : i0;
            const int w = (int)__umulhi((unsigned)i, mTCv), e = i - w * TCv;
            const int c0 = (w + 1) * TCv + e;
            c1[k] = w == 1 ? e : (w == W - 2 ? (W + 1) * TCv + e : -1);          // the second padded column
            a[k] = r0[c0];
            b[k] = r1[c0];                                                          // (extra == 0: the same element again, unused)
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + 256 * k;
            if (i >= nel) break;
            float4 v = a[k];
            if (extra) { v.x += b[k].x; v.y += b[k].y; v.z += b[k].z; v.w += b[k].w; }
            if (c1[k] >= 0) {
                float4 q = r0[c1[k]];
                if (extra) { const float4 c = r1[c1[k]]; q.x += c.x; q.y += c.y; q.z += c.z; q.w += c.w; }
                v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
            }
            dst[i] = v;
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        }
    }
    if (amax) {
#pragma unroll
        for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        __shared__ float wm[4];
        if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            m = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
            atomicMax(amax + n, __float_as_uint(m));                   // (no guarding read of the slot: x6_device.h, amax_commit)
        }
    }
}

int reflect_fold(const float* dpad, float* dx, int N, int H, int W, int TC, unsigned* amax, hipStream_t s)
{
    if (H < 4 || W < 4) { set_error("reflect_fold: H, W must be >= 4", hipSuccess); return PROBAV_EINVAL; }
    if (TC % 4 == 0 && ((reinterpret_cast<uintptr_t>(dpad) | reinterpret_cast<uintptr_t>(dx)) & 15) == 0 && H <= 65535 && N <= 65535) {
        const int TCv = TC / 4;
        const unsigned mTCv = (unsigned)((0x100000000ull + (unsigned)TCv - 1) / (unsigned)TCv);     // floor(i / TCv) = umulhi(i, m) for i < 2^16 * ... (i < W * TCv here)
        if ((long)W * TCv < (1l << 20) && TCv >= 2 && TCv < 4096) {
            hipLaunchKernelGGL(reflect_fold_rows_kernel, dim3((unsigned)H, (unsigned)N), dim3(256), 0, s, reinterpret_cast<const float4*>(dpad),
                               reinterpret_cast<float4*>(dx), H, W, TCv, mTCv, amax);
            return check_launch("reflect_fold");
        }
    }
    const long per = (long)H * W * TC;
    long blocks = (per + 255) / 256;
    const long cap = N >= 4096 ? 1 : 4096 / N;
    if (blocks > cap) blocks = cap;
    const bool v4 = TC % 4 == 0 && ((reinterpret_cast<uintptr_t>(dpad) | reinterpret_cast<uintptr_t>(dx)) & 15) == 0;
    if (v4) {
        blocks = (per / 4 + 255) / 256;
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(reflect_fold_kernel<4>, dim3((unsigned)blocks, (unsigned)N), dim3(256), 0, s, dpad, dx, N, H, W, TC, amax);
    } else
        hipLaunchKernelGGL(reflect_fold_kernel<1>, dim3((unsigned)blocks, (unsigned)N), dim3(256), 0, s, dpad, dx, N, H, W, TC, amax);
    return check_launch("reflect_fold");
}

// General fold: dx[i] = sum of dpad over every padded index that mirrors onto i, per dimension (pads 0..2; needs extent > 2 * pad).
__device__ __forceinline__ int fold_srcs(int i, int n, int p, int (&u)[3])
{
    int c = 0;
    u[c++] = i + p;
    for (int j = 1; j <= p; ++j) {
        if (i == j) u[c++] = p - j;                    // padded index p - j mirrors onto j
        if (i == n - 1 - j) u[c++] = n - 1 + p + j;    // padded index n - 1 + p + j mirrors onto n - 1 - j
    }
    return c;
}
__global__ __launch_bounds__(256) void reflect_fold3_kernel(const float* __restrict__ dpad, float* __restrict__ dx, int N, int H, int W,
                                                           int T, int C, int ph, int pw, int pt)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)N * H * W * T * C) return;
    long r = i;
    const int c = (int)(r % C); r /= C;
    const int t = (int)(r % T); r /= T;
    const int w = (int)(r % W); r /= W;
    const int h = (int)(r % H);
    const int n = (int)(r / H);
    int hs[3], ws[3], ts[3];
    const int nh = fold_srcs(h, H, ph, hs), nw = fold_srcs(w, W, pw, ws), nt = fold_srcs(t, T, pt, ts);
    const int Hp = H + 2 * ph, Wp = W + 2 * pw, Tp = T + 2 * pt;
    float s = 0.f;
    for (int a = 0; a < nh; ++a)
        for (int b = 0; b < nw; ++b)
            for (int d = 0; d < nt; ++d)
                s += dpad[((((long)n * Hp + hs[a]) * Wp + ws[b]) * Tp + ts[d]) * C + c];
    dx[i] = s;
}
int reflect_fold3(const float* dpad, float* dx, int N, int H, int W, int T, int C, int ph, int pw, int pt, hipStream_t s)
{
    if (ph < 0 || pw < 0 || pt < 0 || ph > 2 || pw > 2 || pt > 2 || H <= 2 * ph || W <= 2 * pw || T <= 2 * pt) {
        set_error("reflect_fold3: pads must be 0..2 and smaller than half the extent", hipSuccess); return PROBAV_EINVAL;
    }
    const long n = (long)N * H * W * T * C;
    hipLaunchKernelGGL(reflect_fold3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dpad, dx, N, H, W, T, C, ph, pw, pt);
    return check_launch("reflect_fold3");
}

// tf.clip_by_value(x, lo, hi) then tf.round (half to even == rintf in the default rounding mode)
__global__ __launch_bounds__(256) void clip_round_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n, float lo, float hi)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = clip_rint(in[i], lo, hi);
}
int clip_round(const float* in, float* out, size_t n, float lo, float hi, hipStream_t s)
{
    hipLaunchKernelGGL(clip_round_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n, lo, hi);
    return check_launch("clip_round");
}

// ---------------------------------------------------------------------------------------------------
// Keras Nadam (optimizer_v2; train.py:79-81) on the flat parameter buffer, one launch:
//   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2
//   theta -= lr * ( (1-mu_t) g / (1-Pi_t) + mu_{t+1} m / (1-Pi_t mu_{t+1}) ) / ( sqrt(v / (1-b2^t)) + eps )
// The step-dependent scalars (c_g = (1-mu_t)/(1-Pi_t), c_m = mu_{t+1}/(1-Pi_t mu_{t+1}), c_v = 1/(1-b2^t)) are computed by the
// host in double and passed by value.
// ---------------------------------------------------------------------------------------------------
// GUARD: as in wn_forward_body -- g' = g * ctl->scale, nothing written when ctl->skip is set, the EMA after the update.  One body for both
// kernels: with GUARD = false it is the plain kernel's arithmetic, text and order unchanged (the rule of opt_update).
template <bool GUARD>
__device__ __forceinline__ void nadam_body(float* __restrict__ theta, const float* __restrict__ grad, float* __restrict__ m,
                                           float* __restrict__ v, long n, float lr, float b1, float b2, float eps,
                                           float c_g, float c_m, float c_v, const probav_guard_ctl* __restrict__ ctl,
                                           float* __restrict__ ema, float ema_mom)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if constexpr (GUARD) {
        float g = grad[i];
        if (ctl) {
            if (ctl->skip != 0u) return;
            g *= ctl->scale;
        }
        float t;
        {   // the plain kernel below is compiled to products and sums, none fused: written out with contraction off, so that scale == 1 leaves its bits
            // (see opt_update_exact)
#pragma clang fp contract(off)
            const float bm = b1 * m[i], gm = (1.f - b1) * g;
            const float mi = bm + gm;
            const float bv = b2 * v[i], gv = ((1.f - b2) * g) * g;
            const float vi = bv + gv;
            m[i] = mi; v[i] = vi;
            const float ng = c_g * g, nm = c_m * mi;
            const float up = lr * (ng + nm);
            const float den = sqrtf(vi * c_v) + eps;
            t = theta[i] - up / den;
        }
        theta[i] = t;
        if (ema) ema[i] = ema_mom * ema[i] + (1.f - ema_mom) * t;
    } else {
        const float g = grad[i];
        const float mi = b1 * m[i] + (1.f - b1) * g;
        const float vi = b2 * v[i] + (1.f - b2) * g * g;
        m[i] = mi; v[i] = vi;
        theta[i] -= lr * (c_g * g + c_m * mi) / (sqrtf(vi * c_v) + eps);
    }
}
__global__ __launch_bounds__(256) void nadam_kernel(float* __restrict__ theta, const float* __restrict__ grad, float* __restrict__ m,
                                                   float* __restrict__ v, long n, float lr, float b1, float b2, float eps,
                                                   float c_g, float c_m, float c_v)
{
    nadam_body<false>(theta, grad, m, v, n, lr, b1, b2, eps, c_g, c_m, c_v, nullptr, nullptr, 0.f);
}
__global__ __launch_bounds__(256) void nadam_guard_kernel(float* __restrict__ theta, const float* __restrict__ grad, float* __restrict__ m,
                                                         float* __restrict__ v, long n, float lr, float b1, float b2, float eps,
                                                         float c_g, float c_m, float c_v, const probav_guard_ctl* __restrict__ ctl,
                                                         float* __restrict__ ema, float ema_mom)
{
    nadam_body<true>(theta, grad, m, v, n, lr, b1, b2, eps, c_g, c_m, c_v, ctl, ema, ema_mom);
}
int nadam_step(float* theta, const float* grad, float* m, float* v, long n, float lr, float b1, float b2, float eps,
               float c_g, float c_m, float c_v, hipStream_t s)
{
    if (n <= 0) return PROBAV_OK;
    hipLaunchKernelGGL(nadam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, theta, grad, m, v, n, lr, b1, b2, eps, c_g, c_m, c_v);
    return check_launch("nadam");
}
int nadam_step_guarded(float* theta, const float* grad, float* m, float* v, float* ema, long n, float lr, float b1, float b2, float eps,
                       float c_g, float c_m, float c_v, float ema_mom, const probav_guard_ctl* ctl, hipStream_t s)
{
    if (n <= 0) return PROBAV_OK;
    hipLaunchKernelGGL(nadam_guard_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, theta, grad, m, v, n, lr, b1, b2, eps, c_g, c_m, c_v, ctl, ema, ema_mom);
    return check_launch("nadam_guarded");
}

// ---------------------------------------------------------------------------------------------------
// The gradient's global norm and the step's control block (include/probav_hip.h, 'optimizer options on the device'; Keras global_clipnorm =
// tf.clip_by_global_norm).  grad_sumsq_kernel: GUARD_BLOCKS workgroups of 256 threads whatever the device; thread t of the grid accumulates
// (double)g * g over i = t, t + GUARD_BLOCKS * 256, ... in that order; a butterfly over the wave (every lane ends with the same bits), the four
// waves' sums added in wave order, one fp64 partial per workgroup.  No floating-point atomics: the same gradient gives the same partials on
// every run and on every device.  guard_finish_kernel: one wave adds the partials in index order and derives the block.  It is a launch of its
// own, not a prologue of every consumer wave: the 3 920 waves of the fused step would each repeat an fp64 square root and a division and one
// of them would still have to publish the block for the host's log; as a launch the consumers read two words.
// The squares of finite fp32 values are below 2^256 and at most 2^31 of them are added: the fp64 total is non-finite exactly when an element is.
// ---------------------------------------------------------------------------------------------------
constexpr int GUARD_BLOCKS = 128;
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ grad, long n, double* __restrict__ partial)
{
    const long stride = (long)GUARD_BLOCKS * 256;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    double acc = 0.0;
    for (; i + 3 * stride < n; i += 4 * stride) {                       // four independent loads in flight, added in index order
        const float a = grad[i], b = grad[i + stride], c = grad[i + 2 * stride], d = grad[i + 3 * stride];
        acc += (double)a * a; acc += (double)b * b; acc += (double)c * c; acc += (double)d * d;
    }
    for (; i < n; i += stride) { const float a = grad[i]; acc += (double)a * a; }
    acc = wave_sum(acc);
    __shared__ double ws[4];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}
__global__ __launch_bounds__(64) void guard_finish_kernel(const double* __restrict__ partial, float clipnorm, int skip_nonfinite,
                                                         probav_guard_ctl* __restrict__ ctl)
{
    __shared__ double p[GUARD_BLOCKS];
    for (int k = threadIdx.x; k < GUARD_BLOCKS; k += 64) p[k] = partial[k];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int k = 0; k < GUARD_BLOCKS; ++k) total += p[k];
    const bool finite = total == total && total <= 1.7976931348623157e308;
    const double norm = sqrt(total);
    float scale = 1.f;
    if (clipnorm > 0.f) {
        const double c = (double)clipnorm;
        scale = finite ? (float)(c / (norm > c ? norm : c)) : __builtin_nanf("");
    }
    const unsigned skip = (skip_nonfinite && !finite) ? 1u : 0u;
    ctl->scale = scale;
    ctl->skip = skip;
    ctl->skipped_total = ctl->skipped_total + skip;
    ctl->norm = (float)norm;
}
size_t grad_guard_scratch_bytes() { return (size_t)GUARD_BLOCKS * sizeof(double); }
int grad_guard(const float* grad, long n, float clipnorm, int skip_nonfinite, double* partial, probav_guard_ctl* ctl, hipStream_t s)
{
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(GUARD_BLOCKS), dim3(256), 0, s, grad, n, partial);
    int rc = check_launch("grad_sumsq");
    if (rc) return rc;
    hipLaunchKernelGGL(guard_finish_kernel, dim3(1), dim3(64), 0, s, partial, clipnorm, skip_nonfinite, ctl);
    return check_launch("guard_finish");
}

}  // namespace probav
