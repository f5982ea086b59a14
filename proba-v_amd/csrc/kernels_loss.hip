// The shift-compensated losses of a cfg (gfx950), forward and backward:
//   L1 / L2 / cPSNR      shiftCompensatedL1Loss / L2Loss / cPSNR      (models/loss.py:37-84, 140-187, 226-238)
//   sobel_l1_mix         shiftCompensatedL1EdgeLoss                   (models/loss.py:86-97, 126-137, 214-219)
//   l1msssim             shiftCompensatedRevSSIM                      (models/loss.py:99-124, 189-212)
// All three compare the crop of the prediction with the crop of HR under every shift (i, j) of the (2*border+1)^2 registrations:
//   n = sum M ; b = sum(H - P*M)/n ; C = (P + b)*M ; e = H - C
// (HR is NOT masked -- reference quirk, models/loss.py:146,151)  Sums run in fp64.  What they share is stated once, below.
#include "probav_common.h"
#include "reduce_device.h"

namespace probav {

// C = (P + b) M, the bias-corrected masked prediction, and the residual e = H - C (m = 1.0 on a clear pixel, else 0.0)
__device__ __forceinline__ double corrected(double p, double bias, double m) { return (p + bias) * m; }
__device__ __forceinline__ double residual(double h, double p, double bias, double m) { return h - corrected(p, bias, m); }

// The L x L crop of one sample under the shift (i, j): pixel (r, c) reads HR and the mask at (i + r, j + c), the prediction at (border + r, border + c).
struct Crop {
    const float* H; const uint8_t* M; const float* P;
    int S, border, L, i, j;
    __device__ __forceinline__ bool clear(int r, int c) const { return M[(i + r) * S + j + c] != 0; }
    __device__ __forceinline__ float hr(int r, int c) const { return H[(i + r) * S + j + c]; }
    __device__ __forceinline__ float pred(int r, int c) const { return P[(border + r) * S + border + c]; }
    __device__ __forceinline__ double m(int r, int c) const { return clear(r, c) ? 1.0 : 0.0; }
    __device__ __forceinline__ double residual(int r, int c, double bias) const { return probav::residual((double)hr(r, c), (double)pred(r, c), bias, m(r, c)); }
};
__device__ __forceinline__ Crop crop_at(const float* hr, const uint8_t* mask, const float* pred, int b, int S, int border, int i, int j)
{
    const long o = (long)b * S * S;
    return Crop{hr + o, mask + o, pred + o, S, border, S - 2 * border, i, j};
}
__device__ __forceinline__ Crop crop_of_shift(const float* hr, const uint8_t* mask, const float* pred, int b, int S, int border, int sft)
{
    const int ns = 2 * border + 1, i = sft / ns;
    return crop_at(hr, mask, pred, b, S, border, i, sft - i * ns);
}

// This thread's share of n and of sum(H - P*M): the crop at 256-thread stride.  The caller reduces the two over the workgroup.
__device__ __forceinline__ void crop_walk(const Crop& x, int tid, double& cnt, double& dsum)
{
    cnt = 0.0; dsum = 0.0;
    for (int k = tid; k < x.L * x.L; k += 256) {
        const int r = k / x.L, c = k - r * x.L;
        const float m = x.clear(r, c) ? 1.f : 0.f;
        cnt += (double)m;
        dsum += (double)(x.hr(r, c) - x.pred(r, c) * m);
    }
}
// ... reduced with block_sum: n in every thread, the bias returned
__device__ __forceinline__ double crop_bias(const Crop& x, int tid, double* red, double& cnt)
{
    double dsum;
    crop_walk(x, tid, cnt, dsum);
    cnt = block_sum(cnt, red, tid);
    dsum = block_sum(dsum, red, tid);
    return dsum / cnt;
}

// The minimum over the shifts, taken in ascending shift order with a strict <: the first minimum wins ties.  A shift under which a sample has
// no clear pixel has n = 0 and a NaN candidate: `v < best` is false for it, so it is no candidate (as in probav_score_select).  With no
// candidate at all best stays 1e300 and value() is NaN (arg 0), not the sentinel -- (float)1e300 is +inf and 10 log10(max^2 / 1e300) a
// finite -2 900 dB that a validation mean would swallow.
struct FirstMin {
    double best = 1e300;
    int arg = 0;
    __device__ __forceinline__ void take(double v, int sft) { if (v < best) { best = v; arg = sft; } }
    __device__ __forceinline__ double value() const { return best < 1e300 ? best : __builtin_nan(""); }
};

// ---------------------------------------------------------------------------------------------------
// L1 / L2 / cPSNR:  l1 = sum|e|/n ; l2 = sum e^2/n.  The path is ~1.7 MFLOP per sample, the reference
// needs ~600 tiny TF ops for it, here it is two launches.
// ---------------------------------------------------------------------------------------------------
// One workgroup per (sample, shift row i): its four waves take the shifts (i, j), j = wave, wave + 4, and evaluate them with wavefront
// shuffle reductions only (no block barrier per shift).  Candidates go to a scratch table [B][shifts][2] (fp64); shift_select_kernel picks
// the per-sample minima, batch_mean_kernel the batch means.  (One workgroup per sample looping over all 49 shifts left half of the CUs idle:
// 131 us at batch 128.)
__global__ __launch_bounds__(256) void shift_loss_fwd_kernel(
    const float* __restrict__ hr, const uint8_t* __restrict__ mask, const float* __restrict__ pred, int S, int border,
    double* __restrict__ cand)
{
    const int b = blockIdx.x, i = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int L = S - 2 * border, ns = 2 * border + 1, nshift = ns * ns;
    for (int j = wave; j < ns; j += 4) {
        const int sft = i * ns + j;
        const Crop x = crop_at(hr, mask, pred, b, S, border, i, j);
        // This kernel keeps a loop of its own (not crop_walk: a wave, not the workgroup, owns the shift).  Both passes walk the crop four
        // pixels per lane and round, requested together (one pixel per round was one memory round trip per pixel: 112 of them in a row per
        // wave); the sums take the pixels in the same order as one per round would, so the bits are the same.
        constexpr int U = 4;
        const int n = L * L;
        double cnt = 0.0, dsum = 0.0;
        for (int k0 = lane; k0 < n; k0 += 64 * U) {
            float m[U], h[U], q[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + 64 * u < n ? k0 + 64 * u : k0;
                const int r = k / L, c = k - r * L;
                m[u] = x.clear(r, c) ? 1.f : 0.f;
                h[u] = x.hr(r, c);
                q[u] = x.pred(r, c);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (k0 + 64 * u < n) { cnt += (double)m[u]; dsum += (double)(h[u] - q[u] * m[u]); }
        }
        cnt = wave_sum(cnt); dsum = wave_sum(dsum);
        const double bias = dsum / cnt;
        double s1 = 0.0, s2 = 0.0;
        for (int k0 = lane; k0 < n; k0 += 64 * U) {
            float h[U], q[U]; bool mk[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + 64 * u < n ? k0 + 64 * u : k0;
                const int r = k / L, c = k - r * L;
                mk[u] = x.clear(r, c);
                h[u] = x.hr(r, c);
                q[u] = x.pred(r, c);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (k0 + 64 * u < n) {
                    const double e = residual((double)h[u], (double)q[u], bias, mk[u] ? 1.0 : 0.0);
                    s1 += fabs(e);
                    s2 += e * e;
                }
        }
        s1 = wave_sum(s1) / cnt; s2 = wave_sum(s2) / cnt;
        if (lane == 0) { cand[((long)b * nshift + sft) * 2] = s1; cand[((long)b * nshift + sft) * 2 + 1] = s2; }
    }
}

__global__ __launch_bounds__(64) void batch_mean_kernel(const float* __restrict__ a, const float* __restrict__ b2,
                                                       float* __restrict__ ma, float* __restrict__ mb, int n)
{
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) { s1 += (double)a[i]; s2 += (double)b2[i]; }
    s1 = wave_sum(s1); s2 = wave_sum(s2);
    if (threadIdx.x == 0) { *ma = (float)(s1 / n); *mb = (float)(s2 / n); }
}

// per-sample minima over the shifts (FirstMin); one thread per sample.  -> the sample's l1 and l2 as written
__device__ __forceinline__ void shift_select_sample(const double* __restrict__ cand, int b, int nshift, float max_val, float* __restrict__ l1_out,
                                                    float* __restrict__ l2_out, float* __restrict__ cpsnr_out, int* __restrict__ arg_l1,
                                                    int* __restrict__ arg_l2, float& l1, float& l2)
{
    const double2* c = reinterpret_cast<const double2*>(cand) + (long)b * nshift;
    FirstMin m1, m2;
#pragma unroll 7
    for (int sft = 0; sft < nshift; ++sft) {
        const double2 v = c[sft];
        m1.take(v.x, sft);
        m2.take(v.y, sft);
    }
    l1_out[b] = l1 = (float)m1.value();
    l2_out[b] = l2 = (float)m2.value();
    cpsnr_out[b] = (float)(10.0 * log10((double)max_val * (double)max_val / m2.value()));
    arg_l1[b] = m1.arg;
    arg_l2[b] = m2.arg;
}
// One workgroup of up to 1024 threads: the batch means (batch_mean_kernel's sums, in its order: a wave's lanes take the samples 64 apart, then the butterfly)
// are taken in the same launch -- a 6-us launch less between the forward and the backward pass.
__global__ __launch_bounds__(1024) void shift_select_mean_kernel(const double* __restrict__ cand, int B, int nshift, float max_val,
                                                                float* __restrict__ l1_out, float* __restrict__ l2_out, float* __restrict__ cpsnr_out,
                                                                int* __restrict__ arg_l1, int* __restrict__ arg_l2, float* __restrict__ ma, float* __restrict__ mb)
{
    __shared__ float sl1[1024], sl2[1024];
    const int b = threadIdx.x;
    if (b < B) shift_select_sample(cand, b, nshift, max_val, l1_out, l2_out, cpsnr_out, arg_l1, arg_l2, sl1[b], sl2[b]);
    __syncthreads();
    if (threadIdx.x < 64) {
        double s1 = 0.0, s2 = 0.0;
        for (int i = threadIdx.x; i < B; i += 64) { s1 += (double)sl1[i]; s2 += (double)sl2[i]; }
        s1 = wave_sum(s1); s2 = wave_sum(s2);
        if (threadIdx.x == 0) { *ma = (float)(s1 / B); *mb = (float)(s2 / B); }
    }
}

__global__ __launch_bounds__(64) void shift_select_kernel(const double* __restrict__ cand, int B, int nshift, float max_val,
                                                         float* __restrict__ l1_out, float* __restrict__ l2_out, float* __restrict__ cpsnr_out,
                                                         int* __restrict__ arg_l1, int* __restrict__ arg_l2)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    float l1, l2;
    if (b < B) shift_select_sample(cand, b, nshift, max_val, l1_out, l2_out, cpsnr_out, arg_l1, arg_l2, l1, l2);
}

int shift_loss_forward(const float* hr, const uint8_t* mask, const float* pred, int B, int S, int border,
                       float* l1, float* l2, float* cpsnr, int* arg_l1, int* arg_l2, float* mean_l1, float* mean_l2,
                       float max_val, hipStream_t s)
{
    if (B <= 0 || border < 0 || S <= 2 * border) { set_error("shift_loss_forward: bad shape (size must exceed 2 * border)", hipSuccess); return PROBAV_EINVAL; }
    const int ns = 2 * border + 1;
    // candidate table owned by the library, grown on demand (never inside a captured region: the first call of a shape allocates)
    static double* cand = nullptr;
    static size_t cand_n = 0;
    const size_t need = (size_t)B * ns * ns * 2;
    if (need > cand_n) {
        if (cand) (void)hipFree(cand);
        cand = nullptr; cand_n = 0;
        hipError_t err = hipMalloc((void**)&cand, need * sizeof(double));
        if (err != hipSuccess) { set_error("shift_loss_forward: scratch allocation", err); return PROBAV_EHIP; }
        cand_n = need;
    }
    hipLaunchKernelGGL(shift_loss_fwd_kernel, dim3(B, ns), dim3(256), 0, s, hr, mask, pred, S, border, cand);
    if (B <= 1024) {
        hipLaunchKernelGGL(shift_select_mean_kernel, dim3(1), dim3((unsigned)((B + 63) / 64 * 64)), 0, s, cand, B, ns * ns, max_val, l1, l2, cpsnr, arg_l1, arg_l2, mean_l1, mean_l2);
        return check_launch("shift_loss_forward");
    }
    hipLaunchKernelGGL(shift_select_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, cand, B, ns * ns, max_val, l1, l2, cpsnr, arg_l1, arg_l2);
    hipLaunchKernelGGL(batch_mean_kernel, dim3(1), dim3(64), 0, s, l1, l2, mean_l1, mean_l2, B);
    return check_launch("shift_loss_forward");
}

// Gradient of mean_B min_shift loss w.r.t. pred for the arg-min shift:
//   L1: dP_k = -(M_k/n) (s_k - sum(s M)/n),  s = sign(H - C)      L2: s = 2 (H - C)
__global__ __launch_bounds__(256) void shift_loss_bwd_kernel(
    const float* __restrict__ hr, const uint8_t* __restrict__ mask, const float* __restrict__ pred,
    const int* __restrict__ arg, int S, int border, int which, const float* __restrict__ upstream, float inv_b,
    float* __restrict__ dpred)
{
    const float scale = (upstream ? upstream[0] : 1.f) * inv_b;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Crop x = crop_of_shift(hr, mask, pred, b, S, border, arg[b]);
    const int L = x.L;
    float* G = dpred + (long)b * S * S;
    __shared__ double red[2][4];
    double cnt, dsum;
    crop_walk(x, tid, cnt, dsum);
    cnt = wave_sum(cnt); dsum = wave_sum(dsum);
    if (lane == 0) { red[0][wave] = cnt; red[1][wave] = dsum; }
    __syncthreads();
    cnt = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    dsum = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    const double bias = dsum / cnt;
    __syncthreads();
    double ssum = 0.0;
    for (int k = tid; k < L * L; k += 256) {
        const int r = k / L, c = k - r * L;
        const double e = x.residual(r, c, bias);
        const double sg = which == 1 ? sign_keep_nan(e) : 2.0 * e;
        ssum += sg * x.m(r, c);
    }
    ssum = wave_sum(ssum);
    if (lane == 0) red[0][wave] = ssum;
    __syncthreads();
    ssum = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    for (int k = tid; k < S * S; k += 256) {
        const int Y = k / S, X = k - Y * S, r = Y - border, c = X - border;
        float gk = 0.f;
        if (r >= 0 && r < L && c >= 0 && c < L) {
            const double e = x.residual(r, c, bias);
            const double sg = which == 1 ? sign_keep_nan(e) : 2.0 * e;
            gk = (float)(-(x.m(r, c) / cnt) * (sg - ssum / cnt) * (double)scale);
        }
        G[k] = gk;
    }
}
int shift_loss_backward(const float* hr, const uint8_t* mask, const float* pred, const int* arg, int B, int S,
                        int border, int which, const float* upstream, float* dpred, hipStream_t s)
{
    if (which != 1 && which != 2) { set_error("shift_loss_backward: which must be 1 (L1) or 2 (L2)", hipSuccess); return PROBAV_EINVAL; }
    if (B <= 0 || border < 0 || S <= 2 * border) { set_error("shift_loss_backward: bad shape (size must exceed 2 * border)", hipSuccess); return PROBAV_EINVAL; }
    hipLaunchKernelGGL(shift_loss_bwd_kernel, dim3(B), dim3(256), 0, s, hr, mask, pred, arg, S, border, which, upstream, 1.0f / (float)B, dpred);
    return check_launch("shift_loss_backward");
}

// ---------------------------------------------------------------------------------------------------
// cfg loss = sobel_l1_mix: shiftCompensatedL1EdgeLoss.  Per sample and candidate shift
//   l1 = sum |e| / n,
//   sob = sum (|Gy| + |Gx|) / n,  (Gy, Gx) = tf.image.sobel_edges(H) - sobel_edges(C) = sobel_edges(e): 3x3 cross-correlations
//         [[-1,-2,-1],[0,0,0],[1,2,1]] and its transpose on the REFLECT-padded crop,
//   loss = pi * l1 + (1 - pi) * sob;  minimum over the shifts, mean over the batch.
// One 256-thread block per sample walks the shifts; e lives in LDS (the Sobel taps read it with mirrored indices).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// (Gy, Gx) at pixel k of the crop held in sD [L][L]
__device__ __forceinline__ void sobel_at(const float* sD, int k, int L, double& gy, double& gx)
{
    const int r = k / L, c = k - r * L;
    const int r0 = mirror(r - 1, L) * L, r1 = r * L, r2 = mirror(r + 1, L) * L;
    const int c0 = mirror(c - 1, L), c2 = mirror(c + 1, L);
    gy = ((double)sD[r2 + c0] + 2.0 * sD[r2 + c] + sD[r2 + c2]) - ((double)sD[r0 + c0] + 2.0 * sD[r0 + c] + sD[r0 + c2]);
    gx = ((double)sD[r0 + c2] + 2.0 * sD[r1 + c2] + sD[r2 + c2]) - ((double)sD[r0 + c0] + 2.0 * sD[r1 + c0] + sD[r2 + c0]);
}

__global__ __launch_bounds__(256) void shift_l1edge_fwd_kernel(
    const float* __restrict__ hr, const uint8_t* __restrict__ mask, const float* __restrict__ pred, int S, int border, float pi,
    float* __restrict__ loss_out, int* __restrict__ arg_out)
{
    extern __shared__ float sD[];                                   // [L][L]
    __shared__ double red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int L = S - 2 * border, ns = 2 * border + 1, nshift = ns * ns;
    FirstMin best;
    for (int sft = 0; sft < nshift; ++sft) {
        const Crop x = crop_of_shift(hr, mask, pred, b, S, border, sft);
        double cnt;
        const double bias = crop_bias(x, tid, red, cnt);
        double s1 = 0.0;
        for (int k = tid; k < L * L; k += 256) {
            const int r = k / L, c = k - r * L;
            const double e = x.residual(r, c, bias);
            sD[k] = (float)e;
            s1 += fabs(e);
        }
        s1 = block_sum(s1, red, tid);                               // (its barriers also publish sD)
        double sg = 0.0;
        for (int k = tid; k < L * L; k += 256) {
            double gy, gx;
            sobel_at(sD, k, L, gy, gx);
            sg += fabs(gy) + fabs(gx);
        }
        sg = block_sum(sg, red, tid);
        best.take(((double)pi * s1 + (1.0 - (double)pi) * sg) / cnt, sft);
    }
    if (tid == 0) { loss_out[b] = (float)best.value(); arg_out[b] = best.arg; }
}

// gradient of mean_B min_shift (pi l1 + (1-pi) sob) w.r.t. pred at the arg-min shift:
//   G = dloss/de = [pi sign(e) + (1-pi) Sobel^T(sign(Gy), sign(Gx))] / n      (Sobel^T folds the mirrored pad back onto the crop)
//   dP_k = -M_k (G_k - sum(G M) / n)                                          (the second term is the brightness bias)
__global__ __launch_bounds__(256) void shift_l1edge_bwd_kernel(
    const float* __restrict__ hr, const uint8_t* __restrict__ mask, const float* __restrict__ pred, const int* __restrict__ arg,
    int S, int border, float pi, const float* __restrict__ upstream, float inv_b, float* __restrict__ dpred)
{
    extern __shared__ float sm[];
    __shared__ double red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int L = S - 2 * border, Lp = L + 2;
    float* sD = sm;                     // [L][L]
    float* sY = sD + L * L;             // sign(Gy) [L][L]
    float* sX = sY + L * L;             // sign(Gx)
    float* sG = sX + L * L;             // gradient w.r.t. the padded crop [Lp][Lp], then folded
    const float scale = (upstream ? upstream[0] : 1.f) * inv_b;
    const Crop x = crop_of_shift(hr, mask, pred, b, S, border, arg[b]);
    float* G = dpred + (long)b * S * S;
    double cnt;
    const double bias = crop_bias(x, tid, red, cnt);
    for (int k = tid; k < L * L; k += 256) {
        const int r = k / L, c = k - r * L;
        sD[k] = (float)x.residual(r, c, bias);
    }
    __syncthreads();
    for (int k = tid; k < L * L; k += 256) {
        double gy, gx;
        sobel_at(sD, k, L, gy, gx);
        sY[k] = (float)sign_keep_nan(gy);
        sX[k] = (float)sign_keep_nan(gx);
    }
    __syncthreads();
    // adjoint of the two correlations on the PADDED crop: position (u, v) in [-1, L] x [-1, L] collects the outputs q it feeds
    for (int k = tid; k < Lp * Lp; k += 256) {
        const int u = k / Lp - 1, v = k - (k / Lp) * Lp - 1;
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int bb = 0; bb < 3; ++bb) {
                const int qr = u - (a - 1), qc = v - (bb - 1);      // output whose tap (a, bb) reads (u, v)
                if (qr < 0 || qr >= L || qc < 0 || qc >= L) continue;
                const float ky = (a == 0 ? -1.f : (a == 2 ? 1.f : 0.f)) * (bb == 1 ? 2.f : 1.f);
                const float kx = (bb == 0 ? -1.f : (bb == 2 ? 1.f : 0.f)) * (a == 1 ? 2.f : 1.f);
                acc += ky * sY[qr * L + qc] + kx * sX[qr * L + qc];
            }
        sG[k] = acc;
    }
    __syncthreads();
    // fold the mirrored pad back (pad row -1 mirrors row 1, row L mirrors row L-2; same for columns) and mix with the L1 term
    double gm = 0.0;
    for (int k = tid; k < L * L; k += 256) {
        const int r = k / L, c = k - r * L;
        float acc = 0.f;
        const int us[3] = {r, r == 1 ? -1 : -2, r == L - 2 ? L : -2};       // padded rows that mirror onto r (-2 = none)
        const int vs[3] = {c, c == 1 ? -1 : -2, c == L - 2 ? L : -2};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int bb = 0; bb < 3; ++bb)
                if (us[a] != -2 && vs[bb] != -2) acc += sG[(us[a] + 1) * Lp + vs[bb] + 1];
        const float d = sD[k];
        const float g = pi * (float)sign_keep_nan((double)d) + (1.f - pi) * acc;
        sY[k] = g;                                                   // sY is dead: reuse for G * n
        gm += (double)g * x.m(r, c);
    }
    gm = block_sum(gm, red, tid);
    for (int k = tid; k < S * S; k += 256) {
        const int Y = k / S, X = k - Y * S, r = Y - border, c = X - border;
        float gk = 0.f;
        if (r >= 0 && r < L && c >= 0 && c < L)
            gk = (float)(-(x.m(r, c) / cnt) * ((double)sY[r * L + c] - gm / cnt) * (double)scale);
        G[k] = gk;
    }
}

// Both kernels keep the crop in dynamic LDS.  The forward holds e [L][L] fp32 (at most 40 000 bytes, within the default limit); the backward holds
// e, sign(Gy), sign(Gx) [L][L] and the padded gradient [L+2][L+2], fp32, and launch_lds raises its limit.  The device has 160 KiB of
// LDS for static + dynamic together and the backward also has static LDS (the reduction slots), so the largest accepted crop is the one
// whose 161 616 bytes leave room for them: crop <= 100.  The forward checks the same bound, so that a training step never finds the
// limit after its forward has run.
constexpr int L1EDGE_MAX_CROP = 100;          // (3 L^2 + (L + 2)^2) * 4 + the static slots <= 160 KiB
static size_t l1edge_bwd_lds(int L) { return ((size_t)3 * L * L + (size_t)(L + 2) * (L + 2)) * sizeof(float); }
static_assert(((size_t)3 * L1EDGE_MAX_CROP * L1EDGE_MAX_CROP + (size_t)(L1EDGE_MAX_CROP + 2) * (L1EDGE_MAX_CROP + 2)) * sizeof(float) + 64 <= LDS_LIMIT, "edge-loss crop bound");
static_assert(((size_t)3 * (L1EDGE_MAX_CROP + 1) * (L1EDGE_MAX_CROP + 1) + (size_t)(L1EDGE_MAX_CROP + 3) * (L1EDGE_MAX_CROP + 3)) * sizeof(float) > LDS_LIMIT, "edge-loss crop bound is the largest");
static int l1edge_check(const char* who, int B, int S, int border)
{
    const int L = S - 2 * border;
    if (B <= 0 || border < 0 || L < 3) {
        char msg[160]; snprintf(msg, sizeof(msg), "%s: bad shape (crop = size - 2 * border must be at least 3)", who);
        set_error(msg, hipSuccess); return PROBAV_EINVAL;
    }
    if (L > L1EDGE_MAX_CROP) {
        char msg[200]; snprintf(msg, sizeof(msg), "%s: crop %d exceeds the limit of %d pixels (size - 2 * border <= %d: the crop is held in LDS)", who, L, L1EDGE_MAX_CROP, L1EDGE_MAX_CROP);
        set_error(msg, hipSuccess); return PROBAV_EINVAL;
    }
    return PROBAV_OK;
}
int shift_l1edge_forward(const float* hr, const uint8_t* mask, const float* pred, int B, int S, int border, float pi,
                         float* loss, int* arg, float* mean, float* scratch_mean2, hipStream_t s)
{
    { const int rc = l1edge_check("shift_l1edge_forward", B, S, border); if (rc) return rc; }
    const int L = S - 2 * border;
    hipLaunchKernelGGL(shift_l1edge_fwd_kernel, dim3(B), dim3(256), (size_t)L * L * sizeof(float), s, hr, mask, pred, S, border, pi, loss, arg);
    hipLaunchKernelGGL(batch_mean_kernel, dim3(1), dim3(64), 0, s, loss, loss, mean, scratch_mean2, B);
    return check_launch("shift_l1edge_forward");
}
int shift_l1edge_backward(const float* hr, const uint8_t* mask, const float* pred, const int* arg, int B, int S, int border, float pi,
                          const float* upstream, float* dpred, hipStream_t s)
{
    { const int rc = l1edge_check("shift_l1edge_backward", B, S, border); if (rc) return rc; }
    const int L = S - 2 * border;
    return launch_lds<shift_l1edge_bwd_kernel>("shift_l1edge_backward", dim3(B), dim3(256), l1edge_bwd_lds(L), s, hr, mask, pred, arg, S, border, pi, upstream, 1.0f / (float)B, dpred);
}

// ---------------------------------------------------------------------------------------------------
// cfg loss = l1msssim: shiftCompensatedRevSSIM, restated with the reference's quirks:
//   weights of scale s: w1d = exp(-x / (2 sigma_s^2)), x = linspace(-L/2, L/2, L)  (NOT squared), w = outer(w1d, w1d) * M, normalised
//   per sample;  mu, variance "sigma" and cov are w-weighted moments of H and C;  luminance / contrast / structure use
//   C1, C1, C3;  pcs = prod_s contrast_s structure_s;  ssim term = 1 - sum_{s,b} luminance_{s,b} pcs_b / B;
//   mixed with the w-weighted L1: loss = eta * ssim + (1 - eta) * sum_{s,b,px} w |H - C| / (B * numBytes).
// The loss is ONE scalar per shift for the whole batch, and the minimum over the shifts is taken of that scalar (the batch shares
// the shift).  Kernel 1 (grid B x shifts) leaves 7 weighted sums per (shift, sample, scale); kernel 2 combines them and picks the
// arg-min shift; the backward kernel differentiates that shift.
// ---------------------------------------------------------------------------------------------------
#define RS_NS 5
#define RS_NM 7          // Sw, SwH, SwC, SwHH, SwCC, SwHC, Sw|H-C|

__device__ __forceinline__ double rs_w1d(int k, int L, int s)
{
    const double sig[RS_NS] = {0.5, 1.0, 2.0, 4.0, 8.0};
    const double x = -0.5 * L + (double)k * (double)L / (double)(L - 1);      // tf.linspace(-L/2, L/2, L)
    return exp(-x / (2.0 * sig[s] * sig[s]));
}

__global__ __launch_bounds__(256) void revssim_moments_kernel(
    const float* __restrict__ hr, const uint8_t* __restrict__ mask, const float* __restrict__ pred, int S, int border,
    double* __restrict__ mom /* [shift][B][5][7] */, int B)
{
    extern __shared__ double sW[];                                  // [5][L]
    __shared__ double red[4];
    const int b = blockIdx.x, sft = blockIdx.y, tid = threadIdx.x;
    const int L = S - 2 * border;
    for (int k = tid; k < RS_NS * L; k += 256) sW[k] = rs_w1d(k % L, L, k / L);
    const Crop x = crop_of_shift(hr, mask, pred, b, S, border, sft);
    double cnt;
    const double bias = crop_bias(x, tid, red, cnt);
    double acc[RS_NS][RS_NM];
#pragma unroll
    for (int s = 0; s < RS_NS; ++s)
#pragma unroll
        for (int q = 0; q < RS_NM; ++q) acc[s][q] = 0.0;
    for (int k = tid; k < L * L; k += 256) {
        const int r = k / L, c = k - r * L;
        const double m = x.m(r, c), h = (double)x.hr(r, c), cc = corrected((double)x.pred(r, c), bias, m);
#pragma unroll
        for (int s = 0; s < RS_NS; ++s) {
            const double w = sW[s * L + r] * sW[s * L + c] * m;
            acc[s][0] += w; acc[s][1] += w * h; acc[s][2] += w * cc; acc[s][3] += w * h * h; acc[s][4] += w * cc * cc;
            acc[s][5] += w * h * cc; acc[s][6] += w * fabs(h - cc);
        }
    }
    double* out = mom + ((long)sft * B + b) * RS_NS * RS_NM;
#pragma unroll
    for (int s = 0; s < RS_NS; ++s)
#pragma unroll
        for (int q = 0; q < RS_NM; ++q) {
            const double v = block_sum(acc[s][q], red, tid);
            if (tid == 0) out[s * RS_NM + q] = v;
        }
}

struct RsTerms { double lum[RS_NS], con[RS_NS], str[RS_NS], muH[RS_NS], muS[RS_NS], sH[RS_NS], sS[RS_NS], cov[RS_NS], l1[RS_NS]; };

__device__ __forceinline__ void rs_terms(const double* m, double C1, double C3, RsTerms& t)
{
#pragma unroll
    for (int s = 0; s < RS_NS; ++s) {
        const double* q = m + s * RS_NM;
        const double iw = 1.0 / q[0];
        t.muH[s] = q[1] * iw; t.muS[s] = q[2] * iw;
        t.sH[s] = q[3] * iw - t.muH[s] * t.muH[s];
        t.sS[s] = q[4] * iw - t.muS[s] * t.muS[s];
        t.cov[s] = q[5] * iw - t.muS[s] * t.muH[s];
        t.l1[s] = q[6] * iw;
        t.lum[s] = (2.0 * t.muH[s] * t.muS[s] + C1) / (t.muH[s] * t.muH[s] + t.muS[s] * t.muS[s] + C1);
        t.con[s] = (2.0 * t.sH[s] * t.sS[s] + C1) / (t.sH[s] * t.sH[s] + t.sS[s] * t.sS[s] + C1);
        t.str[s] = (2.0 * t.cov[s] + C3) / (t.sH[s] * t.sS[s] + C3);
    }
}

__global__ __launch_bounds__(64) void revssim_select_kernel(const double* __restrict__ mom, int B, int nshift, float max_val, float eta,
                                                            float* __restrict__ loss_out, int* __restrict__ arg_out)
{
    const double C1 = (0.01 * max_val) * (0.01 * max_val), C3 = 0.5 * (0.03 * max_val) * (0.03 * max_val);
    __shared__ double sl[64];
    __shared__ int sa[64];
    const int lane = threadIdx.x;
    FirstMin mine;
    for (int sft = lane; sft < nshift; sft += 64) {                   // one lane per shift: a fixed-order sum over the batch
        double ssim = 0.0, l1 = 0.0;
        for (int b = 0; b < B; ++b) {
            RsTerms t;
            rs_terms(mom + ((long)sft * B + b) * RS_NS * RS_NM, C1, C3, t);
            double pcs = 1.0, lsum = 0.0;
#pragma unroll
            for (int s = 0; s < RS_NS; ++s) { pcs *= t.con[s] * t.str[s]; lsum += t.lum[s]; l1 += t.l1[s]; }
            ssim += lsum * pcs;
        }
        mine.take((double)eta * (1.0 - ssim / B) + (1.0 - (double)eta) * (l1 / B) / (double)max_val, sft);
    }
    sl[lane] = mine.best;
    sa[lane] = mine.arg;
    __syncthreads();
    if (lane == 0) {
        for (int k = 1; k < 64; ++k)                                 // the lanes' minima: at equal value the earlier shift
            if (sl[k] < mine.best || (sl[k] == mine.best && sa[k] < mine.arg)) { mine.best = sl[k]; mine.arg = sa[k]; }
        loss_out[0] = (float)mine.value();                           // NaN: every shift leaves some sample without a clear pixel
        arg_out[0] = mine.arg;
    }
}

__global__ __launch_bounds__(256) void revssim_bwd_kernel(
    const float* __restrict__ hr, const uint8_t* __restrict__ mask, const float* __restrict__ pred, const int* __restrict__ arg,
    const double* __restrict__ mom, int S, int border, int B, float max_val, float eta, const float* __restrict__ upstream,
    float* __restrict__ dpred)
{
    extern __shared__ double sm2[];
    double* sW = sm2;                                                // [5][L]
    double* sG = sW + RS_NS * (S - 2 * border);                      // [L][L] dLoss/dC
    __shared__ double red[4];
    __shared__ double cA[RS_NS], cB[RS_NS], cC[RS_NS], cMuS[RS_NS], cMuH[RS_NS], cIw[RS_NS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int L = S - 2 * border, sft = arg[0];
    const double C1 = (0.01 * max_val) * (0.01 * max_val), C3 = 0.5 * (0.03 * max_val) * (0.03 * max_val);
    const double up = upstream ? (double)upstream[0] : 1.0;
    for (int k = tid; k < RS_NS * L; k += 256) sW[k] = rs_w1d(k % L, L, k / L);
    if (tid == 0) {
        RsTerms t;
        const double* m = mom + ((long)sft * B + b) * RS_NS * RS_NM;
        rs_terms(m, C1, C3, t);
        double lsum = 0.0;
#pragma unroll
        for (int s = 0; s < RS_NS; ++s) lsum += t.lum[s];
#pragma unroll
        for (int s = 0; s < RS_NS; ++s) {
            double pex = 1.0;                                        // product of contrast * structure over the OTHER scales
#pragma unroll
            for (int q = 0; q < RS_NS; ++q) if (q != s) pex *= t.con[q] * t.str[q];
            const double pcs = pex * t.con[s] * t.str[s];
            const double dl = t.muH[s] * t.muH[s] + t.muS[s] * t.muS[s] + C1;
            const double dlum = (2.0 * t.muH[s] * dl - (2.0 * t.muH[s] * t.muS[s] + C1) * 2.0 * t.muS[s]) / (dl * dl);   // d lum / d muS
            const double dc = t.sH[s] * t.sH[s] + t.sS[s] * t.sS[s] + C1;
            const double dcon = (2.0 * t.sH[s] * dc - (2.0 * t.sH[s] * t.sS[s] + C1) * 2.0 * t.sS[s]) / (dc * dc);       // d con / d sS
            const double ds = t.sH[s] * t.sS[s] + C3;
            const double dstr_cov = 2.0 / ds, dstr_sS = -(2.0 * t.cov[s] + C3) * t.sH[s] / (ds * ds);
            const double dT_con = lsum * pex * t.str[s], dT_str = lsum * pex * t.con[s];
            cA[s] = pcs * dlum;                                      // dT / d muS
            cB[s] = dT_con * dcon + dT_str * dstr_sS;                // dT / d sS
            cC[s] = dT_str * dstr_cov;                               // dT / d cov
            cMuS[s] = t.muS[s]; cMuH[s] = t.muH[s]; cIw[s] = 1.0 / m[s * RS_NM];
        }
    }
    const Crop x = crop_of_shift(hr, mask, pred, b, S, border, sft);
    float* G = dpred + (long)b * S * S;
    double cnt;
    const double bias = crop_bias(x, tid, red, cnt);                 // (barriers inside also publish sW and the c* scalars)
    double gm = 0.0;
    for (int k = tid; k < L * L; k += 256) {
        const int r = k / L, c = k - r * L;
        const double m = x.m(r, c), h = (double)x.hr(r, c), cc = corrected((double)x.pred(r, c), bias, m);
        const double sg = h - cc > 0.0 ? 1.0 : (h - cc < 0.0 ? -1.0 : 0.0);   // this loss's own sign: 0 for NaN ('Non-finite values')
        double g = 0.0;
#pragma unroll
        for (int s = 0; s < RS_NS; ++s) {
            const double w = sW[s * L + r] * sW[s * L + c] * m * cIw[s];        // normalised weight
            g += -((double)eta / B) * w * (cA[s] + 2.0 * cB[s] * (cc - cMuS[s]) + cC[s] * (h - cMuH[s]))
                 - ((1.0 - (double)eta) / ((double)max_val * B)) * w * sg;
        }
        sG[k] = g;
        gm += g * m;
    }
    gm = block_sum(gm, red, tid);
    for (int k = tid; k < S * S; k += 256) {
        const int Y = k / S, X = k - Y * S, r = Y - border, c = X - border;
        float gk = 0.f;
        if (r >= 0 && r < L && c >= 0 && c < L) gk = (float)(x.m(r, c) * (sG[r * L + c] - gm / cnt) * up);
        G[k] = gk;
    }
}

size_t revssim_scratch_bytes(int B, int border) { const int ns = 2 * border + 1; return (size_t)ns * ns * B * RS_NS * RS_NM * sizeof(double); }

// The backward keeps the five windows [5][L] and dLoss/dC [L][L] in dynamic LDS as fp64 (launch_lds raises its limit): the
// largest accepted crop needs 162 400 bytes and the static reduction slots share the device's 160 KiB, which bounds the crop at 140.  The
// forward checks the same bound (see the edge loss above).
constexpr int REVSSIM_MAX_CROP = 140;        // (5 L + L^2) * 8 + the static slots <= 160 KiB
static size_t revssim_bwd_lds(int L) { return ((size_t)RS_NS * L + (size_t)L * L) * sizeof(double); }
static_assert(((size_t)RS_NS * REVSSIM_MAX_CROP + (size_t)REVSSIM_MAX_CROP * REVSSIM_MAX_CROP) * sizeof(double) + 512 <= LDS_LIMIT, "l1msssim crop bound");
static_assert(((size_t)RS_NS * (REVSSIM_MAX_CROP + 1) + (size_t)(REVSSIM_MAX_CROP + 1) * (REVSSIM_MAX_CROP + 1)) * sizeof(double) > LDS_LIMIT, "l1msssim crop bound is the largest");
static int revssim_check(const char* who, int B, int S, int border)
{
    const int L = S - 2 * border;
    if (B <= 0 || border < 0 || L < 2) {
        char msg[160]; snprintf(msg, sizeof(msg), "%s: bad shape (crop = size - 2 * border must be at least 2)", who);
        set_error(msg, hipSuccess); return PROBAV_EINVAL;
    }
    if (L > REVSSIM_MAX_CROP) {
        char msg[200]; snprintf(msg, sizeof(msg), "%s: crop %d exceeds the limit of %d pixels (size - 2 * border <= %d: the crop's gradient is held in LDS)", who, L, REVSSIM_MAX_CROP, REVSSIM_MAX_CROP);
        set_error(msg, hipSuccess); return PROBAV_EINVAL;
    }
    return PROBAV_OK;
}
int revssim_forward(const float* hr, const uint8_t* mask, const float* pred, int B, int S, int border, float max_val, float eta,
                    double* scratch, float* loss, int* arg, hipStream_t s)
{
    { const int rc = revssim_check("revssim_forward", B, S, border); if (rc) return rc; }
    const int L = S - 2 * border, ns = 2 * border + 1;
    hipLaunchKernelGGL(revssim_moments_kernel, dim3(B, ns * ns), dim3(256), (size_t)RS_NS * L * sizeof(double), s, hr, mask, pred, S, border, scratch, B);
    hipLaunchKernelGGL(revssim_select_kernel, dim3(1), dim3(64), 0, s, scratch, B, ns * ns, max_val, eta, loss, arg);
    return check_launch("revssim_forward");
}
int revssim_backward(const float* hr, const uint8_t* mask, const float* pred, const int* arg, const double* scratch, int B, int S,
                     int border, float max_val, float eta, const float* upstream, float* dpred, hipStream_t s)
{
    { const int rc = revssim_check("revssim_backward", B, S, border); if (rc) return rc; }
    const int L = S - 2 * border;
    return launch_lds<revssim_bwd_kernel>("revssim_backward", dim3(B), dim3(256), revssim_bwd_lds(L), s, hr, mask, pred, arg, scratch, S, border, B, max_val, eta, upstream, dpred);
}

}  // namespace probav
