// Scoring kernels (gfx950): the shift-compensated SSIM (cSSIM) of whole images, the second number of every published PROBA-V table
// beside the cPSNR of kernels_score.hip.  evaluate.py --metrics cpsnr,cssim and proba-v_amd/scoring.py drive them.
//
// The metric.  Per image: SR and HR uint16 S x S, M the clear mask of HR (nonzero = clear), border b, L = S - 2b,
// P = SR[b:b+L, b:b+L].  For every shift (u, v) in [0, 2b]^2, row-major, all in fp64:
//     H = HR[u:u+L, v:v+L]     m = M[u:u+L, v:v+L] as 0/1     n = sum m     s1 = sum m (H - P)     bias = s1 / n
//     x = m (P + bias)     y = m H                                  (masked pixels are zero on BOTH sides)
//     F(a)[i, j] = sum_{p, q} g[p] g[q] a[i+p, j+q], g the normalised 11-tap Gaussian of sigma 1.5 (data: gauss11), K = L - 10 outputs a side
//     mx = F(x)  my = F(y)  vx = F(x x) - mx^2  vy = F(y y) - my^2  cxy = F(x y) - mx my     C1 = (0.01 * 65535)^2  C2 = (0.03 * 65535)^2
//     ssim(u, v) = mean over the K^2 windows of ((2 mx my + C1)(2 cxy + C2)) / ((mx^2 + my^2 + C1)(vx + vy + C2))
//     cSSIM = max over the shifts with n > 0, shift = the first (u, v) attaining it; n = 0: the shift's value is NaN.
// A window that sees only masked pixels contributes exactly 1 (every moment is 0: C1 C2 / (C1 C2)).
//
// The folded form.  m is 0/1, so x = m P + bias m and the five filtered quantities follow from six maps of integers:
//     mx = F(mP) + bias F(m)     F(xx) = F(mP^2) + bias (2 F(mP) + bias F(m))     F(xy) = F(mPH) + bias F(mH)     my = F(mH)   F(yy) = F(mH^2)
// The products m P, m H, m P^2, m H^2, m P H are integers below 2^32: exact in fp64, whatever the order they are formed in.
//
// Shape.  ssim_partial_kernel: one workgroup per (image, band of 64 output rows, tile of 64 output columns, shift row u), 2b + 1 waves,
// wave v owns shift (u, v), lane j owns output column j of the tile.  The band's 74 HR rows (at row offset u) are staged in LDS as words
// hr | (mask != 0) << 16, 80 columns wide (64 + 10 taps + 2b), and its 74 rows of P as uint16; positions outside the image are zero and
// belong to no live output.  A lane walks down the rows: the row pass of the six maps at its column from LDS (taps in index order, one
// FMA each), the result into an 11-deep window of registers (the row loop is unrolled by 11, so the window is renamed, never moved),
// the column pass over the window (taps in index order), the SSIM term, added into the lane's sum in row order.  The lane sums are
// added across the wave by a fixed butterfly and the wave writes ONE partial into its own slot of the scratch array: no floating-point
// atomics.  ssim_table_kernel: one thread per (image, shift) adds the slots in index order and divides by K^2 (NaN where n = 0).
// ssim_select_kernel: one thread per image, first maximum over the non-NaN entries.
//
// Exactness.  A table entry is a pure function of the image's cropped inputs of that shift: the staging, the tap order, the row order,
// the butterfly and the slot order are fixed by (S, b) alone, never by the batch size, the image's position or the run; two shifts with
// equal crops execute the same instruction sequence on the same values and give the same bits.  Against the numpy statement
// (scoring.cssim_table_numpy) only the contraction of a*b+c into FMAs differs: ~1e-16 relative on a moment, below 1e-12 on an entry.
//
// Cost model (S = 384, b = 3): 49 shifts x 368^2 windows per image.  Per window-shift a lane issues 11 taps x (3 conversions, 5 products,
// 6 FMAs) for the row pass, 66 FMAs for the column pass and ~35 operations for the SSIM term (one fp64 division): 316 VALU instructions
// and 10 LDS reads per row of the unrolled loop in the gfx950 code, against the 66 FMAs of a minimal separable scheme that would share the
// row pass between neighbouring lanes and the three HR-only maps between shifts.  The row pass is also repeated for the 10 halo rows of
// each band (74 / 64).  244 VGPRs (the 6 x 11 fp64 window is 132 of them): two waves per SIMD, one 7-wave workgroup per CU.
// Measured on one MI355X (tools/ssim_bench.py, profiles/ssim_bench.txt): 53.9 ms for 580 images (92.9 us per image), 52.5 times the
// cPSNR kernels on the same images (1.03 ms), 57 % of the 316-instruction model at the published fp64 vector rate (78.6 TFLOP/s = 39.3e12
// instructions/s); 306 times faster than the same table composed from fp64 torch ops on the device (16.5 s) and ~3 100 times faster than
// the numpy statement (0.29 s per image).  Sharing the HR-only maps through LDS would remove about a third of the instructions; not done.
#include "probav_common.h"
#include "../../include/probav_hip.h"

namespace probav {

namespace {

constexpr int SSIM_MAX_S = 2048, SSIM_TAPS = 11, SSIM_HALO = SSIM_TAPS - 1;
constexpr int SSIM_TW = 64, SSIM_RB = 64;                                // output columns / rows per workgroup
constexpr int SSIM_ROWS = SSIM_RB + SSIM_HALO;                           // staged rows: 74
constexpr int SSIM_WPITCH = SSIM_TW + SSIM_HALO + 6;                     // staged HR columns: 64 lanes + 10 taps + 2b <= 80
constexpr int SSIM_PPITCH = SSIM_TW + SSIM_HALO + 2;                     // staged P columns: 74, padded to 76
constexpr int SSIM_MAPS = 6;                                             // m, mP, mH, mPP, mHH, mPH

inline int ssim_bands(int S, int border) { return (S - 2 * border - SSIM_HALO + SSIM_RB - 1) / SSIM_RB; }
inline int ssim_ctiles(int S, int border) { return (S - 2 * border - SSIM_HALO + SSIM_TW - 1) / SSIM_TW; }

template <int BD>
__global__ __launch_bounds__(64 * (2 * BD + 1)) void ssim_partial_kernel(const uint16_t* __restrict__ sr, const uint16_t* __restrict__ hr,
                                                                          const uint8_t* __restrict__ mask, const int64_t* __restrict__ moments,
                                                                          const double* __restrict__ gauss, int S, int ctiles,
                                                                          double* __restrict__ partial)
{
    constexpr int NS = 2 * BD + 1;
    __shared__ uint32_t w[SSIM_ROWS * SSIM_WPITCH];
    __shared__ uint16_t p[SSIM_ROWS * SSIM_PPITCH];
    const int L = S - 2 * BD, K = L - SSIM_HALO;
    const int band = blockIdx.x / ctiles, ct = blockIdx.x - band * ctiles;
    const int i0 = band * SSIM_RB, j0 = ct * SSIM_TW, u = blockIdx.z;
    const int rows = min(SSIM_RB, K - i0), rin = rows + SSIM_HALO;       // rin <= 74; HR rows i0 + u .. i0 + u + rin - 1 <= S - 1
    const int64_t img = blockIdx.y;
    const size_t base = (size_t)img * S * S;
    for (int k = threadIdx.x; k < rin * SSIM_WPITCH; k += blockDim.x) {
        const int rr = k / SSIM_WPITCH, c = j0 + (k - rr * SSIM_WPITCH);
        uint32_t x = 0;
        if (c < S) {
            const size_t idx = base + (size_t)(i0 + u + rr) * S + c;
            x = (uint32_t)hr[idx] | ((uint32_t)(mask[idx] != 0) << 16);
        }
        w[k] = x;
    }
    for (int k = threadIdx.x; k < rin * SSIM_PPITCH; k += blockDim.x) {
        const int rr = k / SSIM_PPITCH, c = j0 + (k - rr * SSIM_PPITCH);
        p[k] = c < L ? sr[base + (size_t)(BD + i0 + rr) * S + BD + c] : (uint16_t)0;
    }
    __syncthreads();

    const int v = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int shift = u * NS + v;
    const int64_t* mom = moments + ((size_t)img * NS * NS + shift) * 3;
    double* slot = partial + ((size_t)img * NS * NS + shift) * ((size_t)gridDim.x) + blockIdx.x;
    const int64_t n = mom[0];
    if (n <= 0) {                                                        // the shift is skipped (ssim_table_kernel writes its NaN)
        if (lane == 0) *slot = 0.0;
        return;
    }
    const double bias = (double)mom[1] / (double)n;
    const double C1 = (0.01 * 65535.0) * (0.01 * 65535.0), C2 = (0.03 * 65535.0) * (0.03 * 65535.0);
    double g[SSIM_TAPS];
#pragma unroll
    for (int k = 0; k < SSIM_TAPS; ++k) g[k] = gauss[k];
    double win[SSIM_MAPS][SSIM_TAPS];                                    // window slot t holds the row pass of row rr with rr % 11 == t
    double acc = 0.0;
    const bool live = j0 + lane < K;
    for (int r0 = 0; r0 < rin; r0 += SSIM_TAPS) {
#pragma unroll
        for (int t = 0; t < SSIM_TAPS; ++t) {
            const int rr = r0 + t;
            if (rr < rin) {
                const uint32_t* wr = w + rr * SSIM_WPITCH + lane + v;    // lane + v + q <= 63 + 6 + 10 < 80
                const uint16_t* pr = p + rr * SSIM_PPITCH + lane;        // lane + q <= 73 < 76
                double h[SSIM_MAPS];
#pragma unroll
                for (int k = 0; k < SSIM_MAPS; ++k) h[k] = 0.0;
#pragma unroll
                for (int q = 0; q < SSIM_TAPS; ++q) {
                    const uint32_t x = wr[q];
                    const double md = (double)(x >> 16), Hd = (double)(x & 0xffffu), Pd = (double)pr[q];
                    const double mP = md * Pd, mH = md * Hd;
                    h[0] = __builtin_fma(g[q], md, h[0]);
                    h[1] = __builtin_fma(g[q], mP, h[1]);
                    h[2] = __builtin_fma(g[q], mH, h[2]);
                    h[3] = __builtin_fma(g[q], mP * Pd, h[3]);
                    h[4] = __builtin_fma(g[q], mH * Hd, h[4]);
                    h[5] = __builtin_fma(g[q], mP * Hd, h[5]);
                }
#pragma unroll
                for (int k = 0; k < SSIM_MAPS; ++k) win[k][t] = h[k];
                if (rr >= SSIM_HALO) {                                   // output row rr - 10: rows rr - 10 + q sit in slot (t + 1 + q) % 11
                    double f[SSIM_MAPS];
#pragma unroll
                    for (int k = 0; k < SSIM_MAPS; ++k) {
                        double o = 0.0;
#pragma unroll
                        for (int q = 0; q < SSIM_TAPS; ++q) o = __builtin_fma(g[q], win[k][(t + 1 + q) % SSIM_TAPS], o);
                        f[k] = o;
                    }
                    const double mx = f[1] + bias * f[0], my = f[2];
                    const double fxx = f[3] + bias * (2.0 * f[1] + bias * f[0]);
                    const double fxy = f[5] + bias * f[2];
                    const double vx = fxx - mx * mx, vy = f[4] - my * my, cxy = fxy - mx * my;
                    const double term = ((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2));
                    acc += live ? term : 0.0;
                }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) *slot = acc;
}

// one thread per (image, shift): the slots in index order, divided by K^2; NaN where the shift has no clear pixel
__global__ __launch_bounds__(64) void ssim_table_kernel(const double* __restrict__ partial, const int64_t* __restrict__ moments, int64_t total,
                                                        int slots, double k2, double* __restrict__ table)
{
    const int64_t e = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (e >= total) return;
    if (moments[e * 3] <= 0) { table[e] = __builtin_nan(""); return; }
    const double* s = partial + (size_t)e * slots;
    double a = 0.0;
    for (int k = 0; k < slots; ++k) a += s[k];
    table[e] = a / k2;
}

// one thread per image: the first maximum over the entries that are not NaN
__global__ __launch_bounds__(64) void ssim_select_kernel(const double* __restrict__ table, int64_t n_images, int ns, double* __restrict__ cssim,
                                                         int32_t* __restrict__ shift)
{
    const int64_t img = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (img >= n_images) return;
    const double* t = table + (size_t)img * ns * ns;
    int best = -1;
    double bv = 0.0;
    for (int k = 0; k < ns * ns; ++k) {
        const double x = t[k];
        if (x != x) continue;
        if (best < 0 || x > bv) { best = k; bv = x; }
    }
    cssim[img] = best < 0 ? __builtin_nan("") : bv;
    shift[2 * img] = best < 0 ? -1 : best / ns;
    shift[2 * img + 1] = best < 0 ? -1 : best % ns;
}

template <int BD>
int launch_partial(const uint16_t* sr, const uint16_t* hr, const uint8_t* mask, const int64_t* moments, const double* gauss, int64_t N, int S,
                   double* partial, hipStream_t s)
{
    const int bands = ssim_bands(S, BD), ctiles = ssim_ctiles(S, BD);
    hipLaunchKernelGGL(ssim_partial_kernel<BD>, dim3((unsigned)(bands * ctiles), (unsigned)N, (unsigned)(2 * BD + 1)), dim3(64 * (2 * BD + 1)), 0, s,
                       sr, hr, mask, moments, gauss, S, ctiles, partial);
    return check_launch("ssim_partial_kernel");
}

inline bool ssim_shape_ok(int64_t n_images, int S, int border)
{
    return n_images >= 1 && n_images <= 65535 && border >= 0 && border <= 3 && S >= 2 * border + SSIM_TAPS && S <= SSIM_MAX_S;
}

}  // namespace

}  // namespace probav

using namespace probav;

extern "C" size_t probav_ssim_scratch_bytes(int64_t n_images, int S, int border)
{
    if (!ssim_shape_ok(n_images, S, border)) return 0;
    const int ns = 2 * border + 1;
    return (size_t)n_images * ns * ns * ssim_bands(S, border) * ssim_ctiles(S, border) * sizeof(double);
}

extern "C" int probav_ssim_table(const uint16_t* sr, const uint16_t* hr, const uint8_t* mask, const int64_t* moments, const double* gauss11,
                                 int64_t n_images, int S, int border, void* scratch, size_t scratch_bytes, double* table, void* stream)
{
    if (!sr || !hr || !mask || !moments || !gauss11 || !scratch || !table || !ssim_shape_ok(n_images, S, border)) {
        set_error("probav_ssim_table: null/invalid argument (1 <= n_images <= 65535, 0 <= border <= 3, 2 border + 11 <= S <= 2048: the 11-tap "
                  "window needs 11 rows of the crop)", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (scratch_bytes < probav_ssim_scratch_bytes(n_images, S, border)) {
        set_error("probav_ssim_table: scratch smaller than probav_ssim_scratch_bytes()", hipSuccess);
        return PROBAV_ENOSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    double* partial = static_cast<double*>(scratch);
    int rc;
    switch (border) {
        case 0: rc = launch_partial<0>(sr, hr, mask, moments, gauss11, n_images, S, partial, s); break;
        case 1: rc = launch_partial<1>(sr, hr, mask, moments, gauss11, n_images, S, partial, s); break;
        case 2: rc = launch_partial<2>(sr, hr, mask, moments, gauss11, n_images, S, partial, s); break;
        default: rc = launch_partial<3>(sr, hr, mask, moments, gauss11, n_images, S, partial, s); break;
    }
    if (rc) return rc;
    const int ns = 2 * border + 1, K = S - 2 * border - SSIM_HALO;
    const int64_t total = n_images * ns * ns;
    hipLaunchKernelGGL(ssim_table_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, s, partial, moments, total,
                       ssim_bands(S, border) * ssim_ctiles(S, border), (double)K * (double)K, table);
    return check_launch("ssim_table_kernel");
}

extern "C" int probav_ssim_select(const double* table, int64_t n_images, int border, double* cssim, int32_t* shift, void* stream)
{
    if (!table || !cssim || !shift || n_images < 1 || n_images > 0x7fffffff || border < 0 || border > 3) {
        set_error("probav_ssim_select: null/invalid argument", hipSuccess);
        return PROBAV_EINVAL;
    }
    hipLaunchKernelGGL(ssim_select_kernel, dim3((unsigned)((n_images + 63) / 64)), dim3(64), 0, (hipStream_t)stream, table, n_images,
                       2 * border + 1, cssim, shift);
    return check_launch("ssim_select_kernel");
}
