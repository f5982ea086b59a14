// Dataset builder kernels (gfx950): the hot path of utils/dataGenerator.py's checkpoints 2 and 3.
//   clear counts          count_nonzero of every frame's QM / SM, or of every patch's mask     (utils/dataGenerator.py:632, 381, 490, 761)
//   registration          integer-shift circular cross-correlation of every LR frame against its set's reference frame, the frame and its
//                         mask rolled by the argmax shift                                       (utils/dataGenerator.py:616-678)
//   patch extraction      reflect pad + unfold of frames and masks, masked-pixel count per patch (utils/dataGenerator.py:107-171, 553-596)
//
// Registration.  The reference calls skimage's register_translation(ref, img) (upsample_factor=1): the argmax over the 128 x 128 shifts s of
// |cc[s]|, cc[s] = sum_p ref[p] * img[p - s] (circular), ties to the first index in C order; then rolls img by s.  Here cc is that sum taken
// EXACTLY: for uint16 frames every product is < 2^32 and every sum < 2^46, so a uint64 accumulation is the integer itself.  Every value is
// non-negative, so |cc| = cc.  Offsetting ref by an integer c1 and img by c2 adds the same constant to every cc[s]
// (sum_p (ref-c1)(img_s-c2) = cc[s] - c2 sum ref - c1 sum img + n c1 c2), so the argmax is that of cc' over the offset frames; the offsets
// (each frame's floor mean) keep the fp32 transform small and are exact in fp32.
//
// One workgroup per frame: the offset frame's 2-D FFT in LDS (radix-2, 128 x 128 complex fp32 = 128 KiB), times the conjugate of the
// reference's spectrum (computed once per set by prep_ref_spectrum_kernel), inverse FFT: an fp32 estimate e[s] of cc'[s].
// Error bound (first order, Higham, Accuracy and Stability of Numerical Algorithms, thm 24.2, for each radix-2 transform of L = 14 stages with
// twiddles rounded from fp64, eta = mu + gamma_4 (sqrt2 + mu) < 7u, u = 2^-24; one complex product, 3u; ||F v||_inf <= ||v||_1):
//     |e[s] - cc'[s]| <= B = 4 L eta (||x'||_1 ||y'||_2 + ||x'||_2 ||y'||_1) = 392 u (||x'||_1 ||y'||_2 + ||x'||_2 ||y'||_1)
// with x' = ref - c1, y' = img - c2.  The true argmax s* therefore has e[s*] >= max e - 2B: every shift with e[s] >= max e - W,
// W = 2B (1 + 2^-10), is rescored exactly and the largest exact value wins, ties to the smaller index.  Up to PREP_CAND candidates are gathered
// in LDS; more (flat or constant frames: every shift ties) and every wave rescans the whole surface and rescores every shift in the window.
// probav_prep_xcorr_surface returns e and B for one pair (the bound is checked against the exact surface by tests/test_gpu_prep.py).
#include "probav_common.h"
#include "../../include/probav_hip.h"

namespace probav {

namespace {

constexpr int PN = 128, PNN = PN * PN, PREP_THREADS = 512, PREP_CAND = 512;
constexpr size_t PREP_LDS = PNN * sizeof(float2) + 64 * sizeof(float2) + PREP_CAND * sizeof(int) + 64 * sizeof(double);

__device__ __forceinline__ int brev7(int i) { return (int)(__brev((unsigned)i) >> 25); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

struct PrepLds {
    float2* buf;        // [128][128] spectrum; after the inverse transform: float surf[16384] | u16 img[16384] | u16 ref[16384]
    float2* tw;         // exp(-2 pi i k / 128), k < 64
    int* cand;          // candidate shifts
    double* red;        // reduction scratch
};

__device__ __forceinline__ PrepLds prep_lds()
{
    extern __shared__ __align__(16) unsigned char prep_smem[];
    PrepLds L;
    L.buf = reinterpret_cast<float2*>(prep_smem);
    L.tw = L.buf + PNN;
    L.cand = reinterpret_cast<int*>(L.tw + 64);
    L.red = reinterpret_cast<double*>(L.cand + PREP_CAND);
    return L;
}

__device__ __forceinline__ void init_twiddles(float2* tw)
{
    if (threadIdx.x < 64) {
        double s, c;
        sincospi((double)threadIdx.x / 64.0, &s, &c);
        tw[threadIdx.x] = make_float2((float)c, (float)-s);
    }
}

// block-wide sums of four doubles (every thread gets the totals)
__device__ void block_sum4(double v[4], double* red)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int k = 0; k < 4; ++k) {
        double x = v[k];
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        if (lane == 0) red[w * 4 + k] = x;
    }
    __syncthreads();
    for (int k = 0; k < 4; ++k) {
        double t = 0.0;
        for (int i = 0; i < PREP_THREADS / 64; ++i) t += red[i * 4 + k];
        v[k] = t;
    }
    __syncthreads();
}

// 2-D radix-2 transforms of buf (128 x 128, row-major).  Forward: decimation in time, input in bit-reversed order on both axes, output
// natural.  Inverse (unscaled, conjugate twiddles): decimation in frequency, input natural, output bit-reversed on both axes.
__device__ void fft2_dit_forward(float2* buf, const float2* tw)
{
    for (int axis = 0; axis < 2; ++axis)
        for (int lh = 0; lh < 7; ++lh) {
            const int h = 1 << lh;
            for (int b = threadIdx.x; b < PN * 64; b += PREP_THREADS) {
                const int line = axis == 0 ? (b >> 6) : (b & 127), k = axis == 0 ? (b & 63) : (b >> 7);
                const int pos = k & (h - 1), i0 = ((k >> lh) << (lh + 1)) + pos, i1 = i0 + h;
                const int a0 = axis == 0 ? line * PN + i0 : i0 * PN + line, a1 = axis == 0 ? line * PN + i1 : i1 * PN + line;
                const float2 w = tw[pos << (6 - lh)];
                const float2 u = buf[a0], t = cmul(buf[a1], w);
                buf[a0] = make_float2(u.x + t.x, u.y + t.y);
                buf[a1] = make_float2(u.x - t.x, u.y - t.y);
            }
            __syncthreads();
        }
}

__device__ void fft2_dif_inverse(float2* buf, const float2* tw)
{
    for (int axis = 0; axis < 2; ++axis)
        for (int lh = 6; lh >= 0; --lh) {
            const int h = 1 << lh;
            for (int b = threadIdx.x; b < PN * 64; b += PREP_THREADS) {
                const int line = axis == 0 ? (b >> 6) : (b & 127), k = axis == 0 ? (b & 63) : (b >> 7);
                const int pos = k & (h - 1), i0 = ((k >> lh) << (lh + 1)) + pos, i1 = i0 + h;
                const int a0 = axis == 0 ? line * PN + i0 : i0 * PN + line, a1 = axis == 0 ? line * PN + i1 : i1 * PN + line;
                const float2 tc = tw[pos << (6 - lh)], w = make_float2(tc.x, -tc.y);
                const float2 u = buf[a0], v = buf[a1];
                buf[a0] = make_float2(u.x + v.x, u.y + v.y);
                buf[a1] = cmul(make_float2(u.x - v.x, u.y - v.y), w);
            }
            __syncthreads();
        }
}

// floor mean of a frame (exact: the sum of 16384 uint16 is < 2^30) and the 1- and 2-norms of the offset frame
__device__ void frame_stats(const uint16_t* f, double* red, int& c, double& n1, double& n2)
{
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = threadIdx.x; p < PNN; p += PREP_THREADS) v[0] += (double)f[p];
    block_sum4(v, red);
    c = (int)(v[0] / PNN);                                 // exact sum, exact floor for non-negative values
    double w[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = threadIdx.x; p < PNN; p += PREP_THREADS) {
        const double d = (double)((int)f[p] - c);
        w[0] += fabs(d);
        w[1] += d * d;
    }
    block_sum4(w, red);
    n1 = w[0];
    n2 = sqrt(w[1]);
}

// offset frame -> forward spectrum in buf (bit-reversed load)
__device__ void load_and_transform(const uint16_t* f, int c, PrepLds& L)
{
    for (int p = threadIdx.x; p < PNN; p += PREP_THREADS)
        L.buf[brev7(p >> 7) * PN + brev7(p & 127)] = make_float2((float)((int)f[p] - c), 0.f);
    __syncthreads();
    fft2_dit_forward(L.buf, L.tw);
}

__global__ __launch_bounds__(PREP_THREADS) void prep_ref_spectrum_kernel(const uint16_t* __restrict__ frames, const int32_t* __restrict__ ref_frame,
                                                                          const int64_t* __restrict__ set_offsets, int64_t n_frames,
                                                                          float2* __restrict__ spec)
{
    PrepLds L = prep_lds();
    const int64_t r = ref_frame ? ref_frame[blockIdx.x] : (int64_t)blockIdx.x;        // NULL: frame = set (the diagnostic's pair)
    if (ref_frame && !(r >= set_offsets[blockIdx.x] && r < set_offsets[blockIdx.x + 1] && r >= 0 && r < n_frames))
        return;                                            // a reference outside its set: prep_register_kernel flags the set's frames
    init_twiddles(L.tw);
    const uint16_t* f = frames + (size_t)r * PNN;
    int c;
    double n1, n2;
    frame_stats(f, L.red, c, n1, n2);
    load_and_transform(f, c, L);
    float2* out = spec + (size_t)blockIdx.x * PNN;
    for (int p = threadIdx.x; p < PNN; p += PREP_THREADS) out[p] = L.buf[p];
}

__device__ __forceinline__ int set_of(const int64_t* off, int n_sets, int64_t f)
{
    int lo = 0, hi = n_sets - 1;                           // largest s with off[s] <= f
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= f) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One workgroup per frame.  DIAG: write the fp32 surface e (natural order) and info = {B, c_ref, c_img, max e} instead of registering.
template <bool DIAG>
__global__ __launch_bounds__(PREP_THREADS) void prep_register_kernel(const uint16_t* __restrict__ frames, const uint8_t* __restrict__ masks,
                                                                      const int64_t* __restrict__ set_offsets, int n_sets, int64_t n_frames,
                                                                      const int32_t* __restrict__ ref_frame, const float2* __restrict__ spec,
                                                                      int32_t* __restrict__ shifts, uint16_t* __restrict__ reg_frames,
                                                                      uint8_t* __restrict__ reg_masks, int32_t* __restrict__ reg_counts,
                                                                      float* __restrict__ surface, double* __restrict__ info)
{
    PrepLds L = prep_lds();
    __shared__ int n_cand;
    __shared__ unsigned long long best_w[PREP_THREADS / 64];
    const int64_t f = DIAG ? 1 : blockIdx.x;              // DIAG: frames = {ref, img}
    const int s = DIAG ? 0 : set_of(set_offsets, n_sets, f);
    const int64_t r = DIAG ? 0 : ref_frame[s];
    if (!DIAG && !(set_offsets[0] == 0 && set_offsets[n_sets] == n_frames && f >= set_offsets[s] && f < set_offsets[s + 1] &&
                   r >= set_offsets[s] && r < set_offsets[s + 1])) {
        if (threadIdx.x == 0) shifts[2 * f] = shifts[2 * f + 1] = PROBAV_PREP_BAD_SHIFT;   // violated precondition: nothing read, frame not written
        return;
    }
    const uint16_t* img = frames + (size_t)f * PNN;
    const uint16_t* ref = frames + (size_t)r * PNN;
    int sy = 0, sx = 0;

    if (DIAG || f != r) {                                  // the reference frame is not registered (utils/dataGenerator.py:638-639): shift 0
        init_twiddles(L.tw);
        if (threadIdx.x == 0) n_cand = 0;
        int c_img, c_ref;
        double n1_img, n2_img, n1_ref, n2_ref;
        frame_stats(img, L.red, c_img, n1_img, n2_img);
        frame_stats(ref, L.red, c_ref, n1_ref, n2_ref);
        load_and_transform(img, c_img, L);
        const float2* R = spec + (size_t)s * PNN;
        for (int p = threadIdx.x; p < PNN; p += PREP_THREADS) {
            const float2 a = R[p], b = L.buf[p];
            L.buf[p] = cmul(a, make_float2(b.x, -b.y));
        }
        __syncthreads();
        fft2_dif_inverse(L.buf, L.tw);

        // compact the real parts into surf[16384] in natural order, and take the fp32 maximum
        constexpr int PER = PNN / PREP_THREADS;
        float v[PER];
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int q = threadIdx.x + i * PREP_THREADS;
            v[i] = L.buf[brev7(q >> 7) * PN + brev7(q & 127)].x * (1.f / PNN);
            m = fmaxf(m, v[i]);
        }
        __syncthreads();
        float* surf = reinterpret_cast<float*>(L.buf);
        uint16_t* img_l = reinterpret_cast<uint16_t*>(surf + PNN);
        uint16_t* ref_l = img_l + PNN;
#pragma unroll
        for (int i = 0; i < PER; ++i) surf[threadIdx.x + i * PREP_THREADS] = v[i];
        for (int p = threadIdx.x; p < PNN; p += PREP_THREADS) { img_l[p] = img[p]; ref_l[p] = ref[p]; }
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if ((threadIdx.x & 63) == 0) L.red[32 + (threadIdx.x >> 6)] = (double)m;
        __syncthreads();
        double M = -INFINITY;
        for (int i = 0; i < PREP_THREADS / 64; ++i) M = fmax(M, L.red[32 + i]);
        const double u = 1.0 / 16777216.0;
        const double B = 392.0 * u * (n1_ref * n2_img + n2_ref * n1_img);
        const double thr = M - 2.0 * B * (1.0 + 1.0 / 1024.0);
        if (DIAG) {
            for (int p = threadIdx.x; p < PNN; p += PREP_THREADS) surface[p] = surf[p];
            if (threadIdx.x == 0) { info[0] = B; info[1] = c_ref; info[2] = c_img; info[3] = M; }
            return;
        }

        for (int q = threadIdx.x; q < PNN; q += PREP_THREADS)
            if ((double)surf[q] >= thr) {
                const int k = atomicAdd(&n_cand, 1);
                if (k < PREP_CAND) L.cand[k] = q;
            }
        __syncthreads();
        const int nc = n_cand;
        const bool slow = nc > PREP_CAND;                   // never truncated: every shift in the window is rescored
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = PREP_THREADS / 64;
        unsigned long long best = 0;
        const int n_iter = slow ? PNN : nc;
        for (int i = w; i < n_iter; i += nw) {
            int q;
            if (slow) {
                q = i;
                if (!((double)surf[q] >= thr)) continue;       // wave-uniform
            } else {
                q = L.cand[i];
            }
            const int qy = q >> 7, qx = q & 127;
            unsigned long long acc = 0;
            for (int p = lane; p < PNN; p += 64) {
                const int py = p >> 7, px = p & 127;
                acc += (unsigned long long)((unsigned)ref_l[p] * (unsigned)img_l[((py - qy) & 127) * PN + ((px - qx) & 127)]);
            }
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
            const unsigned long long key = (acc << 14) | (unsigned long long)(PNN - 1 - q);   // larger value first, then the smaller index
            best = key > best ? key : best;
        }
        if (lane == 0) best_w[w] = best;
        __syncthreads();
        unsigned long long kb = 0;
        for (int i = 0; i < nw; ++i) kb = best_w[i] > kb ? best_w[i] : kb;
        const int q = PNN - 1 - (int)(kb & (PNN - 1));
        sy = q >> 7;
        sx = q & 127;
    }

    // roll by (sy, sx): out[p] = in[p - s]; the mask the same, as 0/1; its clear count
    const uint8_t* msk = masks + (size_t)f * PNN;
    uint16_t* of = reg_frames + (size_t)f * PNN;
    uint8_t* om = reg_masks + (size_t)f * PNN;
    double cnt[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = threadIdx.x; p < PNN; p += PREP_THREADS) {
        const int src = (((p >> 7) - sy) & 127) * PN + (((p & 127) - sx) & 127);
        of[p] = img[src];
        const uint8_t b = msk[src] != 0;
        om[p] = b;
        cnt[0] += b;
    }
    block_sum4(cnt, L.red);
    if (threadIdx.x == 0) {
        shifts[2 * f] = sy > PN / 2 ? sy - PN : sy;          // skimage wraps indices > midpoint (strict): 64 stays +64
        shifts[2 * f + 1] = sx > PN / 2 ? sx - PN : sx;
        reg_counts[f] = (int32_t)cnt[0];
    }
}

__global__ __launch_bounds__(256) void prep_count_kernel(const uint8_t* __restrict__ data, int64_t len, int32_t* __restrict__ counts)
{
    const uint8_t* d = data + (size_t)blockIdx.x * len;
    int c = 0;
    for (int64_t i = threadIdx.x; i < len; i += 256) c += d[i] != 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    __shared__ int part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__device__ __forceinline__ int reflect_idx(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// one workgroup per (set, patch, frame): out [S][P][T][win][win], P = nh * nw row-major (utils/dataGenerator.py:586-593)
__global__ __launch_bounds__(256) void prep_patches_kernel(const float* __restrict__ frames, const uint8_t* __restrict__ masks, int T, int H, int W,
                                                            int pad, int win, int stride, int nh, int nw, float* __restrict__ patches,
                                                            uint8_t* __restrict__ pmasks, int32_t* __restrict__ counts)
{
    const int64_t b = blockIdx.x;                          // ((s * P) + p) * T + t
    const int t = (int)(b % T), p = (int)((b / T) % (nh * nw));
    const int64_t s = b / ((int64_t)T * nh * nw);
    const int y0 = (p / nw) * stride - pad, x0 = (p % nw) * stride - pad;
    const size_t in = ((size_t)s * T + t) * H * W;
    const size_t out = (size_t)b * win * win;
    int c = 0;
    for (int i = threadIdx.x; i < win * win; i += 256) {
        const int y = reflect_idx(y0 + i / win, H), x = reflect_idx(x0 + i % win, W);
        patches[out + i] = frames[in + (size_t)y * W + x];
        const uint8_t m = masks[in + (size_t)y * W + x] != 0;
        pmasks[out + i] = m;
        c += m;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    __shared__ int part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[b] = part[0] + part[1] + part[2] + part[3];
}

}  // namespace

}  // namespace probav

using namespace probav;

extern "C" int probav_prep_count_nonzero(const uint8_t* data, int64_t n_chunks, int64_t chunk_len, int32_t* counts, void* stream)
{
    if (!data || !counts || n_chunks < 0 || chunk_len < 1 || n_chunks > 0x7fffffff) {
        set_error("probav_prep_count_nonzero: null/invalid argument", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (n_chunks == 0) return PROBAV_OK;
    hipLaunchKernelGGL(prep_count_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, data, chunk_len, counts);
    return check_launch("prep_count_kernel");
}

extern "C" int probav_prep_register(const uint16_t* frames, const uint8_t* masks, const int64_t* set_offsets, int n_sets, int64_t n_frames,
                                    const int32_t* ref_frame, float* spec_scratch, int32_t* shifts, uint16_t* reg_frames, uint8_t* reg_masks,
                                    int32_t* reg_counts, void* stream)
{
    if (!frames || !masks || !set_offsets || !ref_frame || !spec_scratch || !shifts || !reg_frames || !reg_masks || !reg_counts ||
        n_sets < 1 || n_frames < 1 || n_frames > 0x7fffffff) {
        set_error("probav_prep_register: null/invalid argument", hipSuccess);
        return PROBAV_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    float2* spec = reinterpret_cast<float2*>(spec_scratch);
    const int rc = launch_lds<prep_ref_spectrum_kernel>("prep_ref_spectrum_kernel", dim3((unsigned)n_sets), dim3(PREP_THREADS), PREP_LDS, s, frames, ref_frame, set_offsets, n_frames, spec);
    if (rc != PROBAV_OK) return rc;
    return launch_lds<prep_register_kernel<false>>("prep_register_kernel", dim3((unsigned)n_frames), dim3(PREP_THREADS), PREP_LDS, s, frames, masks, set_offsets, n_sets,
                                                   n_frames, ref_frame, (const float2*)spec, shifts, reg_frames, reg_masks, reg_counts, (float*)nullptr, (double*)nullptr);
}

extern "C" int probav_prep_xcorr_surface(const uint16_t* pair, float* spec_scratch, float* surface, double* info, void* stream)
{
    if (!pair || !spec_scratch || !surface || !info) {
        set_error("probav_prep_xcorr_surface: null argument", hipSuccess);
        return PROBAV_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    float2* spec = reinterpret_cast<float2*>(spec_scratch);
    const int rc = launch_lds<prep_ref_spectrum_kernel>("prep_ref_spectrum_kernel", dim3(1), dim3(PREP_THREADS), PREP_LDS, s, pair, (const int32_t*)nullptr, (const int64_t*)nullptr, (int64_t)2, spec);
    if (rc != PROBAV_OK) return rc;
    return launch_lds<prep_register_kernel<true>>("prep_register_kernel<diag>", dim3(1), dim3(PREP_THREADS), PREP_LDS, s, pair, (const uint8_t*)nullptr,
                                                  (const int64_t*)nullptr, 1, (int64_t)2, (const int32_t*)nullptr, (const float2*)spec, (int32_t*)nullptr, (uint16_t*)nullptr, (uint8_t*)nullptr,
                                                  (int32_t*)nullptr, surface, info);
}

extern "C" int probav_prep_patches(const float* frames, const uint8_t* masks, int S, int T, int H, int W, int pad, int win, int stride,
                                   float* patches, uint8_t* patch_masks, int32_t* counts, void* stream)
{
    if (!frames || !masks || !patches || !patch_masks || !counts || S < 1 || T < 1 || H < 1 || W < 1 || pad < 0 || pad >= H || pad >= W ||
        win < 1 || stride < 1 || win > H + 2 * pad || win > W + 2 * pad) {
        set_error("probav_prep_patches: null/invalid argument", hipSuccess);
        return PROBAV_EINVAL;
    }
    const int nh = (H + 2 * pad - win) / stride + 1, nw = (W + 2 * pad - win) / stride + 1;
    const int64_t blocks = (int64_t)S * nh * nw * T;
    if (blocks > 0x7fffffff) { set_error("probav_prep_patches: too many patches for one launch", hipSuccess); return PROBAV_EINVAL; }
    hipLaunchKernelGGL(prep_patches_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames, masks, T, H, W, pad, win, stride, nh,
                       nw, patches, patch_masks, counts);
    return check_launch("prep_patches_kernel");
}
