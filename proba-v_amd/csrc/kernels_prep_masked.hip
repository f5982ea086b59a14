// Dataset builder, cloud-aware registration (gfx950): every LR frame against its set's reference frame by a MASKED normalised correlation
// over a bounded window of integer shifts, then the frame shifted without wrap-around.  The counterpart of the reference's
// registerFrame(..., tech='time') (utils/dataGenerator.py:663-666: skimage masked_register_translation + scipy.ndimage.shift); the
// statement the kernel equals bit for bit is probav_amd.prep.register_masked_numpy.
//
// The statement.  ref, img uint16 [128][128]; rc, ic their clear masks; window R, 1 <= R <= 32.  For every shift s = (dy, dx) in [-R, R]^2,
// dy outer, both ascending (visiting index i = (dy + R)(2R + 1) + dx + R):
//     img_s[p] = img[p - s], ic_s[p] = ic[p - s] where p - s lies inside the frame; ic_s = 0 outside (nothing wraps)
//     m = rc & ic_s, and over m, with a = ref, b = img_s:   n = sum 1   Sa = sum a   Sb = sum b   Saa = sum a^2   Sbb = sum b^2   Sab = sum a b
//     num = n Sab - Sa Sb      da = n Saa - Sa^2      db = n Sbb - Sb^2                                                     (int64)
//     candidate  <=>  10 n >= 3 nmax (nmax = max n over the window)  and  da > 0  and  db > 0
//     v = double(num) / sqrt(double(da) * double(db))
// The shift is the candidate with the largest v, ties to the smallest i; no candidate: shift (0, 0), registered = 0.
// Then out[p] = img[reflect(p - s)] (scipy's 'reflect', d c b a | a b c d), out_mask[p] = ic[p - s] inside the frame and 0 outside,
// count = sum out_mask.  A set's reference frame is copied through: shift (0, 0), registered = 1.
//
// Exactness.  All six moments are integers.  a, b < 2^16 and n <= 2^14, so Sa, Sb < 2^30; Saa, Sbb, Sab < 2^14 * 2^32 = 2^46;
// n Sab, n Saa, n Sbb < 2^60 and Sa Sb, Sa^2, Sb^2 < 2^60.  num is the difference of two values in [0, 2^60), so |num| < 2^60; da and db
// are such differences too and non-negative by Cauchy-Schwarz.  Every value and every product therefore stays below 2^61, inside int64,
// and integer sums do not depend on the order in which lanes, waves or launches add them.  A lane's share of one shift is at most 256
// pixels: its n and its Sa, Sb partials (< 2^24) are uint32, its Saa, Sbb, Sab partials (256 products below 2^32: < 2^40) uint64.
// v takes three int64 -> fp64 conversions (round to nearest even, as numpy's) and exactly four correctly rounded fp64 operations in the
// order written above.  They are spelled __dmul_rn, __dsqrt_rn, __ddiv_rn: single IEEE operations that the compiler may not contract or
// reassociate whatever flags the unit is built with (this unit takes no -ffp-contract flag).  v of a candidate is finite (da db > 0).
// Selection compares (v, i) with a fixed rule, larger v first and then the smaller i, in every lane, wave and the final pass: the result
// does not depend on which wave scored which shift.
//
// Shape.  One workgroup of 16 waves per frame.  LDS: the two frames as uint16 with unclear pixels ZEROED (a' = a rc, b' = b ic: then
// Sab = sum a' b'_s needs no mask, Sa = sum a' ic_s, Sb = sum b'_s rc, and likewise the squares), 2 x 32 KiB; the two masks as 0/1
// bytes, 2 x 16 KiB; v and n of every shift, 12 (2R + 1)^2 bytes (3.4 KiB at R = 8, 49.5 KiB at R = 32: 145.5 KiB in all, one workgroup
// per CU either way).  Wave w scores the shifts i = w, w + 16, ...; its 64 lanes take 64 CONSECUTIVE columns of one row per step, so a
// wave-wide read is 128 consecutive bytes of a frame row (each dword shared by two lanes: a broadcast) or 64 consecutive bytes of a mask
// row, at any dx: consecutive dwords fall into distinct banks, nothing serialises, whatever the row or the column offset.  Columns whose
// source x - dx falls outside the frame are skipped (their ic_s is 0: they add nothing to any moment), rows likewise by the loop bounds.
// The wave's partials are summed by shuffles; lane 0 forms num, da, db and v and stores (v, n).  After a barrier: nmax, the selection, and
// the same workgroup writes the shifted frame, the shifted mask and its clear count from the frame in global memory (L2-resident).
// No float atomics, no scratch from the caller.
#include "probav_common.h"
#include "../../include/probav_hip.h"

namespace probav {

namespace {

constexpr int MN = 128, MNN = MN * MN, MREG_THREADS = 1024, MREG_WAVES = MREG_THREADS / 64, MREG_MAX_WINDOW = 32;
constexpr double MREG_NO_VALUE = -4.0;                     // stored for a shift with da = 0 or db = 0 (every real v is within rounding of [-1, 1])

inline size_t mreg_lds_bytes(int R)
{
    const size_t ns = (size_t)(2 * R + 1) * (2 * R + 1);
    return 2 * MNN * sizeof(uint16_t) + 2 * MNN * sizeof(uint8_t) + ns * (sizeof(double) + sizeof(int32_t));
}

__device__ __forceinline__ int mreg_set_of(const int64_t* off, int n_sets, int64_t f)
{
    int lo = 0, hi = n_sets - 1;                           // largest s with off[s] <= f
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= f) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// (v, i) ordering of the selection: larger v, then the smaller visiting index
__device__ __forceinline__ bool mreg_better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }

// scipy.ndimage 'reflect' (d c b a | a b c d) for |shift| <= 32 < 128: one fold suffices
__device__ __forceinline__ int mreg_reflect(int i) { return i < 0 ? -i - 1 : (i >= MN ? 2 * MN - 1 - i : i); }

__global__ __launch_bounds__(MREG_THREADS) void prep_register_masked_kernel(const uint16_t* __restrict__ frames, const uint8_t* __restrict__ masks,
                                                                             const int64_t* __restrict__ set_offsets, int n_sets, int64_t n_frames,
                                                                             const int32_t* __restrict__ ref_frame, int R,
                                                                             int32_t* __restrict__ shifts, uint8_t* __restrict__ registered,
                                                                             uint16_t* __restrict__ out_frames, uint8_t* __restrict__ out_masks,
                                                                             int32_t* __restrict__ out_counts)
{
    extern __shared__ __align__(16) unsigned char mreg_smem[];
    __shared__ int red_n[MREG_WAVES];
    __shared__ double red_v[MREG_WAVES];
    __shared__ int red_i[MREG_WAVES];
    const int W = 2 * R + 1, NS = W * W;
    uint16_t* ref_l = reinterpret_cast<uint16_t*>(mreg_smem);
    uint16_t* img_l = ref_l + MNN;
    uint8_t* refm_l = reinterpret_cast<uint8_t*>(img_l + MNN);
    uint8_t* imgm_l = refm_l + MNN;
    double* v_s = reinterpret_cast<double*>(imgm_l + MNN);  // byte offset 96 KiB: 8-byte aligned
    int32_t* n_s = reinterpret_cast<int32_t*>(v_s + NS);

    const int64_t f = blockIdx.x;
    const int s = mreg_set_of(set_offsets, n_sets, f);
    const int64_t r = ref_frame[s];
    if (!(set_offsets[0] == 0 && set_offsets[n_sets] == n_frames && f >= set_offsets[s] && f < set_offsets[s + 1] &&
          r >= set_offsets[s] && r < set_offsets[s + 1])) {
        if (threadIdx.x == 0) shifts[2 * f] = shifts[2 * f + 1] = PROBAV_PREP_BAD_SHIFT;   // violated precondition: nothing read, frame not written
        return;
    }
    const uint16_t* img = frames + (size_t)f * MNN;
    const uint8_t* msk = masks + (size_t)f * MNN;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // w in a scalar register: the shift loop is wave-uniform
    int sy = 0, sx = 0, reg = 1;

    if (f != r) {                                          // the set's reference frame is copied through
        const uint16_t* ref = frames + (size_t)r * MNN;
        const uint8_t* rmsk = masks + (size_t)r * MNN;
        for (int p = threadIdx.x; p < MNN; p += MREG_THREADS) {
            const uint8_t mr = rmsk[p] != 0, mi = msk[p] != 0;
            ref_l[p] = mr ? ref[p] : (uint16_t)0;
            img_l[p] = mi ? img[p] : (uint16_t)0;
            refm_l[p] = mr;
            imgm_l[p] = mi;
        }
        __syncthreads();

        for (int i = w; i < NS; i += MREG_WAVES) {         // wave-uniform
            const int dy = i / W - R, dx = i % W - R;
            const int y0 = dy > 0 ? dy : 0, y1 = dy < 0 ? MN + dy : MN;
            unsigned n = 0, sa = 0, sb = 0;
            unsigned long long saa = 0, sbb = 0, sab = 0;
#pragma unroll 2
            for (int y = y0; y < y1; ++y) {
                const int pa = y * MN, pb = (y - dy) * MN - dx;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int x = h * 64 + lane;
                    if ((unsigned)(x - dx) < (unsigned)MN) {
                        const unsigned a = ref_l[pa + x], mr = refm_l[pa + x], b = img_l[pb + x], ms = imgm_l[pb + x];
                        const unsigned ta = a * ms, tb = b * mr;             // a over m, b over m (a, b are zero where their own mask is)
                        n += mr & ms;
                        sa += ta;
                        sb += tb;
                        sab += (unsigned long long)(a * b);                  // products < 2^32: the uint32 product is the integer
                        saa += (unsigned long long)(ta * a);
                        sbb += (unsigned long long)(tb * b);
                    }
                }
            }
            for (int o = 32; o > 0; o >>= 1) {
                n += __shfl_xor(n, o, 64);
                sa += __shfl_xor(sa, o, 64);
                sb += __shfl_xor(sb, o, 64);
                saa += __shfl_xor(saa, o, 64);
                sbb += __shfl_xor(sbb, o, 64);
                sab += __shfl_xor(sab, o, 64);
            }
            if (lane == 0) {
                const long long N = n, Sa = sa, Sb = sb;
                const long long num = N * (long long)sab - Sa * Sb, da = N * (long long)saa - Sa * Sa, db = N * (long long)sbb - Sb * Sb;
                double v = MREG_NO_VALUE;
                if (da > 0 && db > 0) v = __ddiv_rn((double)num, __dsqrt_rn(__dmul_rn((double)da, (double)db)));
                v_s[i] = v;
                n_s[i] = (int32_t)n;
            }
        }
        __syncthreads();

        int nmax = 0;
        for (int i = threadIdx.x; i < NS; i += MREG_THREADS) nmax = max(nmax, n_s[i]);
        for (int o = 32; o > 0; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o, 64));
        if (lane == 0) red_n[w] = nmax;
        __syncthreads();
        for (int k = 0; k < MREG_WAVES; ++k) nmax = max(nmax, red_n[k]);

        double bv = -INFINITY;
        int bi = NS;                                       // NS: no candidate
        for (int i = threadIdx.x; i < NS; i += MREG_THREADS) {
            const double v = v_s[i];
            if (10 * n_s[i] >= 3 * nmax && v > MREG_NO_VALUE && mreg_better(v, i, bv, bi)) { bv = v; bi = i; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (mreg_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { red_v[w] = bv; red_i[w] = bi; }
        __syncthreads();
        bv = -INFINITY;
        bi = NS;
        for (int k = 0; k < MREG_WAVES; ++k)
            if (mreg_better(red_v[k], red_i[k], bv, bi)) { bv = red_v[k]; bi = red_i[k]; }
        reg = bi < NS;
        if (reg) { sy = bi / W - R; sx = bi % W - R; }
    }

    // out[p] = img[reflect(p - s)]; the mask shifted with zeros coming in; its clear count
    uint16_t* of = out_frames + (size_t)f * MNN;
    uint8_t* om = out_masks + (size_t)f * MNN;
    int cnt = 0;
    for (int p = threadIdx.x; p < MNN; p += MREG_THREADS) {
        const int yy = (p >> 7) - sy, xx = (p & 127) - sx;
        of[p] = img[mreg_reflect(yy) * MN + mreg_reflect(xx)];
        uint8_t b = 0;
        if ((unsigned)yy < (unsigned)MN && (unsigned)xx < (unsigned)MN) b = msk[yy * MN + xx] != 0;
        om[p] = b;
        cnt += b;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    __syncthreads();                                       // red_n: the nmax pass has been read by every thread
    if (lane == 0) red_n[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int k = 0; k < MREG_WAVES; ++k) c += red_n[k];
        shifts[2 * f] = sy;
        shifts[2 * f + 1] = sx;
        registered[f] = (uint8_t)reg;
        out_counts[f] = c;
    }
}

}  // namespace

}  // namespace probav

using namespace probav;

extern "C" int probav_prep_register_masked(const uint16_t* frames, const uint8_t* masks, const int64_t* set_offsets, int n_sets, int64_t n_frames,
                                           const int32_t* ref_frame, int window, int32_t* shifts, uint8_t* registered, uint16_t* out_frames,
                                           uint8_t* out_masks, int32_t* out_counts, void* stream)
{
    if (!frames || !masks || !set_offsets || !ref_frame || !shifts || !registered || !out_frames || !out_masks || !out_counts || n_sets < 1 ||
        n_frames < 1 || n_frames > 0x7fffffff) {
        set_error("probav_prep_register_masked: null/invalid argument", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (window < 1 || window > MREG_MAX_WINDOW) {
        set_error("probav_prep_register_masked: window outside 1..32", hipSuccess);
        return PROBAV_EINVAL;
    }
    return launch_lds<prep_register_masked_kernel>("prep_register_masked_kernel", dim3((unsigned)n_frames), dim3(MREG_THREADS), mreg_lds_bytes(window),
                                                   (hipStream_t)stream, frames, masks, set_offsets, n_sets, n_frames, ref_frame, window, shifts, registered,
                                                   out_frames, out_masks, out_counts);
}
