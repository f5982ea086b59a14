// d loss / d x of the whole network as ONE launch (include/probav_hip.h: probav_input_grad): the reverse of models/modelsTF.py:23-27
// (xn = (x - mean) / std, mn = temporal mean), :45-47 (residConv1 on mn) and :58 (mainConv1 on xn, ReLU)
//
//   dx[n,h,w,t,c] = 1/std * (  sum_{a,b,d,co} G[n,h+1-a,w+1-b,t+1-d,co] * wmain[a,b,d,c,co]        mainConv1 'same': backward-data, 32 -> C over 27 taps
//                            + 1/T * sum_{a,b,co} D1[n,h-a,w-b,co] * w1[a,b,c,co] )                 residConv1 'valid': full correlation, the same for every frame
//
// G = g where act0 > 0 else 0 (the ReLU gate the backward-filter of mainConv1 is handed), D1 = d1 where gate1 > 0 (gate1 optional).
//
// The launch is a stream: it reads g and act0 (2 x 128 B per voxel) and writes C floats per voxel; 864 C MACs per voxel are little beside that.  One
// workgroup owns a tile of rh x cw pixels of one sample with ALL its frames.  It lands the gated G of the tile and of a one-voxel halo in LDS as it lies in
// memory, [voxel][32] -- out-of-range voxels (the 'same' borders in h, w and t) as zeros, so the tap loop has no branches.  Then a thread owns one pixel and
// one QUAD of the 32 channels: its 27 x 4 filter values stay in registers, it walks the T + 2 padded frames once, reads its 16 bytes of the nine (a, b)
// neighbours per frame (the eight lanes of a pixel read 128 consecutive bytes) and feeds three running sums -- the outputs t' - 2, t' - 1, t' that padded
// frame t' belongs to.  A finished sum is added up over the pixel's eight lanes (xor shuffles 1, 2, 4) and written.  Per pixel that is 9 (T + 2) reads of
// 128 B instead of 27 T, with no filter fetch inside the loop.  One (h, w) row of G is 25 KB at T = 9 and 53 KB at T = 19, so three whole rows do not fit
// at T = 19: the tile (ig_tile) is chosen per (H, T, C) inside an LDS budget that leaves room for two workgroups on a CU.  The halo is read again by the
// neighbouring tiles, out of L2 (the blocks are numbered so that a sample's tiles share an XCD).
//
// fp32 VALU, no atomics, a fixed summation order (a lane: frames, then the nine neighbours, then its four channels; then the lane tree): the same inputs give the same bits.  A workgroup
// reads one sample only.  Non-finite values ('Non-finite values'): a NaN or inf of g at an OPEN gate reaches every dx it feeds; at a closed
// gate (act0 <= 0, or act0 NaN) it is dropped, as the backward-filter kernels drop it.
#include "probav_common.h"

namespace probav {

constexpr int IG_F = 32;                        // mainConv1's output channels (num_filters of every shipped configuration; input_grad_supported refuses others upstream)
constexpr int IG_Q = IG_F / 4;                  // 16-byte words per voxel
constexpr int IG_R = 9;                         // residConv1's output channels (scale^2)
constexpr int IG_THREADS = 256;
constexpr int IG_MLP = 6;                       // pairs of 16-byte global loads a thread keeps in flight while it lands a tile
constexpr size_t IG_LDS_BUDGET = 80 * 1024;     // two workgroups per CU (160 KB)

struct IgTile { int rh, cw, nvp; size_t lds; };
// padded voxels of a tile: (rh + 2) x (cw + 2) x (T + 2) (nvp)
static size_t ig_lds(int rh, int cw, int T, int C, int* nvp)
{
    const int nv = (rh + 2) * (cw + 2) * (T + 2);
    if (nvp) *nvp = nv;
    return ((size_t)nv * IG_F + (size_t)rh * cw * C) * sizeof(float);
}
// the tile of least work per sample: 5 units per landed voxel (two global reads, one LDS store) and 9 (T + 2) C / 8 per lane slot of a 256-thread pass (its 16-byte LDS reads, in units of 128 B)
static IgTile ig_tile(int H, int T, int C)
{
    IgTile best = {0, 0, 0, 0};
    double best_cost = 0;
    for (int rh = 1; rh <= H; ++rh)
        for (int cw = 1; cw <= H; ++cw) {
            int nvp;
            const size_t lds = ig_lds(rh, cw, T, C, &nvp);
            if (lds > IG_LDS_BUDGET) break;
            const long tiles = (long)((H + rh - 1) / rh) * ((H + cw - 1) / cw);
            const long passes = ((long)rh * cw * IG_Q + IG_THREADS - 1) / IG_THREADS;
            const double cost = (double)tiles * (5.0 * nvp + 9.0 * (T + 2) * C / 8.0 * passes * IG_THREADS);
            if (best.rh == 0 || cost < best_cost) { best = {rh, cw, nvp, lds}; best_cost = cost; }
        }
    return best;
}

bool input_grad_supported(int H, int T, int C)
{
    return H >= 3 && T >= 1 && (C == 1 || C == 3) && (long)H * H * T < (1L << 24) && ig_tile(H, T, C).rh > 0;
}

// i / d for the small non-negative i and d of a tile (i < 2^16, d < 2^8), exact: (i + 0.5) / d is at least 0.5 / d away from an integer, and the two roundings
// of the product move it by less than 2^-22 of its value
__device__ __forceinline__ int ig_div(int i, float inv_d) { return (int)(((float)i + 0.5f) * inv_d); }

template <int C>
__global__ __launch_bounds__(IG_THREADS) void input_grad_kernel(int H, int T, int rh, int cw, int nvp, int tiles_w, int tiles,
                                                                const float* __restrict__ g, const float* __restrict__ act0, const float* __restrict__ wmain,
                                                                const float* __restrict__ d1, const float* __restrict__ gate1, const float* __restrict__ w1,
                                                                float inv_std, float inv_T, float* __restrict__ dx)
{
    extern __shared__ float4 ig_lds4[];
    float4* const G4 = ig_lds4;                                        // [nvp][IG_Q]: a padded voxel's 32 channels as they lie in memory
    float* const rs = reinterpret_cast<float*>(ig_lds4 + (size_t)IG_Q * nvp);   // [rh][cw][C]: the residual path's share of the tile's pixels
    const int tid = threadIdx.x;
    // consecutive block ids go round the XCDs, each with an L2 of its own: renumber so that a sample's tiles, which read each other's halos, share one
    // (the bijective form for any grid size; which block owns which tile changes nothing in what a tile computes)
    const int nwg = gridDim.x, xq = nwg >> 3, xr = nwg & 7, xcd = blockIdx.x & 7;
    const int wg = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (blockIdx.x >> 3);
    const int n = wg / tiles, tile = wg - n * tiles;
    const int th = tile / tiles_w, h0 = th * rh, w0 = (tile - th * tiles_w) * cw;
    const int T2 = T + 2, CW2 = cw + 2, RH2 = rh + 2;

    // ---- the gated G of the tile and its halo -> LDS.  A thread has IG_MLP pairs of 16-byte loads in flight (a slot outside the image loads the
    //      sample's first word and drops it: no branch between the loads), then selects and stores ----
    {
        const int per_col = T2 * IG_Q, total = RH2 * CW2 * per_col;
        const float inv_col = 1.f / (float)per_col, inv_cw2 = 1.f / (float)CW2;
        const float4* const g4 = reinterpret_cast<const float4*>(g) + (long)n * H * H * T * IG_Q;
        const float4* const a4 = reinterpret_cast<const float4*>(act0) + (long)n * H * H * T * IG_Q;
        for (int i0 = tid; i0 < total; i0 += IG_THREADS * IG_MLP) {
            float4 gv[IG_MLP], av[IG_MLP];
            int dst[IG_MLP];
            bool in[IG_MLP];
#pragma unroll
            for (int u = 0; u < IG_MLP; ++u) {
                const int idx = i0 + u * IG_THREADS;
                const int col = ig_div(idx, inv_col), r = idx - col * per_col;
                const int pt = r >> 3, q = r & 7;
                const int ph = ig_div(col, inv_cw2), pw = col - ph * CW2;
                const int h = h0 + ph - 1, w = w0 + pw - 1, t = pt - 1;
                in[u] = idx < total && h >= 0 && h < H && w >= 0 && w < H && t >= 0 && t < T;
                dst[u] = idx < total ? idx : -1;               // (idx = (padded voxel) * IG_Q + q)
                const int gi = in[u] ? ((h * H + w) * T + t) * IG_Q + q : 0;
                gv[u] = g4[gi];
                av[u] = a4[gi];
            }
#pragma unroll
            for (int u = 0; u < IG_MLP; ++u) {
                float4 v;
                v.x = (in[u] && av[u].x > 0.f) ? gv[u].x : 0.f; v.y = (in[u] && av[u].y > 0.f) ? gv[u].y : 0.f;
                v.z = (in[u] && av[u].z > 0.f) ? gv[u].z : 0.f; v.w = (in[u] && av[u].w > 0.f) ? gv[u].w : 0.f;
                if (dst[u] >= 0) G4[dst[u]] = v;
            }
        }
    }
    // ---- the residual path's share: one value per (pixel, c) of the tile ----
    {
        const int H1 = H - 2;
        const float inv_cwc = 1.f / (float)(cw * C);
        for (int i = tid; i < rh * cw * C; i += IG_THREADS) {
            const int lh = ig_div(i, inv_cwc), r = i - lh * cw * C, lw = r / C, c = r - lw * C;
            const int h = h0 + lh, w = w0 + lw;
            float acc = 0.f;
            if (h < H && w < H)
                for (int a = 0; a < 3; ++a) {
                    const int y = h - a;
                    if (y < 0 || y >= H1) continue;
                    for (int b = 0; b < 3; ++b) {
                        const int x = w - b;
                        if (x < 0 || x >= H1) continue;
                        const long di = (((long)n * H1 + y) * H1 + x) * IG_R;
                        const float* wp = w1 + ((a * 3 + b) * C + c) * IG_R;
#pragma unroll
                        for (int co = 0; co < IG_R; ++co) {
                            float d = d1[di + co];
                            if (gate1 && !(gate1[di + co] > 0.f)) d = 0.f;
                            acc = fmaf(d, wp[co], acc);
                        }
                    }
                }
            rs[i] = acc;
        }
    }
    __syncthreads();
    // ---- one (pixel, channel quad) per thread ----
    const float inv_cw = 1.f / (float)cw;
    for (int item = tid; item < rh * cw * IG_Q; item += IG_THREADS) {
        const int pix = item >> 3, q = item & 7;                 // (the eight lanes of a pixel sit in one wave and leave this loop together)
        const int lh = ig_div(pix, inv_cw), lw = pix - lh * cw;
        const int h = h0 + lh, w = w0 + lw;
        if (h >= H || w >= H) continue;
        int col[9];                                              // the nine (a, b) neighbours' padded columns, as word offsets: image pixel (h + 1 - a, w + 1 - b)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) col[a * 3 + b] = ((lh + 2 - a) * CW2 + (lw + 2 - b)) * T2 * IG_Q + q;
        float* const out = dx + (((long)n * H + h) * H + w) * T * C;
#pragma unroll 1
        for (int c = 0; c < C; ++c) {
            float4 wq[27];                                       // wmain[a][b][d][c][4 q .. 4 q + 3]
#pragma unroll
            for (int k = 0; k < 27; ++k) wq[k] = *reinterpret_cast<const float4*>(wmain + (k * C + c) * IG_F + q * 4);
            const float share = inv_T * rs[pix * C + c];
            float p0 = 0.f, p1 = 0.f, p2 = 0.f;                  // the running sums of outputs tp - 2, tp - 1, tp
            for (int tp = 0; tp < T2; ++tp) {                    // padded frame tp = image frame tp - 1 feeds output tp + d - 2 through tap d
                float4 gv[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) gv[k] = G4[col[k] + tp * IG_Q];
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const float4 w0q = wq[k * 3], w1q = wq[k * 3 + 1], w2q = wq[k * 3 + 2];
                    p0 = fmaf(gv[k].x, w0q.x, p0); p0 = fmaf(gv[k].y, w0q.y, p0); p0 = fmaf(gv[k].z, w0q.z, p0); p0 = fmaf(gv[k].w, w0q.w, p0);
                    p1 = fmaf(gv[k].x, w1q.x, p1); p1 = fmaf(gv[k].y, w1q.y, p1); p1 = fmaf(gv[k].z, w1q.z, p1); p1 = fmaf(gv[k].w, w1q.w, p1);
                    p2 = fmaf(gv[k].x, w2q.x, p2); p2 = fmaf(gv[k].y, w2q.y, p2); p2 = fmaf(gv[k].z, w2q.z, p2); p2 = fmaf(gv[k].w, w2q.w, p2);
                }
                if (tp >= 2) {                                   // output tp - 2 has its three frames: the pixel's eight lanes add up, lane 0 writes
                    float v = p0;
                    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
                    if (q == 0) out[(tp - 2) * C + c] = inv_std * (v + share);
                }
                p0 = p1; p1 = p2; p2 = 0.f;
            }
        }
    }
}

int input_grad(int N, int H, int T, int C, const float* g, const float* act0, const float* wmain, const float* d1, const float* gate1, const float* w1,
               float stdv, float* dx, hipStream_t s)
{
    if (N < 1 || !g || !act0 || !wmain || !d1 || !w1 || !dx || !(stdv > 0.f) || !input_grad_supported(H, T, C)) {
        set_error("input_grad: null / unsupported argument (H >= 3, T >= 1, C = 1 or 3, a tile of all T frames must fit the LDS budget)", hipSuccess);
        return PROBAV_EINVAL;
    }
    if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(act0) | reinterpret_cast<uintptr_t>(wmain)) & 15) { set_error("input_grad: g, act0 and wmain must be 16-byte aligned", hipSuccess); return PROBAV_EINVAL; }
    const IgTile tl = ig_tile(H, T, C);
    const int tiles_h = (H + tl.rh - 1) / tl.rh, tiles_w = (H + tl.cw - 1) / tl.cw, tiles = tiles_h * tiles_w;
    if ((long)N * tiles > 0x7fffffffL) { set_error("input_grad: batch too large for one launch", hipSuccess); return PROBAV_EINVAL; }
    const dim3 grid((unsigned)((long)N * tiles)), block(IG_THREADS);
    const float inv_std = 1.f / stdv, inv_T = 1.f / (float)T;
    if (C == 1) return launch_lds<input_grad_kernel<1>>("input_grad", grid, block, tl.lds, s, H, T, tl.rh, tl.cw, tl.nvp, tiles_w, tiles, g, act0, wmain, d1, gate1, w1, inv_std, inv_T, dx);
    return launch_lds<input_grad_kernel<3>>("input_grad", grid, block, tl.lds, s, H, T, tl.rh, tl.cw, tl.nvp, tiles_w, tiles, g, act0, wmain, d1, gate1, w1, inv_std, inv_T, dx);
}

}  // namespace probav
