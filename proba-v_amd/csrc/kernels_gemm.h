// The general matrix route (kernels_gemm.hip): a convolution and its backward-filter as implicit GEMMs on the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32: fp32 in, fp32 accumulate, an exact fma chain), for ANY channel counts.  They read the operands of the
// direct kernels (probav_common.h: conv3d_direct_forward / conv3d_direct_wgrad) -- the filter as [kh][kw][kt][Cin][Cout], no packed
// fragments -- and serve the engine wherever it would otherwise fall to those VALU kernels (engine.hip: conv_route / wgrad_route,
// probav_engine_set_gemm_route).
#pragma once
#include "probav_common.h"

namespace probav {

// forward / backward-data: 1x1x1 and 3x3x3 (3x3x1), zero pads <= 2 on each axis, mirrored H/W pads of 1, output extents that follow from
// the input's; no mirrored depth pad.  Any Cin, Cout, N
bool gemm_conv_supported(const ConvGeom& g);
// y = act( conv(x * [gate > 0], w) + bias ) + skip        (gate / bias / skip optional): the contract of conv3d_direct_forward
int gemm_conv_forward(const ConvGeom& g, const float* x, const float* gate, const float* w, const float* bias, const float* skip, float* y, hipStream_t s);
// launch plan: v = {tile voxels, tile output channels, grid.x (voxel tiles), grid.y (channel tiles), input channels per K chunk, K chunks per tap}
bool gemm_conv_plan_ints(const ConvGeom& g, int v[6]);

// backward-filter: the same kernel sizes, pads <= 1 (what wgrad_route does not call exotic)
bool gemm_wgrad_supported(const ConvGeom& g);
// dw, db as conv3d_direct_wgrad; `partial`: gemm_wgrad_partial_floats(g) floats of scratch, laid out [slabs][taps Cin Cout] then [slabs][Cout]
size_t gemm_wgrad_partial_floats(const ConvGeom& g);
int gemm_conv_wgrad(const ConvGeom& g, const float* x, const float* dy, const float* gate, float* dw, float* db, float* partial, hipStream_t s);
// launch plan: v = {slabs, voxels per slab, tile input channels, tile output channels, workgroups}; the slab count depends on the geometry alone
bool gemm_wgrad_plan_ints(const ConvGeom& g, int v[5]);

// The wide geometries -- what the engine calls exotic, the 19-frame reducer's layers and their backward-data forms -- on the SAME kernels (probav_engine_set_gemm_exotic):
// k x k x k and k x k x 1 for k in {1, 3, 5}; zero pads up to k - 1 per axis (backward-filter: up to 2); mirrored H/W pads and a mirrored depth pad (g.reflect_t)
// up to 2, each on an extent above the pad.  Beside the predicates above, which answer what they always did.  The kernels branch on the uniform g.reflect_t for the
// mirrored depth index; taps, tiles, slabs and the scratch layout follow from the geometry as before (taps up to 125).  A forward launch of more than 27 taps sums in two
// levels (a tap's chunks, then the taps: template parameter TWO of gemm_conv_fwd_kernel), which keeps a 9 000-term fp32 chain inside the route's 2e-6 bar
bool gemm_conv_supported_wide(const ConvGeom& g);
int gemm_conv_forward_wide(const ConvGeom& g, const float* x, const float* gate, const float* w, const float* bias, const float* skip, float* y, hipStream_t s);
bool gemm_conv_plan_ints_wide(const ConvGeom& g, int v[6]);
bool gemm_wgrad_supported_wide(const ConvGeom& g);
int gemm_conv_wgrad_wide(const ConvGeom& g, const float* x, const float* dy, const float* gate, float* dw, float* db, float* partial, hipStream_t s);
bool gemm_wgrad_plan_ints_wide(const ConvGeom& g, int v[5]);

// the forward's accumulator tiles per wave (1, 2 or 4, from Cout): shared with the route's x6 form (kernels_gemm_x6.hip)
int gemm_fwd_nt(const ConvGeom& g);

}  // namespace probav
