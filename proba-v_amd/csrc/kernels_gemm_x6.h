// The general matrix route on the 16-bit matrix pipe (kernels_gemm_x6.hip): the convolution launches of kernels_gemm.hip -- forward and backward-data
// as implicit GEMMs, for ANY channel counts -- in x6 arithmetic (three bf16 truncation pieces per fp32 operand, six piece products on
// v_mfma_f32_32x32x16_bf16, smallest terms first: mac<X6> of x6_device.h).  Same operands, same geometries (gemm_conv_supported),
// same tiles and grids as the fp32 route; the engine launches them where probav_engine_set_gemm_x6 is on (engine.hip: conv_route).  The
// backward-filter stays the fp32 route's.
#pragma once
#include "probav_common.h"

namespace probav {

// y = act( conv(x * [gate > 0], w) + bias ) + skip: the contract of gemm_conv_forward
int gemm_x6_conv_forward(const ConvGeom& g, const float* x, const float* gate, const float* w, const float* bias, const float* skip, float* y, hipStream_t s);
// launch plan, as gemm_conv_plan_ints
bool gemm_x6_conv_plan_ints(const ConvGeom& g, int v[6]);
// the same kernel on the wide geometries (gemm_conv_supported_wide of kernels_gemm.h): where the engine's fourth switch hands it an exotic launch
int gemm_x6_conv_forward_wide(const ConvGeom& g, const float* x, const float* gate, const float* w, const float* bias, const float* skip, float* y, hipStream_t s);
bool gemm_x6_conv_plan_ints_wide(const ConvGeom& g, int v[6]);

}  // namespace probav
