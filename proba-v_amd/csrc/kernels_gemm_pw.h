// The general matrix route's fused pointwise pair (kernels_gemm_pw.hip): a residual block's expConv -> ReLU -> decConv, and its reverse, on the fp32-input
// MFMA without the hidden tensor ever reaching memory.  For F <= 64 input channels, D <= 64 output channels and ANY hidden count H; the operands are the
// route's (x [nvox][F], W1 [F][H], W2 [H][D]: effective weights as the direct kernels read them, no packed fragments).  The engine launches it where both
// probav_engine_set_gemm_route and probav_engine_set_gemm_pair are on and the tuned pair (mfma_pw_supported) does not take the shape.
#pragma once
#include "probav_common.h"

namespace probav {

bool gemm_pw_supported(int F, int H, int D, long nvox);
// dec = (relu(x W1 + b1)) W2 + b2, every element the k-ordered chain of gemm_conv_forward(expConv) then gemm_conv_forward(decConv): the same bits.
// hidden (optional): a dump of the hidden tile, [nvox][H]
int gemm_pw_forward(const float* x, const float* W1, const float* b1, const float* W2, const float* b2, float* dec, float* hidden,
                    long nvox, int F, int H, int D, hipStream_t s);
// slab floats of the reverse launch: slabs x (F H + H D + H + D); the slab count depends on nvox alone
size_t gemm_pw_backward_slab_floats(int F, int H, int D, long nvox);
// dX = dOut + d(pair)/dx ; dW1 [F][H], dW2 [H][D], db1 [H], db2 [D] (all overwritten; the slabs are summed by slab_sum_later in a fixed order)
int gemm_pw_backward(const float* x, const float* dT, const float* dOut, const float* W1, const float* b1, const float* W2, float* dX,
                     float* dW1, float* dW2, float* db1, float* db2, float* slabs, long nvox, int F, int H, int D, hipStream_t s);
// launch plan: v = {voxels per tile, tiles, hidden chunk width, chunks, workgroups, slabs, voxels per slab, 0} (forward: no slabs); false = not supported
bool gemm_pw_plan_ints(int F, int H, int D, long nvox, bool backward, int v[8]);

}  // namespace probav
