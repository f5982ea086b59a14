/* probav_hip.h -- C ABI of libprobav_hip.so: the gfx950 (MI355X) implementation of the WDSR-B Conv3D
 * forward/backward hot path of mmbajo/PROBA-V and its shift-compensated loss.
 *
 * The reference has no native/FFI layer: the path sits behind Python callables that dispatch to
 * TensorFlow ops.  Each entry point below names the reference call it replaces
 * (paths relative to the reference repository).  A binding needs nothing but this header: plain
 * pointers to DEVICE memory (fp32 unless stated), sizes, and a hipStream_t passed as void*.
 *
 * Conventions
 *   - activations [N][H][W][T][C], C innermost (the reference's layout; models/modelsTF.py:19);
 *     kernels [kh][kw][kt][Cin][Cout] (Keras).  All buffers contiguous, 16-byte aligned.
 *   - every call only ENQUEUES work on `stream` and returns; it never synchronises, allocates or
 *     frees device memory (so calls can be captured in a hipGraph).  The exceptions, each of which waits on the
 *     host, allocates or frees and therefore belongs outside a graph capture (tests/test_gpu_bands.py, HOST_WAIT_EXEMPT):
 *       (1) an engine's first call that launches with its layer table (a pass, a weight-norm or optimizer call) uploads that table, a few KB, once;
 *       (2) the single-operator entries probav_conv3d_forward (impl 1-4), probav_pw_forward and probav_pw_backward pack their filter into a scratch the library owns: every such call waits for `stream` to drain and uploads its packing jobs with a blocking copy (the first one also allocates the scratch);
 *       (3) their H3 form (impl 4, probav_conv3d_wgrad included) frees and allocates the library's amax table when a call needs more slots than any call before it;
 *       (4) probav_shift_loss_forward frees and allocates the library's candidate table when its batch times (2 border + 1)^2 exceeds that of every call before it.
 *     The packing scratch, the amax table and the candidate table are the library's own, one of each per process: calls of the entry
 *     points of (2)-(4) that overlap on two streams or two threads are unsafe (the second call repacks, resets or frees what the first
 *     one's kernels still read) -- keep them on one stream, or order them with events.  Everything else, the engine included, only
 *     enqueues.  probav_engine_create itself touches
 *     no device: the size and layout queries of a configuration answer on a host without one.
 *     probav_forward / probav_backward additionally fork work that is off the critical path (the
 *     low-frequency residual path, the sums of the backward-filter slabs) onto one engine-owned side
 *     stream by event and join it back into `stream` before returning: the caller sees plain
 *     stream order.  The side stream is created on the engine's first pass (make that pass outside
 *     a graph capture); PROBAV_NO_SIDE_STREAM=1 in the environment disables it.
 *   - return value: 0 = ok, PROBAV_EINVAL (-1) bad argument, PROBAV_ENOSPACE (-2) a workspace, scratch buffer or weight cache whose
 *     byte-size argument is below its size query's answer (read or written, nothing is launched; the FuseNet entries alone answer
 *     PROBAV_EINVAL), PROBAV_EHIP (-3) a HIP call failed; probav_last_error() gives the text (thread-local).
 *   - thread-safety: an engine handle and its workspace may be used by one thread at a time;
 *     distinct handles are independent (one process per GPU under data parallelism).
 *   - NaN and inf in any buffer are ordinary data.  What each entry point does with them, and the four contracts the library keeps (a
 *     non-finite training step shows in the loss or in probav_grad_guard; clean samples are untouched by poisoned batch mates; non-finite
 *     parameters are refused by the Python loaders; a non-finite prediction stays non-finite) is INTEGRATION.md, "Non-finite values".
 */
#ifndef PROBAV_HIP_H
#define PROBAV_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PROBAV_ABI_VERSION 7

/* Hyper-parameters of WDSRConv3D(name, band, mean, std, maxShift).build(scale, numFilters, kernelSize=3,
 * numResBlocks, expRate, decayRate, numImgLR, patchSizeLR, isGrayScale)   (models/modelsTF.py:8-17) */
typedef struct probav_net_cfg {
    int32_t scale;            /* 3 */
    int32_t num_filters;      /* 32 */
    int32_t num_res_blocks;   /* 12 */
    int32_t exp_rate;         /* 8 */
    int32_t dec_channels;     /* int(numFilters*decayRate) = 25 (models/modelsTF.py:182) */
    int32_t num_img_lr;       /* 9 (7, 13 also defined by the reference; models/modelsTF.py:62-69) */
    int32_t patch_size_lr;    /* 16 */
    int32_t max_shift;        /* 6 */
    float mean, std;          /* per-band constants (train.py:47-52) */
    int32_t in_channels;      /* 1: isGrayScale=True (every shipped cfg); 3: isGrayScale=False -- the input is [N,H,W,T,3], mainConv1 and
                                 residConv1 take three channels, the output stays one channel (models/modelsTF.py:19-20, :23-27) */
} probav_net_cfg;

typedef struct probav_engine probav_engine;

int probav_abi_version(void);
const char* probav_last_error(void);

/* ---- engine: the whole network ------------------------------------------------------------------ */
/* replaces WDSRConv3D(...).build(...)                                   models/modelsTF.py:15-43     */
int probav_engine_create(const probav_net_cfg* cfg, probav_engine** out);
void probav_engine_destroy(probav_engine* e);
/* number of trainable fp32 parameters (535 267 for p16t9c85r12) and the flat layout: layers in Keras
 * checkpoint order, per layer [g(Cout) | v(taps*Cin*Cout) | bias(Cout)]               */
int64_t probav_param_count(const probav_engine* e);
int probav_num_layers(const probav_engine* e);
/* name, offsets (in floats) and kernel shape of layer i; shape is [kh,kw,kt,Cin,Cout]               */
int probav_layer_info(const probav_engine* e, int i, char name[32], int64_t* g_off, int64_t* v_off,
                      int64_t* b_off, int32_t shape[5]);
/* kernel family: 0 = generic direct (VALU) kernels everywhere, 1 = fp32-MFMA row-tile kernels, 2 = fp32 MFMA + strip convolution,
 * 3 = 2 with the x6 kernels where they exist: fp32 in / fp32 out / fp32 accumulate, every fp32 product evaluated as six exact
 * bf16-piece products on the bf16 MFMA pipe, 4 (default) = the same kernels with the H3 arithmetic: three exact products of fp16 piece
 * pairs, every operand scaled by a power of two chosen from the largest magnitude of its scaling group -- one SAMPLE of an activation /
 * gradient tensor, one output COLUMN of a filter matrix (amax slots in the workspace, filled by the producing kernels).  3 and 4 are
 * held to the tolerances of 2 in tests/test_gpu_parity.py.  Results of one family are bitwise reproducible run to run; different
 * families differ by fp32 rounding.  In every family the forward result of a sample is independent of its batch mates, bit for bit
 * (models/modelsTF.py:15-43 has no cross-sample term).                                                                            */
int probav_engine_set_impl(probav_engine* e, int impl);
size_t probav_workspace_bytes(const probav_engine* e, int batch, int training);
/* per-kernel-class timing with HIP events recorded on the launch stream (bench.py's roofline leg).
 * probav_engine_profile(e, 1, n) creates events for n launches and starts recording (allocation
 * happens here, never inside forward/backward); after a stream synchronise,
 * probav_engine_profile_read sums elapsed ms, algorithmic MACs and launch counts per class
 * (nclass >= 8: wn, small, conv3 fwd, conv3 bwd-data, conv3 wgrad, 1x1x1 fwd, 1x1x1 bwd-data,
 * 1x1x1 wgrad) and clears the log.                                                                  */
int probav_engine_profile(probav_engine* e, int enable, int max_launches);
/* restrict the bracketing to the kernel classes whose bit is set (default: all).  An event pair around EVERY launch costs ~6 % of a
 * training step (the launches no longer overlap their ramps); bench.py brackets only the dominant class inside its timed region.  */
int probav_engine_profile_classes(probav_engine* e, uint32_t mask);
int probav_engine_profile_read(probav_engine* e, int nclass, double* ms, double* macs, int64_t* launches);

/* replaces  model(x, training=...)      models/trainClass.py:127,139 ; test.py:117 ; testClass.py:26
 * x [B, P+maxShift, P+maxShift, T, 1] -> y [B, scale*P, scale*P, 1].  With training != 0 the
 * activations needed by probav_backward stay in `ws`.                                               */
int probav_forward(probav_engine* e, const float* params, const float* x, float* y, void* ws,
                   size_t ws_bytes, int batch, int training, void* stream);
/* replaces  tape.gradient(loss, model.trainable_variables)              models/trainClass.py:131
 * dy [B, scale*P, scale*P, 1] -> grads[param_count] (overwritten).  Must follow probav_forward
 * (training=1) on the same ws / batch.                                                              */
int probav_backward(probav_engine* e, const float* params, const float* dy, float* grads, void* ws,
                    size_t ws_bytes, int batch, void* stream);
/* The same in two buffers (ABI 5).  probav_workspace_bytes(e, batch, 1) = saved_bytes + scratch_bytes: the first part is the SAVED STATE of a
 * training forward pass (what `tf.GradientTape` keeps: models/trainClass.py:126-131) -- probav_forward(training=1) needs no more than that --,
 * the second is what only the reverse pass writes on its way (gradient buffers, partial-sum slabs, its amax slots; meaningless before and
 * after).  probav_backward_split READS `saved` and writes `scratch`: the saved state of one forward pass can serve any number of reverse
 * passes (a retained graph, a gradient check), and a framework that tracks which operator writes which of its arguments sees a functional
 * operator.  wcache: the weight cache the forward pass ran from, or NULL.  probav_backward(ws) = probav_backward_split(ws, ws + saved_bytes). */
int probav_workspace_split(const probav_engine* e, int batch, size_t* saved_bytes, size_t* scratch_bytes);
int probav_backward_split(probav_engine* e, const float* params, const float* dy, float* grads, const void* saved, size_t saved_bytes,
                          void* scratch, size_t scratch_bytes, int batch, const void* wcache, size_t wcache_bytes, void* stream);
/* replaces  tape.gradient(loss, [x] + model.trainable_variables): the reverse of models/modelsTF.py:23-27 (normalisation, temporal mean),
 * :45-53 (the low-frequency residual path) and :58 (mainConv1) carried one layer further, down to the LR frames.
 * probav_backward_split with one more output: `grads` is filled exactly as probav_backward_split fills it (the same launches in the same
 * order, the same bits), and dx [B, P+maxShift, P+maxShift, T, C] receives d loss / d x -- one more launch at the end of the pass
 * (probav_input_grad below), fed by d loss / d relu(mainConv1) and by the residual path's gradient at residConv1, which the pass
 * forms anyway.  With frozen parameters the filter gradients are still computed; the caller drops them.                               */
int probav_backward_input(probav_engine* e, const float* params, const float* dy, float* grads, const void* saved, size_t saved_bytes,
                          void* scratch, size_t scratch_bytes, int batch, const void* wcache, size_t wcache_bytes, float* dx, void* stream);

/* ---- optimizer update fused with the weight normalisation of the next step ---------------------------------
 * replaces  optimizer.apply_gradients(...)  +  the WeightNormalization kernel recomputation of the NEXT model call
 *           (models/trainClass.py:132 ; models/modelsTF.py:191-197 ; Keras Nadam / Adam / SGD of train.py:77-83 by coefficients, as probav_nadam_step)
 * One launch updates all parameters in place (params, m, v: probav_param_count floats) and writes the effective weights of the UPDATED
 * parameters (both layouts, inverse norms, amax slots); a second one packs the MFMA operand fragments.  Everything lands in the
 * caller-owned weight cache (probav_weight_cache_bytes).  probav_forward_wc / probav_backward_wc are probav_forward / probav_backward
 * reading that cache instead of recomputing it: three launches leave every training step.  The cache is valid exactly as long as
 * `params` is not modified by anyone else.                                                                                          */
size_t probav_weight_cache_bytes(const probav_engine* e);
int probav_optimizer_step_fused(probav_engine* e, float* params, const float* grads, float* m, float* v, float lr, float beta1,
                                float beta2, float eps, float c_g, float c_m, float c_v, void* wcache, size_t wcache_bytes, void* stream);
/* The same cache from parameters that nothing is updating (inference, evaluation: `model(x)` many times on fixed weights -- test.py:117,
 * models/testClass.py:26): weight normalisation + operand packing once, then every probav_forward_wc starts at its first convolution. */
int probav_weight_cache_build(probav_engine* e, const float* params, void* wcache, size_t wcache_bytes, void* stream);
int probav_forward_wc(probav_engine* e, const float* params, const float* x, float* y, void* ws, size_t ws_bytes, int batch,
                      int training, const void* wcache, size_t wcache_bytes, void* stream);
int probav_backward_wc(probav_engine* e, const float* params, const float* dy, float* grads, void* ws, size_t ws_bytes, int batch,
                       const void* wcache, size_t wcache_bytes, void* stream);

/* ---- loss / metric ------------------------------------------------------------------------------
 * Common to the three losses below (tests/test_gpu_losses.py holds each point to the fp64 oracle):
 *  - shapes: size > 2 * border for L1 / L2 / cPSNR; crop = size - 2 * border in [3, 100] for sobel_l1_mix and in [2, 140] for l1msssim
 *    (their backward kernels hold the crop in LDS, (3 L^2 + (L + 2)^2) floats and (5 L + L^2) doubles, within the device's 160 KiB).  A shape outside
 *    is PROBAV_EINVAL from the FORWARD as from the backward, with the limit in probav_last_error(); nothing is launched.
 *  - ties: among candidates that tie exactly the FIRST in shift order (smallest i * (2 * border + 1) + j) is selected, and the backward
 *    differentiates that one shift.  tf.reduce_min, which the reference uses, splits the gradient equally among the tied shifts.
 *  - no clear pixel: a shift under which a sample has no clear pixel (n = 0) is no candidate; the minimum is over the others (as in
 *    probav_score_select).  A sample with no clear pixel under ANY shift has l1 = l2 = cpsnr = loss = NaN and arg 0, the batch means are
 *    then NaN, and its gradient is NaN inside the crop (0 on the border ring); the gradients of the other samples are unaffected.  For
 *    l1msssim, one scalar for the batch, any such sample makes loss NaN and arg 0; its gradient is then unspecified (not for use).
 *  - the gradient is written for every element of dpred: exactly 0 on the border ring.                                               */
/* replaces Losses.shiftCompensatedL1Loss / L2Loss / cPSNR               models/loss.py:37-84
 * hr, pred [B,S,S,1] f32; mask [B,S,S,1] uint8 (non-zero = clear pixel).  Outputs (device):
 * l1[B], l2[B] minima over the (2*border+1)^2 shifts, cpsnr[B] maximum, arg_l1[B]/arg_l2[B] the
 * arg-min shift ids (i*(2*border+1)+j), mean_l1/mean_l2 the batch means (the two loss scalars).     */
int probav_shift_loss_forward(const float* hr, const uint8_t* mask, const float* pred, int batch, int size,
                              int border, int bit_depth, float* l1, float* l2, float* cpsnr, int32_t* arg_l1,
                              int32_t* arg_l2, float* mean_l1, float* mean_l2, void* stream);
/* gradient of mean_l1 (which=1) or mean_l2 (which=2) w.r.t. pred; `upstream` = device scalar or NULL */
int probav_shift_loss_backward(const float* hr, const uint8_t* mask, const float* pred, const int32_t* arg,
                               int batch, int size, int border, int which, const float* upstream,
                               float* dpred, void* stream);
/* cfg loss = sobel_l1_mix: Losses.shiftCompensatedL1EdgeLoss                     models/loss.py:86-97,126-137,214-219
 * per sample min over the (2*border+1)^2 shifts of  pi * L1 + (1 - pi) * sum|sobel_edges(HR) - sobel_edges(corrected SR)| / n
 * (tf.image.sobel_edges: REFLECT-padded 3x3 correlations; pi = Losses.pi = 0.7).  loss [batch], arg [batch],
 * mean: TWO floats (mean over the batch, scratch).  The backward differentiates the arg-min shift, bias term included.   */
int probav_shift_l1edge_forward(const float* hr, const uint8_t* mask, const float* pred, int batch, int size, int border,
                                float pi, float* loss, int32_t* arg, float* mean, void* stream);
int probav_shift_l1edge_backward(const float* hr, const uint8_t* mask, const float* pred, const int32_t* arg, int batch,
                                 int size, int border, float pi, const float* upstream, float* dpred, void* stream);
/* cfg loss = l1msssim: Losses.shiftCompensatedRevSSIM                             models/loss.py:99-124,189-212
 * ONE scalar for the batch: min over the shifts of  eta * (1 - sum_{scale,sample} luminance * prod_scale(contrast * structure) / B)
 * + (1 - eta) * weighted L1 / (B * (2^bit_depth - 1)), with the reference's five exponential windows (its quirks restated in
 * kernels_loss.hip).  scratch: probav_revssim_scratch_bytes() bytes, written by the forward and read by the backward; loss and arg
 * are one element each (the batch shares the shift).                                                                               */
size_t probav_revssim_scratch_bytes(int batch, int border);
int probav_revssim_forward(const float* hr, const uint8_t* mask, const float* pred, int batch, int size, int border, int bit_depth,
                           float eta, void* scratch, size_t scratch_bytes, float* loss, int32_t* arg, void* stream);
int probav_revssim_backward(const float* hr, const uint8_t* mask, const float* pred, const int32_t* arg, const void* scratch,
                            int batch, int size, int border, int bit_depth, float eta, const float* upstream, float* dpred, void* stream);
/* replaces optimizer.apply_gradients with Keras Nadam                   models/trainClass.py:132, train.py:79-81
 * in place on the flat parameter buffer; m, v = first / second moment slots (n floats each).  The caller supplies the
 * step-dependent scalars of SURVEY.md A.5 (computed in double): c_g = (1-mu_t)/(1-Pi_t), c_m = mu_{t+1}/(1-Pi_t*mu_{t+1}),
 * c_v = 1/(1-beta2^t).  The update is  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  theta -= lr (c_g g + c_m m) / (sqrt(c_v v) + eps),
 * which also is Keras Adam (c_g = 0, c_m = sqrt(1-b2^t)/(1-b1^t), c_v = 1) and plain SGD (c_g = 1, c_m = 0, c_v = 0, eps = 1): the
 * three optimizers of train.py:77-83 are one fused launch.                                                           */
int probav_nadam_step(float* params, const float* grads, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                      float eps, float c_g, float c_m, float c_v, void* stream);
/* ---- optimizer options on the device: global-norm clip, non-finite guard, weight EMA (additions made UNDER ABI 7: purely additive, the
 * version number stays) ---------------------------------------------------------------------------------------------------------------
 * replaces  the Keras optimizer arguments `global_clipnorm` (= tf.clip_by_global_norm over all gradient tensors), `use_ema` / `ema_momentum`
 *           (optimizer_v2 of train.py:77-83), and adds a guard Keras does not have: a step whose gradient holds an inf or a NaN is dropped.
 * probav_grad_guard: two launches.  (1) the sum of squares of the flat gradient in fp64, fixed grid, fixed order, one fp64 partial per
 * workgroup in `scratch` (probav_grad_guard_scratch_bytes; no floating-point atomics: the same gradient gives the same bits).  (2) one
 * workgroup sums the partials in index order and writes the control block:
 *     total = sum g^2 (fp64);  norm = sqrt(total);  scale = clipnorm / max(norm, clipnorm) in fp64, rounded once to fp32 (1 when clipnorm <= 0)
 *     skip  = 1 when skip_nonfinite != 0 and total is not finite (squares of finite fp32 values cannot overflow an fp64 sum: total is
 *             non-finite exactly when some element is), else 0;  skipped_total += skip  (the caller zeroes the block once, before the first step)
 * A non-finite total with clipping on and the guard off gives scale = NaN, as tf.clip_by_global_norm does.  One call = one step's decision.
 * The *_guarded steps read the block on the device: g' = g * scale enters the update rule of probav_nadam_step; with skip set params, m, v
 * and ema are left untouched (the fused step still normalises and packs the unchanged parameters: the weight cache stays valid).  With
 * ema != NULL, after the update:  ema = ema_momentum * ema + (1 - ema_momentum) * params   (Keras's rule, no de-biasing; the caller
 * initialises ema to the initial parameters).  ctl == NULL: no scaling and no skip (EMA only).  With ctl->scale == 1, skip == 0 and
 * ema == NULL the guarded steps leave the bits of the plain ones.  Nothing here is read by the host.                                     */
typedef struct probav_guard_ctl {
    float scale;              /* what every gradient element is multiplied by */
    uint32_t skip;            /* 1: this step is dropped */
    uint32_t skipped_total;   /* running count of dropped steps */
    float norm;               /* global L2 norm of the gradient, fp64 rounded to fp32 */
} probav_guard_ctl;
size_t probav_grad_guard_scratch_bytes(int64_t n);
int probav_grad_guard(const float* grads, int64_t n, float clipnorm /* <= 0: off */, int skip_nonfinite, void* scratch, size_t scratch_bytes,
                      probav_guard_ctl* ctl /* device */, void* stream);
int probav_nadam_step_guarded(float* params, const float* grads, float* m, float* v, float* ema /* or NULL */, int64_t n, float lr,
                              float beta1, float beta2, float eps, float c_g, float c_m, float c_v, float ema_momentum,
                              const probav_guard_ctl* ctl /* device, or NULL: EMA only */, void* stream);
int probav_optimizer_step_fused_guarded(probav_engine* e, float* params, const float* grads, float* m, float* v, float lr, float beta1,
                                        float beta2, float eps, float c_g, float c_m, float c_v, void* wcache, size_t wcache_bytes,
                                        float* ema /* or NULL */, float ema_momentum, const probav_guard_ctl* ctl /* device, or NULL */,
                                        void* stream);
/* replaces tf.clip_by_value(sr, 0, 2**16); tf.round(sr)                 test.py:118-119             */
int probav_clip_round(const float* in, float* out, size_t n, float lo, float hi, void* stream);

/* ---- single operators (what the engine is made of; exported for parity tests) ------------------- */
/* geometry: int32[17] = N, Hi,Wi,Ti,Cin, Ho,Wo,To,Cout, kh,kw,kt, ph,pw,pt, reflect_hw, relu        */
/* y = act(conv(x * [gate>0], w) + bias) + skip; impl 0 = direct, 1 = MFMA row-tile, 2 = MFMA strip, 3 = x6 (strip or row-tile),
 * 4 = H3 (the same kernels with three products of scaled fp16 piece pairs; operand maxima are measured by the library) */
int probav_conv3d_forward(const int32_t geom[17], const float* x, const float* gate, const float* w,
                          const float* bias, const float* skip, float* y, int impl, void* stream);
size_t probav_conv3d_wgrad_scratch_bytes(const int32_t geom[17], int impl);
int probav_conv3d_wgrad(const int32_t geom[17], const float* x, const float* dy, const float* gate,
                        float* dw, float* db, void* scratch, size_t scratch_bytes, int impl, void* stream);
/* fused expConv_i (1x1x1, 32->256) + ReLU + decConv_i (1x1x1, 256->D<=26)      models/modelsTF.py:179-183
 * x [nvox,32], w1 [32,256], b1 [256], w2 [256,D], b2 [D] -> dec [nvox,D]; the 256-channel tensor never reaches HBM
 * impl 2 = fp32 MFMA, 3 = fp32 products as six bf16-piece products on the bf16 MFMA pipe ("x6", same accuracy class),
 * 4 = three products of scaled fp16 piece pairs ("H3", same accuracy class) */
/* vox_per_sample: voxels of one patch (nvox must be a multiple; 0 = treat the call as one sample): the unit the H3 arithmetic scales by */
int probav_pw_forward(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* dec,
                      int64_t nvox, int64_t vox_per_sample, int D, int impl, void* stream);
/* its reverse pass: d_dec [nvox,D], d_skip [nvox,32] (gradient arriving over the residual connection)
 * -> dx = d_skip + dL/dx [nvox,32], dw1 [32,256], db1 [256], dw2 [256,D], db2 [D]
 * ACCURACY OF THE FILTER GRADIENTS, impl 4 (declared bound; tests/test_gpu_h3_range.py::test_pointwise_filter_gradients_slice_by_slice
 * asserts it).  dx, db1, db2 and every slice of dw1 / dw2 whose channel is within 2^-18 of its sample's largest value are at fp32 level
 * (<= 5e-6 of the slice's own maximum, the bar impl 2 and 3 meet on every slice).  dw1 (a ROW = one input channel of x) and dw2 (a
 * COLUMN = one channel of d_dec) contract over the voxels, but the kernel cuts x and d_dec into their two fp16 pieces ONCE per tile
 * with the per-SAMPLE power-of-two scale that the products contracting over those channels need; a channel that sits 2^-k below its
 * sample's maximum keeps both pieces normal only down to k = 18, and loses one bit of its second piece per binade below: the row /
 * column of such a channel is resolved to <= 1e-4 of its own maximum at k = 24 (measured 4.8e-5 / 9.0e-5) -- still far inside
 * north_star's 1e-3, and invisible in a whole-tensor norm.  The cure of the 3x3x3 backward-filter kernel (second pieces lifted by 2^11,
 * the cross products in an accumulator set of their own) needs 256 more accumulator registers than a wave has.  impl 2 / 3: no such floor. */
/* db1 AT LARGE BATCHES (measured; tests/test_gpu_plans.py::test_pointwise_plan_backward_matches_oracle).  The outputs of the bf16 / fp16 MFMA pipe carry a one-sided
 * error of about -1.4e-8 of their magnitude (the fp32 MFMA of impl 2: none).  db1 is the one plain sum of such outputs over every voxel of the call, so the term grows with
 * the voxel count while db1 grows with its square root.  impl 4 up to 1 024 samples (pw_bwd_w4_kernel) alternates the sign of that product tile by tile and cancels it:
 * 2.9e-7 of max |db1| at 128 x 4 356 voxels.  The general forms (impl 3; impl 4 above 1 024 samples) sum it as it comes: 5e-7 at 4 356 voxels, 5.2e-6 at 128 x 4 356. */
size_t probav_pw_backward_scratch_bytes(int D);
int probav_pw_backward(const float* x, const float* d_dec, const float* d_skip, const float* w1, const float* b1,
                       const float* w2, float* dx, float* dw1, float* db1, float* dw2, float* db2, void* scratch,
                       size_t scratch_bytes, int64_t nvox, int64_t vox_per_sample, int D, int impl, void* stream);
/* the network's input gradient as ONE launch: the reverse of models/modelsTF.py:23-27 (xn = (x - mean) / std, mn = the temporal mean of xn),
 * :45-47 (residConv1, 3x3 'valid' on mn) and :58 (mainConv1, 3x3x3 'same' on xn, ReLU)
 *   dx[n,h,w,t,c] = 1/std * (  sum_{a,b,d,co} G[n,h+1-a,w+1-b,t+1-d,co] * wmain[a,b,d,c,co]
 *                            + 1/T * sum_{a,b,co} D1[n,h-a,w-b,co] * w1[a,b,c,co] )          (indices outside a tensor contribute 0)
 * G = g where act0 > 0, else 0; D1 = d1 where gate1 > 0 (gate1 == NULL: d1 as it is).
 * g, act0 [B,H,H,T,32]: d loss / d relu(mainConv1) and relu(mainConv1); wmain [3,3,3,C,32] (all three 16-byte aligned);
 * d1, gate1 [B,H-2,H-2,9]: the gradient at residConv1's output and that output; w1 [3,3,1,C,9]; C = 1 or 3; dx [B,H,H,T,C].
 * fp32 VALU, no atomics, one fixed summation order: the same inputs give the same bits, and a sample never reads another sample.      */
int probav_input_grad(int batch, int H, int T, int C, const float* g, const float* act0, const float* wmain, const float* d1,
                      const float* gate1 /* or NULL */, const float* w1, float stdv, float* dx, void* stream);
/* weight normalisation of every layer of the engine: params -> weff, weffT, inv_norm (ws-internal
 * layouts, exported for tests): sizes probav_weff_count() floats and probav_cout_total() floats      */
int64_t probav_weff_count(const probav_engine* e);
int64_t probav_cout_total(const probav_engine* e);
int probav_wn_forward(probav_engine* e, const float* params, float* weff, float* weffT, float* inv_norm, void* stream);
/* grads[param_count]: the g and v entries of every layer are written (d loss / d g, d loss / d v); the bias entries are left as they were
 * (a bias is no function of weff: the passes write its gradient themselves)                                                          */
int probav_wn_backward(probav_engine* e, const float* params, const float* dweff, const float* inv_norm,
                       float* grads, void* stream);

/* What runs on the engine's side stream (see the conventions at the top): 0 = nothing, 1 = the slab sums and the low-frequency residual
 * path, 2 (default) = also the backward-filter kernels of the 3x3x3 layers, whose results only the weight-norm backward at the very end
 * reads: at the lowest stream priority they fill the tails of the caller's chain (-3 % per step) -- and share the chip with the kernels
 * they run beside, so a per-kernel timing (bench.py's roofline leg, a rocprofv3 kernel summary) is taken in mode 1.                        */
int probav_engine_side_stream(probav_engine* e, int mode);

/* ---- measurement aid -------------------------------------------------------------------------------------------------------------- */
/* Enqueues `launches` launches of nothing but dependent v_mfma_f32_32x32x16_f16 on every compute unit (one wave per SIMD, `iters` x 16
 * MFMAs per wave, operands from `seed`: 128 x 16 bytes of fp16 data).  Timed by the caller (events on `stream`), it gives the matrix rate
 * THIS device sustains under load -- the boxes of a pool differ -- as launches * 256 * 4 * iters * 16 * 32768 FLOP / time.
 * `sink` receives 256 * 256 floats.  bench.py reports it as `sustained_mfma_tflops` beside the step time.                                */
int probav_mfma_probe(const void* seed, float* sink, int iters, int launches, void* stream);
/* The same with the MFMA shape as a parameter (ABI 4): shape 0 = v_mfma_f32_32x32x16_f16 (iters x 16 MFMAs of 32 768 FLOP per wave), shape 1 =
 * v_mfma_f32_16x16x32_f16 (iters x 32 MFMAs of 16 384 FLOP: the same FLOP per wave, the same cycles per FLOP).  Where the chip lowers its clock
 * under matrix load the clock it holds depends on the shape (MI355X_MICROARCH.md, DVFS give-back, item 7): bench.py reports both rates. */
int probav_mfma_probe_shape(const void* seed, float* sink, int iters, int launches, int shape, void* stream);

/* ---- introspection of a training forward pass (parity tests; tf.keras would expose these as layer outputs) -------------------- */
/* where a saved activation lives inside the caller's workspace after probav_forward(training=1): offset and length in floats.
 * kind: ACT = input of residual block `index` (index num_res_blocks = output of the last block; ACT 0 = relu(mainConv1), models/modelsTF.py:58),
 * DEC = decConv_index output (:182-183), RED = relu(convReducer_{index+1}) (:159-160), RESID1 = relu(residConv1) (:47)                 */
#define PROBAV_VIEW_ACT 0
#define PROBAV_VIEW_DEC 1
#define PROBAV_VIEW_RED 2
#define PROBAV_VIEW_RESID1 3
#define PROBAV_VIEW_INPUT 4         /* the normalised input xn [B, P+maxShift, P+maxShift, T, C] (models/modelsTF.py:23-24): its count is the size of d loss / d x */
int probav_workspace_view(const probav_engine* e, int batch, int training, int kind, int index, int64_t* offset_floats, int64_t* count);
/* the post-ReLU hidden tile relu(expConv_block(x)) [B*(P+s)^2*T][256] (models/modelsTF.py:179-180) exactly as the fused forward kernel
 * of the current kernel family (3 or 4) evaluates it -- that tensor never reaches memory otherwise.  Call after probav_forward(training=1)
 * with the same workspace; the ReLU gates of the reverse pass are the signs of these values.  On an engine whose un-fused route runs in
 * x6 arithmetic (probav_engine_gemm_arith == 1, no fused pair) it is the route's expConv launch again, as the reverse pass recomputes
 * the hidden tensor: [..][F x expRate], dec_scratch is not written.                                                                    */
int probav_debug_hidden(probav_engine* e, const float* params, const void* ws /* saved state: read only */, size_t ws_bytes, int batch, int block, float* hidden,
                        float* dec_scratch /* [voxels][dec channels] floats: the launch's regular output, discarded */,
                        const void* wcache /* the weight cache the forward pass ran from, or NULL */, void* stream);
/* ABI 7.  Which arrangement probav_debug_hidden evaluates the tile in (kernel family 4): 0 (default) the 32x32x16 one, whose order of additions is the one the
 * reverse pass recomputes the tile -- and decides its ReLU gates -- in; 1 the forward kernel's own (16x16x32).  The two sum the same piece products in different
 * orders; a pre-activation that is zero to rounding can be open in one and closed in the other (tests/test_gpu_parity.py bounds how many, and how large).  Process-wide. */
int probav_debug_hidden_from_forward_kernel(int on);

/* ---- plan report (parity tests), an addition made under ABI 7 ------------------------------------------------------------------------- */
/* Which kernel a single-operator call would launch, and the integers of its launch plan, from the very functions the launch paths call.  Host only: nothing
 * is launched and no device is needed.  tests/plan_cases.py names, per plan class, the geometry that reaches it; tests/test_gpu_plans.py holds each to the oracle.
 * probav_plan_conv: geom as probav_conv3d_forward; gated / has_skip: whether the call passes a gate (forward, backward-data: the input's; backward-filter: dY's)
 * / a skip tensor; op FORWARD = probav_conv3d_forward with a bias, BWD_DATA = the same without one (the engine's backward-data launches), WGRAD =
 * probav_conv3d_wgrad.  report[0] = the kernel (PROBAV_PLAN_NONE: the call is refused with PROBAV_EINVAL), [1] nsplit column ranges per row, [2] nstrips per
 * patch (row-tile kernels: tiles), [3] SR rows per strip (tile), [4] nslot ring depth (cw4, pp), [5] grid, [6] rvp staging items per thread (pp), [7] 0; a
 * field the kernel's plan does not have is 0.  DIRECT: a VALU kernel (the generic one, or the dedicated upscale pair).
 * probav_plan_pw: the fused pointwise pair, arguments as probav_pw_forward / probav_pw_backward; report[0] = the kernel, [7] = wps, the waves per sample of
 * pw_bwd_w4_kernel (PW4), the rest 0. */
#define PROBAV_PLAN_NONE 0
#define PROBAV_PLAN_CW4 1            /* conv3_w4_kernel */
#define PROBAV_PLAN_PP 2             /* conv3_pp_kernel */
#define PROBAV_PLAN_PSTRIP 3         /* conv3_pstrip_kernel */
#define PROBAV_PLAN_STRIP 4          /* conv3_strip_kernel */
#define PROBAV_PLAN_ROWTILE 5        /* conv3_mfma_kernel, any arithmetic */
#define PROBAV_PLAN_DIRECT 6
#define PROBAV_PLAN_WG4 7            /* conv3_wgrad_w4_kernel */
#define PROBAV_PLAN_WGRAD_X6 8       /* conv3_wgrad_x6_kernel, X6 arithmetic */
#define PROBAV_PLAN_WGRAD_X6_H3 9    /* conv3_wgrad_x6_kernel, H3 arithmetic */
#define PROBAV_PLAN_WGRAD_MFMA 10    /* conv3_wgrad_mfma_kernel */
#define PROBAV_PLAN_PW4 20           /* pw_bwd_w4_kernel */
#define PROBAV_PLAN_PW_X6_H3 21      /* pw_bwd_x6_kernel, H3 arithmetic */
#define PROBAV_PLAN_PW_X6 22         /* pw_fwd_x6_kernel / pw_bwd_x6_kernel, X6 arithmetic */
#define PROBAV_PLAN_PF4 23           /* pw_fwd_w4_kernel */
#define PROBAV_PLAN_PW_H3K 24        /* pw_fwd_h3k_kernel */
#define PROBAV_PLAN_PW_MFMA 25       /* pw_fwd_mfma_kernel / its backward */
#define PROBAV_PLAN_OP_FORWARD 0
#define PROBAV_PLAN_OP_BWD_DATA 1
#define PROBAV_PLAN_OP_WGRAD 2
int probav_plan_conv(const int32_t geom[17], int impl, int gated, int has_skip, int op, int32_t report[8]);
int probav_plan_pw(int64_t nvox, int64_t vox_per_sample, int D, int impl, int backward, int32_t report[8]);

/* ---- the general matrix route (csrc/kernels_gemm.hip), additions made under ABI 7 ------------------------------------------------------ */
/* Every tuned kernel above exists for the shipped channel counts (32 filters, expansion 8, 25 channels behind the decay convolution); at any other
 * count the engine falls to the generic direct (VALU) kernels.  The general matrix route runs those launches -- convolution forward / backward-data
 * and backward-filter, 1x1x1 and 3x3x3, any Cin and Cout -- as implicit GEMMs on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: the direct kernels'
 * arithmetic, an exact fp32 fma chain, on the matrix cores).  It is a SWITCH on the engine, off by default, kept apart from the kernel family:
 * probav_engine_set_impl keeps it.  With it on, at family >= 1, a launch goes to the route exactly when it would otherwise run the generic direct
 * kernel on a geometry that kernel's own callers do not call exotic (5x5x5, mirrored depth pads, zero pads above 2, mirrored pads above 1 stay
 * direct, unless the fourth switch below, probav_engine_set_gemm_exotic, hands them over) -- nothing a matrix, split-operand or dedicated small kernel (upscale pair, one-channel input, fused residual path, the tuned one-channel
 * backward-filter) serves changes hands; family 0 is the direct kernels with or without it.  The backward-filter's slab regions differ in size, so
 * probav_workspace_bytes / probav_workspace_split change with the switch: size the buffers after setting it.  Results of a sample do not depend on
 * its batch mates and are bitwise reproducible; they differ from the direct kernels' by fp32 rounding (another order of additions).
 * PROBAV_GEMM_ROUTE (set, non-zero) at probav_engine_create turns it on, as PROBAV_IMPL chooses the family.                                  */
int probav_engine_set_gemm_route(probav_engine* e, int on);
int probav_engine_gemm_route(const probav_engine* e);      /* 1 / 0 */
/* The single operators: arguments as probav_conv3d_forward / probav_conv3d_wgrad without `impl`.  A geometry the route does not take (see above; the
 * backward-filter takes pads <= 1 only) is refused with PROBAV_EINVAL and nothing is written; probav_gemm_conv3d_wgrad_scratch_bytes is 0 for it.
 * A scratch smaller than probav_gemm_conv3d_wgrad_scratch_bytes: PROBAV_ENOSPACE, nothing written.                                           */
int probav_gemm_conv3d_forward(const int32_t geom[17], const float* x, const float* gate, const float* w,
                               const float* bias, const float* skip, float* y, void* stream);
size_t probav_gemm_conv3d_wgrad_scratch_bytes(const int32_t geom[17]);
int probav_gemm_conv3d_wgrad(const int32_t geom[17], const float* x, const float* dy, const float* gate,
                             float* dw, float* db, void* scratch, size_t scratch_bytes, void* stream);
/* probav_plan_conv for an engine with the route ON (host only): PROBAV_PLAN_GEMM / PROBAV_PLAN_WGRAD_GEMM where that engine's launch of the
 * geometry goes to the route, probav_plan_conv's report everywhere else (refusals of impl included).
 * GEMM: report[1] = tiles along Cout, [2] = tiles along the output voxels, [3] = voxels per tile, [4] = output channels per tile, [5] = grid =
 *   [1] x [2], [6] = input channels per K chunk, [7] = K chunks per filter tap.
 * WGRAD_GEMM: report[1] = slabs (a function of the geometry alone, never of the device), [2] = voxels per slab, [3] x [4] = the Cin x Cout tile of
 *   a workgroup, [5] = grid = slabs x taps x tiles; the scratch is [1] x 4 x (taps Cin Cout + Cout) bytes.                                     */
#define PROBAV_PLAN_GEMM 11          /* gemm_conv_fwd_kernel */
#define PROBAV_PLAN_WGRAD_GEMM 12    /* gemm_conv_wgrad_kernel */
int probav_plan_conv_gemm(const int32_t geom[17], int impl, int gated, int has_skip, int op, int32_t report[8]);
/* The launches of ONE training step of `batch` patches (forward with training != 0, then backward) by route, from the functions the passes route
 * with (host only): counts[0] convolution launches (forward, backward-data, the recomputed hidden tensor) on the generic direct kernel, [1] on the
 * general matrix route, [2] backward-filter launches on the generic direct kernel, [3] on the route.  Launches of the matrix, split-operand and
 * dedicated small kernels and of the fused residual path / pointwise pair are not counted.                                                     */
int probav_engine_route_counts(const probav_engine* e, int batch, int32_t counts[4]);
/* The same four counts of what the engine's passes have ACTUALLY launched since the last reset, incremented where the launches are issued: after one
 * training step they equal probav_engine_route_counts (tests/test_gpu_gemm_route.py holds the census to them).  reset != 0 clears them after the read.  */
int probav_engine_launched_counts(probav_engine* e, int32_t counts[4], int reset);
/* The route's fused pointwise pair (csrc/kernels_gemm_pw.hip; host-only entry points, additions made under ABI 7).  On the route a residual block's
 * expConv -> ReLU -> decConv runs as separate launches whose hidden tensor ([voxels][F x expRate]) passes through memory: written and read once in
 * the forward pass, recomputed, written and read again with its gradient in the reverse pass.  A SECOND SWITCH, off by default, fuses the pair into
 * one launch each way for F <= 64 filters, D <= 64 decay channels and any hidden count: the hidden tile stays in registers, and the workspace loses
 * its three hidden-sized tensors (H of the saved state, Hb and dH of the reverse scratch) for one slab region per block -- size the buffers after
 * setting it.  It takes effect exactly when the family is >= 1, the route is on, the shape has no tuned pair (the shipped 32 -> 256 -> D <= 26 keeps its
 * own, whatever the switches) and the shape is in range; everywhere else the wish is kept and changes nothing.  probav_engine_set_impl and
 * probav_engine_set_gemm_route keep the wish; PROBAV_GEMM_PAIR (set, non-zero) at probav_engine_create sets it.
 * Forward results are those of the un-fused route BIT FOR BIT (each element is the same k-ordered fp32 fma chain); the reverse pass recomputes the
 * hidden tile with that chain (the forward's ReLU gates), sums dX in a fixed order per voxel and the weight gradients over slabs whose count follows
 * from the voxel count alone: reproducible, a sample independent of its batch mates, gradients equal to the un-fused route's to fp32 rounding.
 * A switch flipped between a training forward and its backward is refused by the backward (PROBAV_EINVAL, nothing written).  The launch census
 * (probav_engine_route_counts) does not count the fused pair: per block [1] drops by 5 and [3] by 2.
 * probav_debug_hidden serves the general fused pair in every family >= 1.                                                                       */
int probav_engine_set_gemm_pair(probav_engine* e, int on);
int probav_engine_gemm_pair(const probav_engine* e);       /* the wish: 1 / 0 */
int probav_engine_pair_kind(const probav_engine* e);       /* what the engine runs now: 0 un-fused, 1 the tuned fused pair, 2 the general fused pair */
/* The general pair's launch plan, from the functions its launches call: report[0] = voxels per workgroup tile (0: shape not supported, all zero),
 * [1] = tiles, [2] = hidden channels per chunk, [3] = chunks, [4] = workgroups of the launch (backward: the input-gradient kernel's tiles + slabs x
 * groups of eight chunks of the weight-gradient kernel), [5] = slabs and [6] = voxels per slab (backward only; functions of nvox alone), [7] = 0.   */
int probav_plan_pw_gemm(int F, int H, int D, int64_t nvox, int backward, int32_t report[8]);
/* The route on the 16-bit matrix pipe (csrc/kernels_gemm_x6.hip; host-only entry points, additions made under ABI 7).  The route's un-fused launches
 * above evaluate their products on v_mfma_f32_32x32x2_f32.  A THIRD SWITCH, off by default, runs every CONVOLUTION launch that conv_route hands to the
 * route -- forward, backward-data and the reverse pass's recomputed expConv, 1x1x1 and 3x3x3, any Cin and Cout -- in x6 arithmetic instead: each fp32 operand cut into three
 * bf16 truncation pieces, the six largest piece products on v_mfma_f32_32x32x16_bf16, smallest terms first, fp32 accumulation (the arithmetic of the
 * family-3 kernels: no operand scaling, no amax slots, no dependence on dynamic range).  Nothing else changes hands: the route's BACKWARD-FILTER stays
 * fp32 (an x6 form of it was measured slower than gemm_conv_wgrad_kernel: INTEGRATION.md, 'The general matrix route'), the fused pair stays fp32, tuned,
 * split-operand, dedicated and VALU launches stay where they are, family 0 never sees the switch.  Tiles and grids are the fp32 route's and no scratch
 * is involved, so probav_workspace_bytes / probav_workspace_split and probav_engine_route_counts do not move with the switch.
 * It takes effect exactly when the family is >= 1, the route is on and the wish is set (probav_engine_gemm_arith); probav_engine_set_impl,
 * probav_engine_set_gemm_route and probav_engine_set_gemm_pair keep the wish; PROBAV_GEMM_X6 (set, non-zero) at probav_engine_create sets it.
 * Results are reproducible bit for bit, a sample does not depend on its batch mates, and they differ from the fp32 route's by rounding (each product to
 * about 2^-24 relative).  With the switch on, pair on and pair off no longer give the same forward bits: the un-fused 1x1x1 launches are then x6 and the
 * pair is fp32; both are held to the oracle.  The recomputed expConv of the reverse pass must take the forward's gates, so a switch flipped between a
 * training forward and its backward is refused by the backward (PROBAV_EINVAL, nothing written) -- whenever probav_engine_gemm_arith differs between the
 * two, also on a network none of whose launches are the route's (the shipped one): the refusal is the engine state's, as the pair's is.        */
int probav_engine_set_gemm_x6(probav_engine* e, int on);
int probav_engine_gemm_x6(const probav_engine* e);         /* the wish: 1 / 0 */
int probav_engine_gemm_arith(const probav_engine* e);      /* what the route's convolution launches run now: 0 fp32, 1 x6 */
/* The x6 launch's plan for a geometry the route takes (host only), in the shape of probav_plan_conv_gemm's GEMM report: report[0] =
 * PROBAV_PLAN_GEMM_X6 (op forward / backward-data), [1..7] as there.  All zero (PROBAV_PLAN_NONE) for a geometry the route's kernel does not
 * take, and for op backward-filter, which has no x6 kernel (probav_plan_conv_gemm reports the fp32 one).                                       */
#define PROBAV_PLAN_GEMM_X6 13       /* gemm_conv_fwd_x6_kernel */
int probav_plan_conv_gemm_x6(const int32_t geom[17], int gated, int has_skip, int op, int32_t report[8]);
/* The route's exotic launches (host-only entry points, additions made under ABI 7).  The switches above leave what conv_route / wgrad_route call EXOTIC
 * on the generic direct kernels: a mirrored depth pad, kernel size 5, mirrored H/W pads of 2, zero pads above 2 and, for the backward-filter, any pad
 * above 1.  Only the 19-frame network (the reference's ConvReduceAndUpscaleEx) has such launches: forward and backward-filter of its reducers 1-4 (a
 * 5x5x5 layer on a pad of 2 mirrored on H, W and T; 3x3x3 layers on mirrored pads (2,2,1), (2,2,0), (2,2,0)) and the backward-data of the 5x5x5 layer, a
 * zero-pad correlation with pads of 4 -- five convolution and four backward-filter launches per step.  A FOURTH SWITCH, off by default, hands them to
 * the route's kernels: the same gemm_conv_fwd_kernel / gemm_conv_fwd_x6_kernel (following probav_engine_gemm_arith) and gemm_conv_wgrad_kernel (fp32),
 * through wider support predicates -- k x k x k and k x k x 1 for k in {1, 3, 5}; zero pads up to k - 1 per axis (backward-filter: up to 2); mirrored
 * H/W pads and a mirrored depth pad up to 2, each on an extent above the pad.  A tap on zero padding (the pads-of-4 backward-data) is multiplied by
 * its zero, not skipped, as elsewhere on the route; the mirrored layers have no zero padding.  The route does not report amax: where the neighbours
 * are H3 kernels (family 4 at 32 filters) the engine fills the output's slots behind the launch, as for the route's other launches.
 * It takes effect exactly when the family is >= 1, the route is on and the wish is set; probav_engine_set_impl, probav_engine_set_gemm_route,
 * probav_engine_set_gemm_pair and probav_engine_set_gemm_x6 keep the wish; PROBAV_GEMM_EXOTIC (set, non-zero) at probav_engine_create sets it.  On an
 * engine without exotic launches (7, 9 and 13 frames) nothing moves.  At 19 frames probav_engine_route_counts becomes {0, +5, 0, +4} and the four
 * backward-filter slab regions change size (slabs x (taps Cin Cout + Cout) floats, taps up to 125), so probav_workspace_bytes /
 * probav_workspace_split change with the switch: size the buffers after setting it.  A switch flipped between a training forward and its backward
 * is refused by the backward (PROBAV_EINVAL, nothing written), as for the pair and x6.  Results are reproducible bit for bit and a sample does
 * not depend on its batch mates; they differ from the direct kernels' by fp32 rounding.                                                         */
int probav_engine_set_gemm_exotic(probav_engine* e, int on);
int probav_engine_gemm_exotic(const probav_engine* e);     /* the wish: 1 / 0 */
/* The route's launch plans for a wide geometry, from the functions the launches call.  geom[17] has no field for the mirrored depth pad: reflect_t
 * states it.  op forward / backward-data: probav_plan_conv_gemm's GEMM report, report[0] = PROBAV_PLAN_GEMM (x6 == 0) or PROBAV_PLAN_GEMM_X6; op
 * backward-filter: its WGRAD_GEMM report (x6 ignored: the backward-filter is fp32).  All zero for a geometry the wide predicates refuse (k = 7, a pad
 * above k - 1, a mirrored pad of 3 or one not below its extent).  probav_gemm_wgrad_wide_scratch_bytes: the backward-filter's scratch, slabs x 4 x
 * (taps Cin Cout + Cout) bytes, 0 for a refused geometry.  probav_gemm_conv3d_* and probav_plan_conv_gemm* above answer what they always did.    */
int probav_plan_conv_gemm_wide(const int32_t geom[17], int reflect_t, int x6, int op, int32_t report[8]);
size_t probav_gemm_wgrad_wide_scratch_bytes(const int32_t geom[17], int reflect_t);

/* ---- dataset builder (utils/dataGenerator.py; proba-v_amd/prep.py), additions of ABI 7 ------------------------------------------------ */
/* Frames are one flat [n_frames][H][W] array; a ragged list of image sets is that array plus set_offsets[n_sets+1] (int64, ascending,
 * set_offsets[0] = 0).  Masks are uint8, nonzero = set.  Kernels and the registration error bound: csrc/kernels_prep.hip.
 * counts[i] = number of nonzero bytes of data[i*chunk_len .. (i+1)*chunk_len): count_nonzero of every QM / SM frame, or of every patch's
 * mask                                    replaces the per-frame / per-patch list comprehensions of utils/dataGenerator.py:381, 490, 632, 761 */
int probav_prep_count_nonzero(const uint8_t* data, int64_t n_chunks, int64_t chunk_len, int32_t* counts, void* stream);
/* Registers every 128 x 128 uint16 frame against its set's reference frame ref_frame[set] (an index into frames, chosen by the caller).
 * shifts [n_frames][2] (y, x as skimage reports them: indices > 64 wrapped to negative), reg_frames = np.roll(frame, shift), reg_masks =
 * np.roll(mask != 0, shift) as 0/1, reg_counts = their count of ones.  The shift is the argmax of the EXACT integer circular
 * cross-correlation, ties to the first index in C order; the reference frame itself gets shift 0.  spec_scratch: n_sets * 128 * 128 * 2
 * floats.  Preconditions (device arrays, so not checked on the host): set_offsets[0] = 0, non-decreasing, set_offsets[n_sets] = n_frames,
 * and set_offsets[s] <= ref_frame[s] < set_offsets[s+1] (no empty set).  A frame whose set breaks them is not read or written: its shift
 * is {PROBAV_PREP_BAD_SHIFT, PROBAV_PREP_BAD_SHIFT} (probav.prep raises on it).
 *                                         replaces registerImagesInSet / registerFrame(tech='freq')   utils/dataGenerator.py:616-678 */
#define PROBAV_PREP_BAD_SHIFT (-2147483647 - 1)
int probav_prep_register(const uint16_t* frames, const uint8_t* masks, const int64_t* set_offsets, int n_sets, int64_t n_frames,
                         const int32_t* ref_frame, float* spec_scratch, int32_t* shifts, uint16_t* reg_frames, uint8_t* reg_masks,
                         int32_t* reg_counts, void* stream);
/* Diagnostic of the registration: for pair = {ref, img} ([2][128][128] uint16) the fp32 correlation surface e[128][128] the kernel ranks
 * shifts by (of the frames offset by their floor means c_ref, c_img) and info[4] = {B, c_ref, c_img, max e}: B bounds |e - exact| at every
 * shift.  spec_scratch: 128 * 128 * 2 floats.                      (utils/dataGenerator.py:669, skimage register_translation) */
int probav_prep_xcorr_surface(const uint16_t* pair, float* spec_scratch, float* surface, double* info, void* stream);
/* Reflect pad by `pad` (np.pad 'reflect'), then every win x win window at `stride`, row-major: frames [S][T][H][W] fp32 and masks [S][T][H][W]
 * uint8 -> patches [S][P][T][win][win], patch_masks (0/1) the same, counts [S][P][T] = ones of each patch mask, P = nh * nw,
 * nh = (H + 2 pad - win) / stride + 1.  HR: pad 0, window = stride = 48.
 *                                         replaces the pad + generatePatches of utils/dataGenerator.py:107-171, 553-596 */
int probav_prep_patches(const float* frames, const uint8_t* masks, int S, int T, int H, int W, int pad, int win, int stride, float* patches,
                        uint8_t* patch_masks, int32_t* counts, void* stream);
/* Cloud-aware registration (csrc/kernels_prep_masked.hip): every 128 x 128 uint16 frame against its set's reference frame by a masked
 * normalised correlation over the window [-window, window]^2 of integer shifts, 1 <= window <= 32 (otherwise PROBAV_EINVAL, nothing
 * launched).  For a shift s, over the pixels p that are clear in the reference and whose source p - s lies inside the frame and is clear
 * in the frame (nothing wraps): the exact integer moments n, Sa, Sb, Saa, Sbb, Sab of a = ref[p], b = frame[p - s], num = n Sab - Sa Sb,
 * da = n Saa - Sa^2, db = n Sbb - Sb^2 (int64, all below 2^61) and v = double(num) / sqrt(double(da) * double(db)) in four correctly
 * rounded fp64 operations.  A shift is a candidate when 10 n >= 3 max_s n, da > 0 and db > 0; the largest v wins, ties to the first shift
 * with dy outer, both ascending.  shifts [n_frames][2] = (dy, dx); registered [n_frames] = 1, or 0 where no shift is a candidate (then the
 * shift is (0, 0)).  out_frames[p] = frame[reflect(p - s)] (scipy.ndimage 'reflect': d c b a | a b c d), out_masks[p] = (mask[p - s] != 0)
 * inside the frame and 0 outside, out_counts = its count of ones.  A set's reference frame is copied through (shift 0, registered 1).
 * Preconditions and their PROBAV_PREP_BAD_SHIFT marking as probav_prep_register; no scratch.  The statement the kernel equals bit for bit:
 * probav_amd.prep.register_masked_numpy.
 *                                         the counterpart of registerFrame(tech='time')                utils/dataGenerator.py:663-666 */
int probav_prep_register_masked(const uint16_t* frames, const uint8_t* masks, const int64_t* set_offsets, int n_sets, int64_t n_frames,
                                const int32_t* ref_frame, int window, int32_t* shifts, uint8_t* registered, uint16_t* out_frames,
                                uint8_t* out_masks, int32_t* out_counts, void* stream);
/* Refined quality masks (csrc/kernels_refine.hip): the pixels of co-registered uint16 frames [n_frames][H][W] (any H, W >= 1) that the
 * quality masks call clear but that lie far from the temporal median of their set's clear looks are taken out of the masks.  Per set
 * (frames x[t], clear c[t] = masks != 0, t < T) and per pixel, all in integers:
 *     sat[t] = c[t] and saturation >= 0 and x[t] > saturation;  c'[t] = c[t] and not sat[t];  n = #c'
 *     med = the clear values' element (n - 1) / 2 in ascending order (the lower median);  d[t] = |x[t] - med|
 *     mad = the element (n - 1) / 2 of the clear d in ascending order;  s = max(mad, floor_dn)
 *     o[t] = c'[t] and n >= min_clear and 16 d[t] > k16 s        (strict; 16 d < 2^20 and k16 s < 2^26: int32)
 *     pixel_masks [n_sets][3][H][W] uint64, bit t = frame t of the set: plane 0 = c, plane 1 = sat, plane 2 = o
 *                                                                (an output, and the second launch's input; bits T .. 63 are zero)
 *     g[t][p] = any (sat | o)[t][q] over |q - p|_inf <= dilate, q inside the frame (nothing wraps or reflects)
 *     out_masks[t] = c[t] and not g[t] (0/1);  out_counts[t] = its ones;  flagged[t] = {sum sat[t], sum o[t]} (before the dilation)
 * Host-known arguments outside their ranges return PROBAV_EINVAL and launch nothing: 0 <= k16 <= 1024, 0 <= floor_dn <= 65535,
 * 3 <= min_clear <= 64, 0 <= dilate <= 3, -1 <= saturation <= 65535 (-1: no saturation test), 1 <= max_set_len <= 64 (the longest set;
 * it sizes the LDS of the launch).  Preconditions on the device array as probav_prep_register: set_offsets[0] = 0, non-decreasing,
 * set_offsets[n_sets] = n_frames, and here 1 <= set_offsets[s+1] - set_offsets[s] <= max_set_len.  A set that breaks them is neither
 * read nor written; each of its frames f has out_counts[f] = PROBAV_PREP_BAD_COUNT and flagged[f] = {PROBAV_PREP_BAD_COUNT,
 * PROBAV_PREP_BAD_COUNT} (probav.prep raises on it).  Frames are never changed; no scratch beside `pixel_masks` (24 n_sets H W bytes).  The statement the kernels
 * equal bit for bit: probav_amd.prep.refine_masks_numpy.
 *                                         the counterpart of nothing in the reference: its README names the radiometric half of the
 *                                         problem (LR frames are never clipped to their 14-bit depth) and leaves it there */
#define PROBAV_PREP_BAD_COUNT (-1)
int probav_prep_refine_masks(const uint16_t* frames, const uint8_t* masks, const int64_t* set_offsets, int n_sets, int64_t n_frames, int H, int W,
                             int max_set_len, int k16, int floor_dn, int min_clear, int dilate, int saturation, uint64_t* pixel_masks,
                             uint8_t* out_masks, int32_t* out_counts, int32_t* flagged, void* stream);

/* ---- scoring (evaluate.py; proba-v_amd/scoring.py), additions of ABI 7 ------------------------------------------------------------- */
/* The ESA PROBA-V shift-compensated clear PSNR of whole images; it replaces the reference's unfinished evaluate.py:76-87, which calls
 * Losses.shiftCompensatedcPSNR (models/loss.py:37-53) and so leaves HR unmasked.  Per image, SR and HR uint16 [S][S], mask uint8 [S][S]
 * (nonzero = clear pixel of HR), border b, L = S - 2b, P = SR[b:b+L, b:b+L]; for every shift (u, v) in [0, 2b]^2, row-major (k = u (2b+1) + v):
 *     d = HR[u:u+L, v:v+L] - P,  m = mask[u:u+L, v:v+L],  n = sum m,  s1 = sum m d,  s2 = sum m d^2          (exact integers)
 *     cMSE = (n s2 - s1^2) / n^2,  cPSNR = 10 log10(65535^2 / min cMSE), the first (u, v) attaining the minimum wins.
 * Kernels, exactness and cost model: csrc/kernels_score.hip.
 * moments [n_images][(2b+1)^2][3] int64 = (n, s1, s2) of every shift, exact.  Arrays are [n_images][S][S], contiguous.
 * 1 <= n_images <= 65535, 0 <= b <= 3, 2b < S <= 2048.                    evaluate.py:76-87, models/loss.py:37-53 (with HR masked) */
int probav_score_moments(const uint16_t* sr, const uint16_t* hr, const uint8_t* mask, int64_t n_images, int S, int border,
                         int64_t* moments, void* stream);
/* From the moments: per image cpsnr (fp64; +inf when min cMSE = 0), shift [2] = (u, v) of the first exact minimum of cMSE (n = 0 shifts
 * skipped), bias = s1 / n of that shift (mean of HR - SR over its clear pixels), n_clear = its n.  An image with n = 0 at every shift
 * gets cpsnr = bias = NaN, shift = (-1, -1), n_clear = 0.  n s2 - s1^2 is formed in 128-bit integers and shifts are compared exactly
 * (num_a n_b^2 < num_b n_a^2); only the winner's cMSE is rounded to fp64.                              evaluate.py:76-87, models/loss.py:37-53 */
int probav_score_select(const int64_t* moments, int64_t n_images, int border, double* cpsnr, int32_t* shift, double* bias,
                        int64_t* n_clear, void* stream);

/* The shift-compensated SSIM (cSSIM) of whole images, the number published beside the cPSNR.  Images, mask, border, L, P and the shift
 * order as above; for every shift (u, v), all in fp64:
 *     H = HR[u:u+L, v:v+L],  m = mask[u:u+L, v:v+L] as 0/1,  n = sum m,  s1 = sum m (H - P)    (the exact integers of probav_score_moments)
 *     bias = s1 / n                                              (one fp64 division; n = 0: the shift is skipped, its value is NaN)
 *     x = m (P + bias),  y = m H                                 (masked pixels are zero on BOTH sides, as the published implementations do)
 *     g[j] = exp(-(j - 5)^2 / (2 * 1.5^2)), j = 0..10, divided by their sum: gauss11, 11 doubles computed by the caller and read as data
 *     F(a)[i, j] = sum_{p, q} g[p] g[q] a[i+p, j+q], "valid": K x K outputs, K = L - 10
 *     mx = F(x)  my = F(y)  vx = F(x x) - mx^2  vy = F(y y) - my^2  cxy = F(x y) - mx my,   C1 = (0.01 * 65535)^2,  C2 = (0.03 * 65535)^2
 *     ssim(u, v) = mean over the K^2 windows of ((2 mx my + C1)(2 cxy + C2)) / ((mx^2 + my^2 + C1)(vx + vy + C2))
 * A window that sees only masked pixels contributes exactly 1.  table [n_images][(2b+1)^2] fp64 = ssim(u, v), NaN where n = 0.  moments:
 * the output of probav_score_moments for the same arguments.  scratch: probav_ssim_scratch_bytes(n_images, S, border) bytes (0 for an
 * unsupported shape; PROBAV_ENOSPACE when scratch_bytes is smaller), one slot per workgroup and shift: no floating-point atomics, and an
 * entry is a pure function of the image's crops (the same bits for any batch, position or run; equal crops give equal bits).
 * 1 <= n_images <= 65535, 0 <= b <= 3, 2b + 11 <= S <= 2048.  Shape, exactness and cost model: csrc/kernels_ssim.hip; the statement the
 * kernel is held to: probav_amd.scoring.cssim_table_numpy. */
size_t probav_ssim_scratch_bytes(int64_t n_images, int S, int border);
int probav_ssim_table(const uint16_t* sr, const uint16_t* hr, const uint8_t* mask, const int64_t* moments, const double* gauss11,
                      int64_t n_images, int S, int border, void* scratch, size_t scratch_bytes, double* table, void* stream);
/* From the table: per image cssim = the largest entry that is not NaN, shift [2] = (u, v) of the FIRST entry attaining it; every entry
 * NaN: cssim = NaN, shift = (-1, -1). */
int probav_ssim_select(const double* table, int64_t n_images, int border, double* cssim, int32_t* shift, void* stream);

/* ---- batch augmentation (proba-v_amd/augment.py), an addition of ABI 7 ------------------------------------------------------------- */
/* One launch builds a training batch from the device-resident UN-augmented patches: lr [n_base][H][H][T][C] fp32, hr [n_base][S][S] fp32,
 * mask [n_base][S][S] uint8 (copied as bytes).  recipe [batch][3 + T] int32, row b = {i, f, k, perm[0..T)}: base sample i, flip code f
 * (0 none, 1 axis 0, 2 axis 1, 3 both), k counter-clockwise quarter turns, frame permutation perm.  In numpy terms, on one sample:
 *     lr_b[b] = rot90(flip(lr[i][:, :, perm], FL[f]), k)    hr_b[b] = rot90(flip(hr[i], FL[f]), k)    mask_b[b] likewise
 * (flip first, then rotate).  Outputs lr_b [batch][H][H][T][C], hr_b / mask_b [batch][S][S]; bits are moved, never computed with.
 * A row with i outside [0, n_base), f or k outside 0..3 or a perm entry outside [0, T) is skipped (its outputs are left as they were):
 * nothing is read outside the base arrays.  1 <= T <= 64, 1 <= C <= 16, H, S <= 1024 and one sample of each tensor must fit 64 KiB of
 * LDS beside a row table.  Kernel: csrc/kernels_augment.hip.
 *                                         replaces augmentByShufflingLRImgs / augmentByFlipping / augmentByRotating and the 320 x data
 *                                         set they materialise                                        utils/dataGenerator.py:227-273 */
int probav_augment_batch(const float* lr, const float* hr, const uint8_t* mask, int64_t n_base, int H, int T, int C, int S,
                         const int32_t* recipe, int64_t batch, float* lr_b, float* hr_b, uint8_t* mask_b, void* stream);

/* ---- test-time self-ensemble (proba-v_amd/ensemble.py), additions of ABI 7 ---------------------------------------------------------- */
/* E(x) = (1 / V) sum_v G_v^-1( round( clip( net(A_v(x)), lo, hi ) ) ): the mean over V variants of one patch, every member clipped and rounded
 * before the mean as resolveBySampleAveraging does through resolve (test.py:137-146), with flips and quarter turns beside its frame orders.
 * A variant is a recipe row {i, f, k, perm[0..T)} in the convention of probav_augment_batch; row n V + v is variant v of base patch n.
 * Kernels: csrc/kernels_ensemble.hip.
 *
 * Expand: lr [n_base][H][H][T][C] fp32, recipe [rows][3 + T] int32 -> out [rows][H][H][T][C], out[b] = rot90(flip(lr[i][:, :, perm], FL[f]), k):
 * the LR tensor of probav_augment_batch alone (same limits, same skipping of a row that points outside the base array).   test.py:137-146 */
int probav_ensemble_expand(const float* lr, int64_t n_base, int H, int T, int C, const int32_t* recipe, int64_t rows, float* out, void* stream);
/* Reduce: sr [n_base V][S][S] fp32 (raw network output), recipe [n_base V][3 + T] ->
 *     out[n] = (1 / V) sum_{v < V} flip(rot90(rint(clip(sr[n V + v], lo, hi)), -k_v), FL[f_v])        (rint: half to even, as probav_clip_round)
 * summed in fp32 for v = 0 .. V - 1 (exact: 1 <= V <= 256 members of at most 2^16), divided once by V with the correctly rounded fp32
 * division, and rounded half to even once more when final_round != 0.  grid = 0: out [n_base][S][S]; grid = g >= 1: the stitched images
 * [n_base / g^2][g S][g S] of test.py:149-160 (patch n is block ((n / g) % g, n % g) of image n / g^2; n_base a multiple of g^2).
 * PROBAV_EINVAL, nothing launched: V outside 1..256, S over 90 (a prediction and its accumulator must fit 64 KiB of LDS), lo > hi.
 * A base patch with an f or k outside 0..3 among its rows is skipped (its output is left as it was).                   test.py:137-146 */
int probav_ensemble_reduce(const float* sr, const int32_t* recipe, int64_t n_base, int V, int T, int S, float lo, float hi, int final_round,
                           int grid, float* out, void* stream);

/* ---- overlapped-tile inference (proba-v_amd/tiles.py), an addition of ABI 7 ------------------------------------------------------------- */
/* The blend of overlapping tile predictions into whole images ('Overlapped tiles').  sr [n_images n n][S][S] fp32: the
 * predictions of the n x n tiles of every image in row-major order, raw network output or members that are already rounded; tile (a, c) has
 * its origin at (a hr_stride, c hr_stride).  w [S] int32, device: a window of positive integers, W2[i][j] = w[i] w[j].  For every pixel (y, x) of
 * out [n_images][G][G], G = (n - 1) hr_stride + S, over the tiles t = (a, c) that cover it, with p = rint(clip(sr, lo, hi)) (rint: half to
 * even, as probav_clip_round):
 *     N = sum_t W2[y - o_a][x - o_c] p_t[y - o_a][x - o_c],  D = sum_t W2[y - o_a][x - o_c],  out[y][x] = N / D rounded half to even
 * in exact 64-bit integer arithmetic (q = floor(N / D); q + 1 when 2 (N - q D) > D, or == D and q odd).  Nothing is floating point after the
 * rint, so the image does not depend on the launch, and with hr_stride = S it is the plain stitch of test.py:149-160.
 * Range: at most ceil(S / hr_stride)^2 <= S^2 tiles cover a pixel, so |N| <= S^2 max(w)^2 max|p|.  The callers keep every w[i] in [1, 1024]
 * (tiles.py checks the window before it is uploaded; the library cannot see device memory) and p in [0, 2^16]: with S <= 90, S^2 < 2^13 and
 * |N| < 2^13 2^20 2^16 = 2^49, far below 2^63.  In general S^2 max(w)^2 max(|lo|, |hi|) must stay below 2^62.
 * PROBAV_EINVAL, nothing launched: a null pointer, n_images, n or S below 1, hr_stride outside 1..S (a gap between tiles would leave D = 0),
 * lo > hi, clip bounds beyond +-2^24 (the result is stored as fp32), G over 32767.  Kernel: csrc/kernels_tile.hip.
 *                                         replaces reconstruct_from_patches for overlapping tiles         test.py:149-160 */
int probav_tile_blend(const float* sr, const int32_t* w, int64_t n_images, int n, int S, int hr_stride, float lo, float hi, float* out, void* stream);

/* ---- bicubic-mean baseline (proba-v_amd/baseline.py), an addition of ABI 7 --------------------------------------------------------------- */
/* The competition's baseline ('Bicubic-mean baseline'): every LR frame of an image set upscaled 3 x by the Keys cubic
 * (a = -1/2, half-pixel centres, clamped indices) and the chosen frames averaged, in exact integer arithmetic.  frames uint16 and clear
 * uint8 (nonzero = clear pixel) are [n_frames][H][W]; set_offsets [n_sets + 1] as above.  HR index Y reads the LR rows
 * clamp(i0 - 1 .. i0 + 2, 0, H - 1), i0 = floor((Y - 1) / 3), with the weights over 27 of the phase (Y - 1) mod 3:
 *     0: (0, 27, 0, 0)      1: (-2, 21, 9, -1)      2: (-1, 9, 21, -2)
 * columns likewise; U_f[Y][X] = sum_ij wy_i wx_j frame_f[row_i][col_j], an integer over 729.
 * mode PROBAV_BASELINE_ESA: the frames of a set whose clear count equals the set's largest, all ties included (K per set);
 * mode PROBAV_BASELINE_CLEAR: at HR pixel (Y, X) the frames with clear[f][Y / 3][X / 3] set, or every frame of the set where none is (K per pixel).
 *     N = sum_f U_f,  D = 729 K,  out = clip(N / D rounded half to even, 0, 65535)     (floor division, 2 (N mod D) against D, ties to even)
 * out [n_sets][3 H][3 W] fp32 holding integers; k_used [n_sets] = K (esa) or the set's frame count (clear).  counts_scratch: int32
 * [n_frames], the caller's; it receives every frame's clear count in esa mode and is not touched in clear mode.  Nothing is floating point
 * and nothing is atomic, so the image does not depend on the launch.  H, W >= 1; 3 H, 3 W <= 2^20; sets of 1 .. 4096 frames
 * (N stays below 4096 * 65535 * 1089 < 2^39).  Preconditions on the device array as probav_prep_register: set_offsets[0] = 0,
 * set_offsets[n_sets] = n_frames, every set of 1 .. 4096 frames; a set that breaks them is not read or written and gets
 * k_used = PROBAV_BASELINE_BAD_SET (probav_amd.baseline raises on it).  PROBAV_EINVAL, nothing launched: a null pointer, scale != 3,
 * an unknown mode, a size outside the ranges above.  Kernel: csrc/kernels_baseline.hip; the statement it equals bit for bit:
 * probav_amd.baseline.baseline_numpy.
 *                                         replaces the unfinished bicubicMean / padding and the baseline upscaling it was meant to call
 *                                                                                                     evaluate.py:142-197, utils/utils.py:534-586 */
#define PROBAV_BASELINE_ESA 0
#define PROBAV_BASELINE_CLEAR 1
#define PROBAV_BASELINE_BAD_SET (-1)
int probav_baseline_upscale_mean(const uint16_t* frames, const uint8_t* clear, const int64_t* set_offsets, int n_sets, int64_t n_frames, int H, int W,
                                 int scale, int mode, int32_t* counts_scratch, float* out, int32_t* k_used, void* stream);

/* ---- frame-window ensemble (proba-v_amd/frame_windows.py), an addition of ABI 7 ---------------------------------------------------------- */
/* W predictions of every tile, each from another window of k frames slid over the tile's frames sorted from clearest to dirtiest, and their
 * weighted mean ('Frame windows').
 * Gather.  patches [N][T_pre][win][win] fp32 and counts [N][T_pre] int32 (masked pixels of every frame of the tile, 0 .. pixels = win^2):
 * the outputs of probav_prep_patches.  Per tile: frame t is eligible iff counts[t] < L (L = frame_windows.max_masked(pixels, threshold):
 * the builder's fp64 test turned into an integer one on the host); when none is, all T_pre are.  The E eligible frames ordered by (count
 * ascending, frame index ascending) are r[0 .. E); m = ceil(k / E); Q[i] = r[i / m] for i < E m, the dataset builder's tiled, sorted list;
 * window j < W takes Q[(j step + i) % (E m)], i < k.
 *     x      [N][W][win][win][k] fp32: x[n][j][y][x][i] = patches[n][sel[n][j][i]][y][x], copied bit for bit (test.py's transpose);
 *     sel    [N][W][k] int32: the frame indices;
 *     weight [N][W] int32: mode PROBAV_WINDOWS_CLEAR the sum over the window's k frames of (pixels - count), mode PROBAV_WINDOWS_UNIFORM 1;
 *            a tile whose weights are all 0 gets all 1.
 * (W - 1) step + k <= T_pre, so a tile whose frames are all eligible never wraps; W = 1 is exempt (one window is the builder's own choice, which
 * tiles a pool shorter than k).  One workgroup per tile stages the tile in LDS once:
 * T_pre planes of win^2 floats, each padded by up to 3, which must fit 160 KiB beside 1 KiB of tables (T_pre win^2 <= 40 960 floats at the most: win = 44 admits
 * T_pre <= 21).  PROBAV_EINVAL, nothing launched: a null pointer, N < 1, T_pre, W or k outside 1..64, step < 1, (W - 1) step + k > T_pre with W > 1,
 * L outside 0 .. win^2 + 1, an unknown mode, a tile that does not fit LDS.
 * Reduce.  sr [N W][S][S] fp32 (raw network output, or members that are already rounded), weight [N][W] int32, non-negative with a positive
 * sum per tile (what the gather writes); p = rint(clip(sr, lo, hi)) as probav_clip_round;
 *     out[n][y][x] = (sum_j weight[n][j] p[n W + j][y][x]) / (sum_j weight[n][j])   rounded half to even
 * in exact 64-bit integer arithmetic (floor division, 2 (N mod D) against D, ties to the even quotient): out [N][S][S] fp32 holding integers.
 * Range: weight < 2^31, p <= 2^24, W <= 64: sums below 2^61 (the gather's weights are at most k pixels: below 2^46 at the shipped sizes).
 * A tile whose weights sum to 0 or less breaks the precondition and gets 0.  PROBAV_EINVAL, nothing launched: a null pointer, N or S below 1,
 * W outside 1..64, lo > hi or a NaN bound, clip bounds beyond +-2^24.  Kernels: csrc/kernels_windows.hip; the statements they equal bit for
 * bit: probav_amd.frame_windows.frame_windows_select_numpy / _gather_numpy / _reduce_numpy.
 *                                         the "sliding window over the LR frames sorted from clearest to dirtiest" of the reference's
 *                                         ideas to try; the frame choice is removeAndReplaceDirtyFrames'     utils/dataGenerator.py:326-551 */
#define PROBAV_WINDOWS_CLEAR 0
#define PROBAV_WINDOWS_UNIFORM 1
int probav_frame_windows_gather(const float* patches, const int32_t* counts, int64_t N, int T_pre, int win, int k, int L, int W, int step, int mode,
                                float* x, int32_t* weight, int32_t* sel, void* stream);
int probav_frame_windows_reduce(const float* sr, const int32_t* weight, int64_t N, int W, int S, float lo, float hi, float* out, void* stream);

/* ---- random crops (proba-v_amd/crops.py), additions of ABI 7 ----------------------------------------------------------------------------- */
/* Training samples cut at arbitrary origins out of registered scenes that stay on the device ('Random crops'), instead of
 * the fixed grid of patches that stages 3 to 5 of the dataset builder dump.  Kernels: csrc/kernels_crops.hip; the statements they equal bit
 * for bit: probav_amd.crops.window_counts_numpy / crop_batch_numpy.
 *
 * Window counts.  masks uint8 [M][H][W] (nonzero = masked) -> counts int32 [M][ny][nx]: counts[m][a][c] = the masked pixels of rows
 * a stride .. a stride + win - 1 and columns c stride .. c stride + win - 1 of mask m padded by `pad` on every side as np.pad(..., 'reflect')
 * pads it; ny = (H + 2 pad - win) / stride + 1, nx likewise.  Exact integers, no atomics.  The validity table of every crop origin is
 * the HR masks with pad 0, win = scale P, stride = scale.  PROBAV_EINVAL, nothing launched: a null pointer, M < 1, H or W outside 1..32767,
 * pad outside 0 .. min(H, W) - 1, win outside 1 .. min(1024, H + 2 pad, W + 2 pad), stride outside 1..1024, 64 (W + 2 pad) bytes of column sums
 * over the 160 KiB of LDS. */
int probav_window_counts(const uint8_t* masks, int64_t M, int H, int W, int pad, int win, int stride, int32_t* counts, void* stream);
/* Crop batch.  Scenes: lr fp32 and lr_mask uint8 (nonzero = masked) [n_scenes][T_pre][H][H]; hr fp32 and hr_clear (one byte per pixel,
 * 1 = clear) [n_scenes][scale H][scale H].  positions int32 [n_positions][3] = {scene, y, x}, 0 <= y, x <= H - P; recipe int32
 * [batch][3 + k] = {j, f, q, perm[0..k)}: position j, then flip code f and q quarter turns in the convention of probav_augment_batch.
 * Per row, with the LR window = rows y .. y + win - 1, columns x .. x + win - 1 of the scene reflect-padded by `pad` (data and mask alike):
 *     counts[t] = masked pixels of frame t of the window; Q = window 0 of probav_frame_windows_gather's list for (counts, k, L);
 *     sel  [batch][k] int32:              sel[b][i] = Q[i]
 *     lr_b [batch][win][win][k] fp32:     rot90(flip(W, FL[f]), q) of W[y][x][i] = frame Q[perm[i]] of the LR window
 *     hr_b [batch][S][S] fp32, S = scale P: the same flip and turns of rows scale y .. scale y + S - 1, columns scale x .. of hr
 *     mask_b [batch][S][S]:               likewise of hr_clear
 * copied bit for bit.  A row with j outside [0, n_positions), f or q outside 0..3, a perm entry outside [0, k), or whose position lies
 * outside the scenes is skipped (its outputs are left as they were); callers validate recipes on the host.  Every output byte has one
 * writer.  PROBAV_EINVAL, nothing launched: a null pointer, a count below 1, T_pre or k outside 1..64, P outside 1..H, pad outside 0 .. H - 1,
 * win outside P .. min(P + 2 pad, 1024), scale outside 1..64 or scale P over 1024, L outside 0 .. win^2 + 1, or a sample (k LR windows, or the HR
 * window, beside a row table) that does not fit the 160 KiB of LDS. */
int probav_crop_batch(const float* lr, const uint8_t* lr_mask, const float* hr, const uint8_t* hr_clear, int64_t n_scenes, int T_pre, int H,
                      int P, int pad, int win, int scale, int k, int L, const int32_t* positions, int64_t n_positions, const int32_t* recipe,
                      int64_t batch, float* lr_b, float* hr_b, uint8_t* mask_b, int32_t* sel, void* stream);

/* ---- FuseNet (proba-v_amd/fusenet_numpy.py), additions of ABI 7 --------------------------------------------------------------------------- */
/* The reference's stitching network (models/modelsTF.py:391-474, FuseNetv3; INTEGRATION.md, 'FuseNet').  x [batch][H][W] fp32 (raw DN);
 * flat = conv2d/kernel [48][48][1][64] | conv2d/bias [64] | instance_normalization/gamma [64] | beta [64], flat_count = 147648.
 *     y[b][r][s][c] = sum_{i,j < 48} x[b][r+i-23][s+j-23] kernel[i][j][0][c]      zero outside the image (TF 'SAME': 23 before, 24 after).  The bias
 *                     is NOT added: it cancels in y - mu below, so no kernel reads it and its gradient is exact zeros
 *     stats[b][c]   = (mu, 1 / sqrt(var + 1e-3)): mean and biased variance of y[b][.][.][c] over the H W pixels
 *     m[b][r][s]    = (1/64) sum_c l,  l = a if a >= 0 else 0.3 a,  a = gamma[c] (y - mu) / sqrt(var + 1e-3) + beta[c]
 *     out           = x + m (residual != 0), or m
 * y [batch][H][W][64] and stats [batch][64][2] are outputs of the forward and inputs of the backward.  Backward: g = d loss / d out
 * [batch][H][W] -> dflat [147648] = d loss / d flat (bias part: zeros).  No d loss / d x.  Arithmetic: the fp32-input MFMA (an fp32 fma
 * chain); every cross-thread reduction is fp64 in a fixed order, no floating-point atomics, so the bits depend on the arguments only and a
 * sample's y, stats and m do not depend on its batch.  workspace: probav_fusenet_workspace_bytes(batch, H, W, backward) bytes (0 for an
 * unsupported shape), written and read inside one call.  PROBAV_EINVAL, nothing launched: a null pointer, batch, H or W < 1, batch > 65535,
 * H or W > 32768, batch H W 64 >= 2^31, flat_count != 147648, a workspace smaller than the query's answer, or flat / y / stats / workspace not
 * 16-byte aligned.  Kernels: csrc/kernels_fusenet.hip. */
size_t probav_fusenet_workspace_bytes(int batch, int H, int W, int backward);
int probav_fusenet_forward(const float* x, const float* flat, int64_t flat_count, int batch, int H, int W, int residual, float* out, float* y,
                           float* stats, void* workspace, size_t workspace_bytes, void* stream);
int probav_fusenet_backward(const float* g, const float* x, const float* y, const float* stats, const float* flat, int64_t flat_count, int batch,
                            int H, int W, float* dflat, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
